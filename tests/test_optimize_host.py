"""CPU tests of the posterior mode (potus_optimize): the reference the GPU tests compare with (tests/optimize_ref.py) finds the mode
from two starts, the struct and its defaults are the header's, the names are where users look for them, and the entry points refuse
without touching a device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import optimize_ref as ref
from us_potus_model_amd import _abi, sampler

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("variant,jacobian", [("full", False), ("full", True), ("no_mode_adjustment", False)])
def test_reference_reaches_the_mode_from_two_starts(variant, jacobian):
    r = ref.small_reference(variant, jacobian)
    obj = r["obj"]
    assert r["gnorm"] <= 1e-10, r["gnorm"]
    q2, g2, nit, nfev = ref.reference_mode(obj, np.random.default_rng(11).uniform(-2, 2, obj.D))
    assert g2 <= 1e-10, g2
    lam = r["lambda_min"]
    print(f"{variant} jacobian={jacobian}: ||g|| {r['gnorm']:.2e} / {g2:.2e}, lambda_min {lam:.4f}, L-BFGS {r['iterations']} / {nit} iterations, "
          f"||q1 - q2|| {np.linalg.norm(q2 - r['q']):.2e}")
    assert lam > 0.9                                       # strictly concave at the mode (the no-mode variant: -Hessian >= I everywhere)
    if variant != "full":
        assert lam >= 1.0 - 1e-6
    # strong concavity around the mode: two points with these gradients cannot be further apart
    assert np.linalg.norm(q2 - r["q"]) <= (r["gnorm"] + g2) / (0.95 * lam)


def test_jacobian_moves_rho_only_in_the_full_variant():
    a, b = ref.small_reference("full", False), ref.small_reference("full", True)
    i = a["obj"].irho
    rho = [1.0 / (1.0 + np.exp(-r["q"][i])) for r in (a, b)]
    assert abs(rho[0] - rho[1]) > 1e-3, rho               # the Jacobian log(rho) + log(1 - rho) pulls rho towards 1/2
    assert ref.rho_index(a["data"], "no_mode_adjustment") is None


def test_remove_jacobian_is_the_derivative_of_what_it_subtracts():
    r = ref.small_reference("full", False)
    obj, i = r["obj"], r["obj"].irho
    q = np.random.default_rng(5).uniform(-1, 1, obj.D)
    lp1, g1 = obj.m.log_prob_grad(q)
    lp0, g0 = ref.remove_jacobian(lp1, g1, q, i)
    h = 1e-6
    e = np.zeros(obj.D)
    e[i] = h
    jac = lambda x: ref.remove_jacobian(0.0, np.zeros(obj.D), x, i)[0]           # minus the Jacobian terms
    assert abs((jac(q + e) - jac(q - e)) / (2 * h) - (g0[i] - g1[i])) < 1e-8
    assert np.array_equal(np.delete(g0, i), np.delete(g1, i))


def test_opts_struct_and_defaults():
    assert C.sizeof(_abi.PotusOptimizeOpts) == 64
    L = sampler.load_library()
    o = _abi.PotusOptimizeOpts()
    C.memset(C.byref(o), 0, 64)
    L.potus_default_optimize_opts(C.byref(o))
    assert (o.jacobian, o.history_size, o.iter, o.path_offset) == (0, 5, 2000, 0)
    assert (o.init_alpha, o.tol_obj, o.tol_rel_obj, o.tol_grad, o.tol_rel_grad, o.tol_param) == (1e-3, 1e-12, 1e4, 1e-8, 1e7, 1e-8)
    L.potus_default_optimize_opts(None)                    # a NULL struct is ignored


def test_names_are_declared_exported_and_in_the_r_shim():
    hdr = (ROOT / "include" / "potus_hmc.h").read_text()
    shim = (ROOT / "R" / "potus_sampling.R").read_text()
    L = sampler.load_library()
    for name in ("potus_default_optimize_opts", "potus_optimize", "potus_optimize_timing", "potus_R_optimize"):
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in sampler.EXPORTS and hasattr(L, name), name
    assert "typedef struct potus_optimize_opts" in hdr
    assert '.C("potus_R_optimize"' in shim and re.search(r"^potus_optimize <- function\(", shim, re.M)
    assert hasattr(sampler.Handle, "optimize") and hasattr(sampler.PotusModel, "optimize") and hasattr(sampler, "Optimum")
    from us_potus_model_amd import timeline
    assert callable(timeline.modes)


def test_refusals_need_no_device():
    L = sampler.load_library()
    o = _abi.PotusOptimizeOpts()
    L.potus_default_optimize_opts(C.byref(o))
    q, lp, gn, info = np.zeros(4), np.zeros(1), np.zeros(1), np.zeros(3, np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = L.potus_optimize(12345, C.byref(o), None, 1, dp(q), dp(lp), dp(gn), info.ctypes.data_as(C.POINTER(C.c_int32)), 0, 0, None)
    assert rc == 4                                         # POTUS_ERR_STATE: no such handle
    buf = C.create_string_buffer(256)
    L.potus_last_error(buf, 256)
    assert b"handle" in buf.value
    assert L.potus_optimize_timing(None) == 1              # POTUS_ERR_ARG
    st = (C.c_int * 1)(-1)
    L.potus_R_optimize((C.c_int * 1)(12345), (C.c_int * 7)(0, 5, 10, 0, 1, 0, 0), (C.c_double * 6)(1e-3, 0, 0, 1e-4, 0, 0), dp(q), dp(q), dp(lp), dp(gn),
                       info.ctypes.data_as(C.POINTER(C.c_int)), (C.c_int * 2)(0, 1), dp(q), st)
    assert st[0] == 4
