"""CPU tests of the Laplace approximation (potus_laplace): the reference the GPU tests compare with (tests/laplace_ref.py) agrees with
itself, the struct and its defaults are the header's, the names are where users look for them, and the entry points refuse without
touching a device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import laplace_ref as lref
import optimize_ref as oref
from us_potus_model_amd import _abi, sampler, synthetic

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("variant,jacobian", [("full", True), ("full", False), ("no_mode_adjustment", True)])
def test_oracle_differences_approach_autograd_and_then_flatten(variant, jacobian):
    """Central differences of the oracle gradient against autograd on the Stan transcription: truncation h^2 from 1e-3 to 1e-4, then the
    rounding of the gradient over 2 h takes over (measured: 1.2e-6, 1.2e-8, 3.5e-9 for the full variant with the Jacobian)."""
    r = lref.small_precision(variant, jacobian)
    err = [float(np.abs(lref.small_precision_fd(variant, jacobian, h) - r["P"]).max()) for h in (1e-3, 1e-4, 1e-5)]
    ev = np.linalg.eigvalsh(r["P"])
    print(f"{variant} jacobian={jacobian}: max|P_fd - P_autograd| at h = 1e-3, 1e-4, 1e-5: {err}; max|P| {np.abs(r['P']).max():.1f}; lambda {ev[0]:.4f} .. {ev[-1]:.1f}")
    assert np.array_equal(r["P"], r["P"].T)
    assert err[1] < err[0] / 20                                  # h^2: a factor of 100 in exact arithmetic
    assert err[2] < err[0] and err[2] < 1e-6 * np.abs(r["P"]).max()        # no longer falling by 100: rounding, still below the truncation at 1e-3
    assert err[2] > err[1] / 100
    assert abs(ev[0] - oref.small_reference(variant, jacobian)["lambda_min"]) < 1e-5
    if variant != "full":
        assert ev[0] >= 1.0 - 1e-9                                # prior = identity, likelihood positive semi-definite


def test_jacobian_term_changes_one_entry():
    a, b = lref.small_precision("full", True), lref.small_precision("full", False)
    i = oref.rho_index(a["data"], "full")
    # at one point the two differ in entry (rho, rho) by the Jacobian's second derivative 2 rho (1 - rho); the modes differ, so compare at one
    P0 = lref.precision_autograd(a["data"], "full", False, a["q"])
    d = a["P"] - P0
    rho = 1.0 / (1.0 + np.exp(-a["q"][i]))
    assert abs(d[i, i] - 2.0 * rho * (1.0 - rho)) < 1e-12
    d[i, i] = 0.0
    assert np.abs(d).max() < 1e-12 and np.abs(a["P"] - b["P"]).max() > 1e-4


def test_library_normals_are_standard_normal_and_keyed_by_draw():
    u = np.stack([lref.library_normals(1843, n, 101) for n in range(200)])
    assert u.shape == (200, 101) and abs(u.mean()) < 0.03 and abs(u.std() - 1.0) < 0.03
    assert not np.array_equal(u[0], u[1]) and np.array_equal(u[3], lref.library_normals(1843, 3, 101))
    assert np.array_equal(lref.library_normals(1843, 3, 100), u[3][:100])          # an odd D drops the pair's second half
    assert not np.array_equal(lref.library_normals(1844, 3, 101), u[3])


def test_log_ratio_of_the_reference():
    """What the issue measured on the CPU: sd 0.034 for the no-mode variant, 0.42-0.47 with max 3.4 for the full one (1 000 draws)."""
    u = np.random.default_rng(1).standard_normal((1000, 292))
    for variant, lo, hi in (("no_mode_adjustment", 0.02, 0.05), ("full", 0.35, 0.55)):
        r = lref.small_precision(variant, True)
        lr, X = lref.log_ratio(r["obj"], r["q"], r["P"], u[:, :r["obj"].D])
        print(f"{variant}: log ratio mean {lr.mean():.4f} sd {lr.std():.4f} max {lr.max():.3f}")
        assert lo < lr.std() < hi and abs(lr.mean()) < 0.1
        assert np.allclose((X @ r["P"] * X).sum(1), (u[:, :r["obj"].D] ** 2).sum(1), rtol=1e-10)     # x' P x = |u|^2


def test_opts_struct_and_defaults():
    assert C.sizeof(_abi.PotusLaplaceOpts) == 24
    L = sampler.load_library()
    o = _abi.PotusLaplaceOpts()
    C.memset(C.byref(o), 0xFF, 24)
    L.potus_default_laplace_opts(C.byref(o))
    assert (o.jacobian, o.draw_offset, o.pad0, o.pad1, o.h) == (1, 0, 0, 0, 1e-4)
    L.potus_default_laplace_opts(None)                    # a NULL struct is ignored
    assert _abi.LAPLACE_CODES == {0: "OK", 1: "NOT_PD", 2: "NOT_FINITE"}


def test_names_are_declared_exported_and_in_the_r_shim():
    hdr = (ROOT / "include" / "potus_hmc.h").read_text()
    shim = (ROOT / "R" / "potus_sampling.R").read_text()
    L = sampler.load_library()
    for name in ("potus_default_laplace_opts", "potus_laplace", "potus_laplace_write_array_device", "potus_laplace_scores_device", "potus_laplace_summary",
                 "potus_laplace_timing", "potus_R_laplace"):
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in sampler.EXPORTS and hasattr(L, name), name
    assert "typedef struct potus_laplace_opts" in hdr
    assert '.C("potus_R_laplace"' in shim and re.search(r"^potus_laplace <- function\(", shim, re.M)
    for name in ("laplace_opts", "laplace", "laplace_rows_device", "laplace_scores", "laplace_summary", "laplace_timing"):
        assert hasattr(sampler.Handle, name), name
    assert hasattr(sampler.PotusModel, "laplace") and hasattr(sampler, "Laplace")


def test_refusals_need_no_device():
    L = sampler.load_library()
    o = _abi.PotusLaplaceOpts()
    L.potus_default_laplace_opts(C.byref(o))
    q, info = np.zeros(4), np.zeros(4)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert L.potus_laplace(12345, C.byref(o), dp(q), 1, None, 0, None, None, None, dp(info), None) == 4     # POTUS_ERR_STATE: no such handle
    buf = C.create_string_buffer(256)
    L.potus_last_error(buf, 256)
    assert b"handle" in buf.value
    assert L.potus_laplace_timing(None) == 1              # POTUS_ERR_ARG
    assert L.potus_laplace_write_array_device(12345, 0, 1, None) == 4 and L.potus_laplace_scores_device(12345, 0, 1, None) == 4
    assert L.potus_laplace_summary(12345, 0, 1, None, 270, None, None, None, None) == 4
    st = (C.c_int * 1)(-1)
    L.potus_R_laplace((C.c_int * 1)(12345), (C.c_int * 6)(1, 0, 1, 0, 0, 0), (C.c_double * 1)(1e-4), dp(q), dp(q), dp(q), dp(q), dp(q), dp(info), dp(q), st)
    assert st[0] == 4


def test_python_side_argument_errors():
    """Handle.laplace checks shapes before the library sees a pointer; without a GPU there is no handle, so the checks run on a stand-in."""
    class Stub(sampler.Handle):
        def __init__(self):                               # no device, no library handle
            self.D, self.L = 5, sampler.load_library()
    s = Stub()
    with pytest.raises(ValueError, match="mode has shape"):
        s.laplace(np.zeros(4), 3)
    with pytest.raises(ValueError, match="u has shape"):
        s.laplace(np.zeros(5), 3, u=np.zeros((2, 5)))
    with pytest.raises(ValueError, match="u has shape"):
        s.laplace(np.zeros((2, 5)), 3, u=np.zeros((3, 5)))
    with pytest.raises(TypeError, match="unknown Laplace option"):
        s.laplace(np.zeros(5), 3, step=1e-3)
    with pytest.raises(TypeError, match="unknown Laplace option"):
        s.laplace_opts(pad0=1)
    with pytest.raises(sampler.PotusError, match="no Laplace draws"):
        s.laplace_scores()
    o = s.laplace_opts(h=1e-5, jacobian=0, draw_offset=7)
    assert (o.h, o.jacobian, o.draw_offset) == (1e-5, 0, 7)
    data = synthetic.small("full")
    opt = object.__new__(sampler.Optimum)
    opt.jacobian, opt.q, opt.best = False, np.zeros((1, 5)), 0
    with pytest.raises(ValueError, match="found with jacobian"):
        sampler.PotusModel("full").laplace(data, mode=opt, jacobian=True)
