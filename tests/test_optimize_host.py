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


# ------------------------------------------------------------------------------------------------ the L-BFGS state machine (tests/lbfgs_ref.py)
# The reference of tests/test_gpu_lbfgs.py on the CPU oracle: its direction against a dense H, its accepted steps against the two Wolfe
# conditions, its end point against the mode -- and, for exactly the inputs the GPU tests use, which branches they reach, how far every
# comparison stays from its threshold and which code ends each path, so that the GPU tests are known to reach what they claim.
import functools
from collections import Counter

import lbfgs_ref as lb

MARGIN = 1e-4                     # asserted clearance of every comparison on the oracle: 1e5 x the 1e-9 below which the GPU tests would skip


@functools.lru_cache(maxsize=None)
def _objective(design, jacobian=True):
    data, variant = lb.designs()[design]
    return ref.Objective(data, variant, jacobian)


@pytest.mark.parametrize("m", lb.HISTORIES)
def test_two_loop_is_the_dense_h_times_g(m):
    """Before and after the ring wraps (2 m + 3 iterations, 43 for m = 20).  Bound: 2 e_ref (float64 against longdouble dot products) plus the
    dense form's own rounding -- two D-term matrix products per pair and the final H g: (2 n + 1) D eps A |g| with A >= |H| built from absolute
    values by the same formula."""
    obj = _objective("small_full")
    D = obj.D
    opt = lb.LBFGS(obj, history_size=m, **lb.OFF)
    st = opt.start(lb.starts(D)[0])
    worst, wrapped = 0.0, 0
    for l in range(2 * m + 3):
        step = opt.iterate(st)
        assert step["ok"] and not step["retried"]
        assert opt.accept(st, step["x"], step["f"], step["g"], step["rec"])[0] == 0
        n = st.history()
        assert n == min(l + 1, m)
        wrapped += l + 1 > m
        H, A = lb.dense_h(st.S, st.Y, st.gamma, D)
        e_ref = np.abs(st.d - lb.two_loop(st.g, st.S, st.Y, st.gamma, long=True))
        bound = 2.0 * e_ref + (2 * n + 1) * D * lb.EPS * (A @ np.abs(st.g))
        err = np.abs(st.d - H @ st.g)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (m, l, float((err / bound).max()))
        assert abs(st.gd - st.g @ H @ st.g) <= (2 * n + 3) * D * lb.EPS * (np.abs(st.g) @ A @ np.abs(st.g))
    print(f"history {m}: largest |two-loop - dense| / bound {worst:.3f}, {wrapped} iterations after the wrap")
    assert wrapped >= 3


def test_a_scaling_or_ring_error_would_show():
    """The dense form is independent enough to notice: gamma of the OLDEST pair, or the pairs in the ring's storage order after the wrap."""
    obj = _objective("small_full")
    opt = lb.LBFGS(obj, history_size=2, **lb.OFF)
    st = opt.start(lb.starts(obj.D)[0])
    for _ in range(5):
        step = opt.iterate(st)
        opt.accept(st, step["x"], step["f"], step["g"], step["rec"])
    H, _ = lb.dense_h(st.S, st.Y, st.gamma, obj.D)
    good = np.abs(st.d - H @ st.g).max()
    stale = float(st.S[0] @ st.Y[0]) / float(st.Y[0] @ st.Y[0])
    assert np.abs(lb.two_loop(st.g, st.S, st.Y, stale) - H @ st.g).max() > 1e6 * good
    assert np.abs(lb.two_loop(st.g, st.S[::-1], st.Y[::-1], st.gamma) - H @ st.g).max() > 1e6 * good


@functools.lru_cache(maxsize=None)
def _survey():
    """Every run the GPU tests make, on the oracle.  rows: (design, what, path) -> the result of LBFGS.run."""
    with np.errstate(all="ignore"):                         # (init_alpha = 1e300 sends the Jacobian's logarithms to infinity)
        return _survey_rows()


def _survey_rows():
    rows = {}
    for design in lb.designs():
        D = _objective(design).D
        q0 = lb.starts(D)
        for m in lb.HISTORIES:
            for ia in lb.INIT_ALPHAS:
                for p in range(2):
                    rows[design, f"replay m={m} alpha0={ia:g}", p] = lb.LBFGS(_objective(design), history_size=m, init_alpha=ia, iter=lb.ITER).run(q0[p])
        for jac in (True, False):
            obj = _objective(design, jac)
            cases = [("defaults", {}), ("maxit", dict(iter=lb.ITER)), ("lsfail", dict(init_alpha=1e300))] + [(f"iter={k}", dict(iter=k)) for k in (1, 2, 3)]
            if jac:
                cases += [(k, dict(lb.OFF, **t)) for k, t in lb.SINGLE.items()]
            for name, kw in cases:
                for p in range(2):
                    rows[design, f"{name} jacobian={int(jac)}", p] = lb.LBFGS(obj, **kw).run(q0[p])
        if design.startswith("small"):                      # tests/test_gpu_optimize.py::test_limits_and_failed_starts
            for p, x0 in enumerate(lb.default_starts(D)):
                rows[design, "defaults jacobian=0, the starts of test_gpu_optimize", p] = lb.LBFGS(_objective(design, False)).run(x0)
    d = lb.FLIP["design"]
    rows[d, "flip", 0] = lb.LBFGS(_objective(d), history_size=lb.FLIP["history_size"], init_alpha=lb.FLIP["init_alpha"], iter=lb.ITER).run(lb.flip_start(_objective(d).D))
    return rows


def test_branch_table_of_the_gpu_inputs():
    rows = _survey()
    table, ends = {}, Counter()
    for (design, what, p), r in rows.items():
        ends[r["code"]] += 1
        t = table.setdefault((design, what.split(" alpha0")[0] if what.startswith("replay") else what.split(" jacobian")[0]), Counter())
        for s in r["steps"]:
            t.update(s["rec"].branches)
    names = sorted({b for t in table.values() for b in t})
    print("branches reached, per design and kind of run (both paths, all initial steps):")
    for key, t in table.items():
        print(f"  {key[0]:13s} {key[1]:28s} " + " ".join(f"{b}={t[b]}" for b in names if t[b]))
    print("paths ended by code:", dict(sorted(ends.items())))
    total = Counter()
    for t in table.values():
        total.update(t)
    for b in lb.REACHABLE + ("zoom_near_flip",):
        assert total[b] > 0, b
    for design in lb.designs():                             # the strided loops' second trip sees every branch of the search too
        mine = Counter()
        for (d, _), t in table.items():
            if d == design:
                mine.update(t)
        need = lb.REACHABLE if design.endswith("full") else tuple(b for b in lb.REACHABLE if b not in ("nonfinite", "bisection"))
        assert all(mine[b] > 0 for b in need), (design, mine)
    for m in lb.HISTORIES:                                  # the ring wraps within the compared range
        assert all(rows[d, f"replay m={m} alpha0=1", p]["iterations"] >= min(m + 9, 29) for d in lb.designs() for p in range(2)), m
    for code in range(1, 8):
        assert ends[code] > 0, code
    for b in ("zoom_near", "retry_gradient", "skipped_pair", "history_reset"):      # (the module docstring of test_gpu_lbfgs.py says why)
        assert total[b] == 0, b


def test_clearances_of_the_gpu_inputs():
    """No comparison of any run the GPU tests make comes within MARGIN of its threshold on the oracle; in the single-tolerance runs the rule
    that fires is at least 1 % below its threshold and every earlier value at least 0.4 % above."""
    rows = _survey()
    worst = {}
    for (design, what, p), r in rows.items():
        for l, s in enumerate(r["steps"]):
            c = s["rec"].clearance
            if c < worst.get(design, (np.inf,))[0]:
                worst[design] = (c, what, p, l, s["rec"].closest)
            assert c >= MARGIN, (design, what, p, l, s["rec"].closest, c)
    for design, w in worst.items():
        print(f"  {design}: smallest clearance {w[0]:.2e} ({w[4]}; {w[1]}, path {w[2]}, iteration {w[3]})")
    for design in lb.designs():
        for c, (name, kw) in enumerate(lb.SINGLE.items(), start=1):
            thr = lb.LBFGS(None, **dict(lb.OFF, **kw)).thresholds()[name]
            for p in range(2):
                r = rows[design, f"{name} jacobian=1", p]
                assert r["code"] == c and 19 <= r["iterations"] <= 40, (design, name, p, r["code"], r["iterations"])
                q = [s["rules"][name] / thr for s in r["steps"]]
                print(f"  {design} {name} path {p}: ends at {r['iterations']}, fired at {q[-1]:.3f} of its threshold, earlier >= {min(q[:-1]):.3f}")
                assert q[-1] <= 0.99 and min(q[:-1]) >= 1.004
        for p in range(2):
            r = rows[design, "lsfail jacobian=1", p]
            assert (r["code"], r["iterations"], r["evals"]) == (lb.LSFAIL, 0, 21)
            assert rows[design, "maxit jacobian=1", p]["code"] == lb.MAXIT and rows[design, "defaults jacobian=1", p]["code"] == lb.RELGRAD


@pytest.mark.parametrize("design", ["small_full", "wide_nomode"])
def test_accepted_steps_satisfy_both_wolfe_conditions(design):
    """Recomputed from the run's own points in longdouble, not from the flags the search took its decision on."""
    obj = _objective(design)
    n = 0
    for what in ("replay m=5 alpha0=1", "replay m=1 alpha0=100", "replay m=20 alpha0=0.001", "defaults jacobian=1"):
        for p in range(2):
            r = _survey()[design, what, p]
            for l, s in enumerate(r["steps"]):
                x1 = r["x"][l] + s["alpha"] * s["d"]
                assert np.array_equal(x1, r["x"][l + 1])
                f1, g1 = obj(x1)
                gd0, dh = lb.dot(r["g"][l], s["d"], long=True), lb.dot(g1, s["d"], long=True)
                assert gd0 > 0 and lb.wolfe(r["f"][l], gd0, s["alpha"], f1, dh) == (True, True), (what, p, l)
                assert s["first_trial"] == (lb.DEFAULTS["init_alpha"] if "defaults" in what else float(what.split("alpha0=")[1])) if l == 0 else s["first_trial"] == 1.0
                n += 1
    assert n > 200


@pytest.mark.parametrize("variant,jacobian", [("full", False), ("full", True), ("no_mode_adjustment", False)])
def test_reference_state_machine_reaches_the_mode(variant, jacobian):
    """The defaults with tol_grad = 1e-4 alone: ABSGRAD, and the end point inside optimize_ref's strong-concavity bound of its mode."""
    r = ref.small_reference(variant, jacobian)
    obj = r["obj"]
    out = lb.LBFGS(obj, **dict(lb.OFF, tol_grad=1e-4)).run(np.zeros(obj.D))
    gn = np.linalg.norm(out["g"][-1])
    dist = np.linalg.norm(out["x"][-1] - r["q"])
    print(f"{variant} jacobian={jacobian}: code {out['code']} after {out['iterations']} iterations, {out['evals']} evaluations; ||g|| {gn:.2e}, ||q - q_ref|| {dist:.2e}")
    assert out["code"] == lb.ABSGRAD and gn < 1e-4
    assert dist <= (gn + r["gnorm"]) / (0.95 * r["lambda_min"])
