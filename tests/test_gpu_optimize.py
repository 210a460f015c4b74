"""The posterior mode on the MI355X (potus_optimize, k_opt_lbfgs: batched L-BFGS, one workgroup per path) against the CPU reference of
tests/optimize_ref.py (scipy L-BFGS on the oracle, polished by Newton-CG), against potus_log_prob_grad and potus_constrain of the same
handle, and against stand-alone handles for the data sets of a potus_set_datasets_ex handle.

Bounds.  A path that ends ABSGRAD has ||g||_2 < tol_grad in the device's arithmetic; the oracle's gradient there may differ by the gap
between the two implementations, which each test measures at that point.  With -Hessian >= lambda I between two points,
||a - b|| <= ||g(a) - g(b)|| / lambda <= (||g(a)|| + ||g(b)||) / lambda: lambda is the reference's lambda_min times 0.95 (the Hessian
moves over a 1e-4 neighbourhood) on the small designs and exactly 1 on the no-mode variant (prior = identity, likelihood PSD)."""
import ctypes as C
import re

import numpy as np
import pytest

import lbfgs_ref
import optimize_ref as ref
from conftest import GOLD
from oracle_lib import OracleModel
from us_potus_model_amd import _abi, dataprep, synthetic, timeline
from us_potus_model_amd.sampler import Handle, PotusError, PotusModel

pytestmark = pytest.mark.gpu
OPTS = dict(seed=1843, cus_per_chain=1, twin=0)
TIGHT = dict(tol_obj=0.0, tol_rel_obj=0.0, tol_grad=1e-4, tol_rel_grad=0.0, tol_param=0.0, iter=5000)
LOOSE = dict(TIGHT, tol_grad=1e-2)
VARIANTS = ("full", "no_mode_adjustment")
ABSGRAD, MAXIT, INIT = 3, 6, 8


def raw(res):
    return b"".join(np.ascontiguousarray(res[k]).tobytes() for k in ("q", "lp", "grad_norm", "return_code", "iterations", "grad_evals"))


def status_of(fn):
    try:
        fn()
    except PotusError as e:
        return int(re.search(r"error (\d+)", str(e)).group(1))
    return 0


@pytest.fixture(scope="module")
def small():
    """Per variant: a plain handle, the four starts (zeros and three U(-2, 2) rows) and the results of ONE call per Jacobian setting."""
    out = {}
    for v in VARIANTS:
        data = synthetic.small(v)
        h = Handle(data, v, chains=1, **OPTS)
        q0 = np.vstack([np.zeros(h.D), np.random.default_rng(20161108).uniform(-2, 2, (3, h.D))])
        q0.setflags(write=False)
        res = {j: h.optimize(q0, jacobian=j, cols=(0, h.n_cols), **TIGHT) for j in (0, 1)}
        out[v] = dict(data=data, h=h, q0=q0, res=res, irho=ref.rho_index(data, v))
    yield out
    for v in VARIANTS:
        out[v]["h"].close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("jacobian", [0, 1])
def test_reaches_the_mode(small, variant, jacobian):
    s, r = small[variant], ref.small_reference(variant, bool(jacobian))
    h, res, obj = s["h"], s["res"][jacobian], r["obj"]
    print(variant, jacobian, "codes", res["return_code"], "iterations", res["iterations"], "evaluations", res["grad_evals"], "||g||", res["grad_norm"])
    assert (res["return_code"] == ABSGRAD).all() and (res["grad_norm"] < 1e-4).all()
    lp, g = h.log_prob_grad(res["q"])
    g_ref_norm = np.linalg.norm(obj.grad(r["q"]))
    for p in range(4):
        g_gpu = g[p] if jacobian else ref.remove_jacobian(lp[p], g[p], res["q"][p], s["irho"])[1]
        assert abs(np.linalg.norm(g_gpu) - res["grad_norm"][p]) <= 1e-9 * res["grad_norm"][p]
        g_or = obj.grad(res["q"][p])
        gap = np.linalg.norm(g_gpu - g_or)
        dist = np.linalg.norm(res["q"][p] - r["q"])
        bound = (np.linalg.norm(g_or) + g_ref_norm) / (0.95 * r["lambda_min"])
        print(f"  path {p}: oracle ||g|| {np.linalg.norm(g_or):.3e}, gap {gap:.3e}, ||q - q_ref|| {dist:.3e} <= {bound:.3e}")
        assert np.linalg.norm(g_or) <= 1e-4 + gap
        assert dist <= bound


def test_jacobian_setting(small):
    f, n = small["full"], small["no_mode_adjustment"]
    rho = [1.0 / (1.0 + np.exp(-f["res"][j]["q"][0, f["irho"]])) for j in (0, 1)]
    print("rho_e_bias without / with the Jacobian:", rho)
    assert raw(f["res"][0]) != raw(f["res"][1]) and rho[0] - rho[1] > 0.01     # (0.6815 against 0.6673 on the oracle)
    assert raw(n["res"][0]) == raw(n["res"][1]) and n["res"][0]["rows"].tobytes() == n["res"][1]["rows"].tobytes()


@pytest.mark.parametrize("variant", VARIANTS)
def test_lp_out(small, variant):
    s = small[variant]
    for j in (0, 1):
        res = s["res"][j]
        lp, g = s["h"].log_prob_grad(res["q"])
        if j:
            assert lp.tobytes() == res["lp"].tobytes()
        else:
            want = np.array([ref.remove_jacobian(lp[p], g[p], res["q"][p], s["irho"])[0] for p in range(4)])
            assert np.all(np.abs(want - res["lp"]) <= 1e-12 * np.abs(want))


@pytest.mark.parametrize("variant", VARIANTS)
def test_determinism_and_batching(small, variant):
    s = small[variant]
    h, q0 = s["h"], s["q0"]
    again = h.optimize(q0, jacobian=0, cols=(0, h.n_cols), **TIGHT)
    assert raw(again) == raw(s["res"][0]) and again["rows"].tobytes() == s["res"][0]["rows"].tobytes()
    few = dict(iter=25)                                                   # bytes must agree wherever a path stops
    both = h.optimize(q0[1:], **few)
    lib = h.optimize(None, 3, **few)
    assert np.isfinite(lib["q"]).all() and np.abs(lib["q"]).max() < 50 and raw(lib) != raw(both)
    one_lib = h.optimize(None, 1, path_offset=0, **few)
    for p in range(3):
        a = h.optimize(q0[1 + p:2 + p], path_offset=p, **few)
        b = h.optimize(None, 1, path_offset=p, **few)
        for k in ("q", "lp", "grad_norm", "return_code", "iterations", "grad_evals"):
            assert a[k].tobytes() == both[k][p:p + 1].tobytes(), (p, k)
            assert b[k].tobytes() == lib[k][p:p + 1].tobytes(), (p, k)
    assert raw(one_lib) == raw(h.optimize(None, 1, **few))
    assert lib["q"][0].tobytes() != lib["q"][1].tobytes()


def three_dates():
    """synthetic.small with three run dates that keep different polls and have different priors (timeline.mask builds each date's data)."""
    data = synthetic.small("full")
    Ns, Nn, S = int(data["N_state_polls"]), int(data["N_national_polls"]), int(data["S"])
    rng = np.random.default_rng(3)
    keep_s = np.stack([rng.uniform(size=Ns) < 0.5, rng.uniform(size=Ns) < 0.8, np.ones(Ns, bool)])
    keep_n = np.stack([rng.uniform(size=Nn) < 0.5, rng.uniform(size=Nn) < 0.8, np.ones(Nn, bool)])
    prior = np.tile(np.asarray(data["mu_b_prior"], dtype=np.float64), (3, 1))
    prior[0] += np.linspace(-0.3, 0.4, S)
    prior[1] -= 0.1
    return timeline.design_of(data, keep_s, keep_n, prior, np.full(3, float(data["mu_b_T_scale"])))


def test_data_sets_equal_stand_alone_handles():
    design = three_dates()
    h = Handle(design["data"], "full", chains=3, **OPTS)
    timeline.set_design(h, design)
    q0 = np.random.default_rng(9).uniform(-2, 2, (6, h.D))
    few = dict(iter=40, jacobian=1)
    many, many_lib = h.optimize(q0, cols=(0, h.n_cols), **few), h.optimize(None, 6, cols=(0, h.n_cols), **few)
    assert status_of(lambda: h.optimize(q0[:4])) == 1                  # 4 paths over 3 data sets
    assert status_of(lambda: h.constrain(q0[:1])) != 0                 # (what row_out is there for)
    a, b, _ = h.layout["predicted_score"]
    for p in range(6):
        g = Handle(timeline.data_of(design, p // 2), "full", chains=1, **OPTS)
        for m, one in ((many, g.optimize(q0[p:p + 1], cols=(0, h.n_cols), **few)), (many_lib, g.optimize(None, 1, path_offset=p, cols=(0, h.n_cols), **few))):
            for k in ("q", "lp", "grad_norm", "return_code", "iterations", "grad_evals", "rows"):
                assert one[k].tobytes() == m[k][p:p + 1].tobytes(), (p, k)
        g.close()
    assert np.isfinite(many["rows"][:, 7:]).all() and (many["iterations"] > 0).all()
    for d in (1, 2):
        assert np.abs(many["rows"][0, a:b] - many["rows"][2 * d, a:b]).max() > 1e-3
    # a plain potus_set_datasets handle: the outcomes differ, the path picks its data set's
    hp = Handle(design["data"], "full", chains=2, **OPTS)
    ys = np.stack([np.asarray(design["data"]["n_democrat_state"]), np.asarray(design["data"]["n_democrat_state"]) // 2])
    yn = np.stack([np.asarray(design["data"]["n_democrat_national"])] * 2)
    hp.set_datasets(ys, yn)
    r2 = hp.optimize(q0[:2], **few)
    g = Handle(design["data"], "full", chains=1, **OPTS)
    assert g.optimize(q0[:1], **few)["q"].tobytes() == r2["q"][:1].tobytes() and g.optimize(q0[1:2], **few)["q"].tobytes() != r2["q"][1:2].tobytes()
    for x in (g, hp, h):
        x.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_rows(small, variant):
    s = small[variant]
    h = s["h"]
    for j in (0, 1):
        res = s["res"][j]
        rows = res["rows"]
        assert rows.shape == (4, h.n_cols)
        assert rows[:, 0].tobytes() == res["lp"].tobytes() and np.isnan(rows[:, 1:7]).all()
        assert np.ascontiguousarray(rows[:, 7:]).tobytes() == h.constrain(res["q"]).tobytes()
        a, b, _ = h.layout["predicted_score"]
        part = h.optimize(s["q0"], jacobian=j, cols=(a, b), **TIGHT)["rows"]
        assert part.tobytes() == np.ascontiguousarray(rows[:, a:b]).tobytes()


@pytest.mark.parametrize("variant", VARIANTS)
def test_limits_and_failed_starts(small, variant):
    s = small[variant]
    h, q0 = s["h"], s["q0"]
    lp0, g0 = h.log_prob_grad(q0)
    lp_start = np.array([ref.remove_jacobian(lp0[p], g0[p], q0[p], s["irho"])[0] for p in range(4)])
    r3 = h.optimize(q0, iter=3)
    assert (r3["return_code"] == MAXIT).all() and (r3["iterations"] == 3).all() and (r3["lp"] > lp_start).all()
    assert (r3["grad_evals"] >= 4).all() and (r3["grad_evals"] <= 1 + 3 * 20).all()
    bad = q0.copy()
    bad[2, 5] = np.nan
    rb = h.optimize(bad, iter=3, cols=(0, 8))
    assert rb["return_code"][2] == INIT and np.isnan(rb["q"][2]).all() and np.isnan(rb["lp"][2]) and np.isnan(rb["grad_norm"][2])
    for p in (0, 1, 3):
        for k in ("q", "lp", "grad_norm", "return_code", "iterations", "grad_evals"):
            assert rb[k][p].tobytes() == r3[k][p].tobytes(), (p, k)
    # defaults: the code and the iteration count of the state machine in numpy (tests/lbfgs_ref.py) on the handle's own log_prob_grad with the
    # Jacobian removed -- RELGRAD on the oracle (tests/test_optimize_host.py) -- and further than three iterations get
    rd = h.optimize(q0)
    print(variant, "defaults: codes", rd["return_code"], "iterations", rd["iterations"], "||g||", rd["grad_norm"])

    def fun(q):
        lp, g = h.log_prob_grad(q)
        return ref.remove_jacobian(float(lp[0]), g[0], q, s["irho"])
    want = [lbfgs_ref.LBFGS(fun).run(q0[p]) for p in range(4)]
    assert all(st["rec"].clearance >= lbfgs_ref.CLEAR_MIN for w in want for st in w["steps"])
    assert rd["return_code"].tolist() == [w["code"] for w in want] and rd["iterations"].tolist() == [w["iterations"] for w in want]
    assert (rd["lp"] > r3["lp"]).all()


def test_refusals_and_an_undisturbed_run(small):
    s = small["full"]
    h, q0, data = s["h"], s["q0"], s["data"]
    ARG, UNSUP = 1, 6
    assert status_of(lambda: h.optimize(None, 0)) == ARG
    assert status_of(lambda: h.optimize(q0, history_size=0)) == ARG and status_of(lambda: h.optimize(q0, history_size=21)) == ARG
    assert status_of(lambda: h.optimize(q0, iter=0)) == ARG
    for t in ("tol_obj", "tol_rel_obj", "tol_grad", "tol_rel_grad", "tol_param"):
        assert status_of(lambda: h.optimize(q0, **{t: -1.0})) == ARG and status_of(lambda: h.optimize(q0, **{t: float("nan")})) == ARG, t
    for a in (0.0, -1.0, float("inf"), float("nan")):
        assert status_of(lambda: h.optimize(q0, init_alpha=a)) == ARG, a
    assert status_of(lambda: h.optimize(q0, jacobian=2)) == ARG
    assert status_of(lambda: h.optimize(q0, cols=(5, 5))) == ARG and status_of(lambda: h.optimize(q0, cols=(0, h.n_cols + 1))) == ARG
    L, o = h.L, h.optimize_opts()
    dp, n = C.POINTER(C.c_double), q0.shape[0]
    q, lp, info = np.zeros((n, h.D)), np.zeros(n), np.zeros((n, 3), np.int32)
    args = lambda qq, ll, ii: (h.h, C.byref(o), q0.ctypes.data_as(dp), n, qq, ll, None, ii, 0, 0, None)
    pq, pl, pi = q.ctypes.data_as(dp), lp.ctypes.data_as(dp), info.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.potus_optimize(*args(None, pl, pi)) == ARG and L.potus_optimize(*args(pq, None, pi)) == ARG and L.potus_optimize(*args(pq, pl, None)) == ARG
    assert L.potus_optimize(*args(pq, pl, pi)) == 0                       # gnorm_out may be NULL
    hk = Handle(data, "full", chains=1, seed=1843, cus_per_chain=2, twin=0)
    assert hk.cus_per_chain == 2 and status_of(lambda: hk.optimize(np.zeros((1, hk.D)))) == UNSUP
    hk.close()
    hd = Handle(data, "full", chains=1, seed=1843, cus_per_chain=1, twin=0, metric=_abi.METRICS["dense_e"])
    assert status_of(lambda: hd.optimize(np.zeros((1, hd.D)))) == UNSUP
    hd.close()
    # a sampling run with a refused and a successful call in its middle gives the bytes of an uninterrupted one
    run = dict(chains=2, num_warmup=20, num_samples=20, **OPTS)
    a, b = Handle(data, "full", **run), Handle(data, "full", **run)
    before = b.optimize(q0[:2], iter=10)                                  # before init
    for x in (a, b):
        x.init()
    a.run(40)
    b.run(20)
    assert status_of(lambda: b.optimize(q0, iter=0)) == ARG
    mid = b.optimize(q0[:2], iter=10)
    b.run(20)
    assert raw(before) == raw(mid) == raw(h.optimize(q0[:2], iter=10))
    assert a.draws().tobytes() == b.draws().tobytes() and a.chain_status() == b.chain_status()
    a.close()
    b.close()


def test_r_entry_point(small):
    s = small["full"]
    h, q0 = s["h"], s["q0"]
    n, D = q0.shape[0], h.D
    a, b, _ = h.layout["predicted_score"]
    want = h.optimize(q0, jacobian=1, iter=30, history_size=7, init_alpha=1e-2, path_offset=3, cols=(a, b))
    q, lp, gn, info, rows, st = np.zeros((n, D)), np.zeros(n), np.zeros(n), np.zeros((n, 3), np.int32), np.zeros((n, b - a)), (C.c_int * 1)(-1)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    o = h.optimize_opts()
    h.L.potus_R_optimize((C.c_int * 1)(h.h), (C.c_int * 7)(1, 7, 30, 3, n, 1, 1), (C.c_double * 6)(1e-2, o.tol_obj, o.tol_rel_obj, o.tol_grad, o.tol_rel_grad, o.tol_param),
                         dp(np.ascontiguousarray(q0)), dp(q), dp(lp), dp(gn), info.ctypes.data_as(C.POINTER(C.c_int)), (C.c_int * 2)(a, b), dp(rows), st)
    assert st[0] == 0
    got = dict(q=q, lp=lp, grad_norm=gn, return_code=info[:, 0], iterations=info[:, 1], grad_evals=info[:, 2])
    assert raw(got) == raw(want) and rows.tobytes() == want["rows"].tobytes()
    assert h.optimize_timing() > 0.0


def test_optimum_of_the_model_call(small):
    s = small["full"]
    opt = PotusModel("full").optimize(s["data"], jacobian=False, init=s["q0"], **TIGHT)
    assert np.ascontiguousarray(opt.q).tobytes() == s["res"][0]["q"].tobytes() and opt.codes == ["ABSGRAD"] * 4
    assert opt.best == int(np.argmax(opt.lp)) and opt.mle("lp__") == opt.lp[opt.best]
    S, T = int(s["data"]["S"]), int(s["data"]["T"])
    lay = s["h"].layout
    ps, mu = opt.mle("predicted_score"), opt.mle("mu_b")
    assert ps.shape == (T, S) and mu.shape == (S, T) and np.allclose(ps.T, 1.0 / (1.0 + np.exp(-mu)), rtol=0, atol=1e-12)
    row = s["res"][0]["rows"][opt.best]
    assert ps[T - 1, 2] == row[lay["predicted_score"][0] + (T - 1) + T * 2] and opt.mle("rho_e_bias") == row[lay["rho_e_bias"][0]]
    assert opt.as_inits(3).shape == (3, s["h"].D) and (opt.as_inits(3) == opt.q[opt.best]).all()
    opt.close()


@pytest.fixture(scope="module")
def real():
    """The committed 2012 (no-mode) and 2016 (full) data: four paths each on the device, one scipy run on the oracle's fast gradient."""
    out = {}
    for year, variant in (("2012", "no_mode_adjustment"), ("2016", "full")):
        data = dataprep.load_npz(GOLD / f"data_{year}.npz")["data"]
        h = Handle(data, variant, chains=1, **OPTS)
        q0 = np.vstack([np.zeros(h.D), np.random.default_rng(int(year)).uniform(-2, 2, (3, h.D))])
        a, b, _ = h.layout["predicted_score"]
        res = h.optimize(q0, cols=(a, b), **LOOSE)
        ms = h.optimize_timing()
        h.close()
        m, irho = OracleModel(data, variant), ref.rho_index(data, variant)

        class Fast:
            D = m.D

            @staticmethod
            def neg(q):
                lp, g = ref.remove_jacobian(*m.log_prob_grad(q, fast=True), q, irho)
                return -lp, -g
        q_ref, nit, nfev = ref.scipy_lbfgs(Fast, np.zeros(m.D))
        grad = (lambda m, irho: lambda q: ref.remove_jacobian(*m.log_prob_grad(q), q, irho)[1])(m, irho)     # (this year's model, not the loop's last)
        out[year] = dict(res=res, q_ref=q_ref, grad=grad, m=m, S=int(data["S"]), T=int(data["T"]), lay=(a, b), ms=ms, nit=nit)
    return out


def test_real_shapes_2012_strong_concavity(real):
    r = real["2012"]
    res = r["res"]
    print("2012: codes", res["return_code"], "iterations", res["iterations"], "evaluations", res["grad_evals"], "||g||", res["grad_norm"], "kernel ms", r["ms"],
          "scipy iterations", r["nit"])
    pts = [res["q"][p] for p in range(4)] + [r["q_ref"]]
    gn = [np.linalg.norm(r["grad"](q)) for q in pts]
    for i in range(5):
        for j in range(i):
            d = np.linalg.norm(pts[i] - pts[j])
            print(f"  {j}-{i}: ||q_a - q_b|| {d:.3e} <= {gn[i] + gn[j]:.3e}")
            assert d <= gn[i] + gn[j]


def test_real_shapes_2016_election_day(real):
    r = real["2016"]
    res, S, T = r["res"], r["S"], r["T"]
    print("2016: codes", res["return_code"], "iterations", res["iterations"], "evaluations", res["grad_evals"], "||g||", res["grad_norm"], "kernel ms", r["ms"],
          "scipy iterations", r["nit"])
    assert (res["return_code"] == ABSGRAD).all() and (res["grad_norm"] < 1e-2).all()
    score = res["rows"][:, T - 1::T]                                       # predicted_score is T x S column-major
    assert score.shape == (4, S)
    a, _ = r["lay"]
    want = r["m"].write_array(r["q_ref"])[a - 7:][T - 1::T][:S]
    print("  max |score - reference| per path", np.abs(score - want).max(axis=1), "spread across paths", np.ptp(score, axis=0).max())
    assert np.abs(score - want).max() <= 1e-5 and np.ptp(score, axis=0).max() <= 1e-5


def test_timeline_modes():
    data = dataprep.load_npz(GOLD / "data_2016.npz")["data"]
    full = timeline.load_fixture(GOLD / "timeline_2016.npz", data)
    design = timeline.design_of(data, full["keep_state"][:3], full["keep_national"][:3], full["mu_b_prior"][:3], full["mu_b_T_scale"][:3], full["run_dates"][:3])
    out = timeline.modes(design, "full", paths_per_date=1)
    S = int(data["S"])
    print("timeline.modes: codes", out["return_code"].ravel(), "iterations", out["iterations"].ravel(), "kernel ms", out["ms"])
    assert out["predicted_score"].shape == (3, 1, S) and out["q"].shape[:2] == (3, 1)
    assert ((out["return_code"] >= 1) & (out["return_code"] <= 5)).all() and list(out["best"]) == [0, 0, 0]
    assert np.abs(out["predicted_score"][0] - out["predicted_score"][2]).max() > 1e-4
    for d in range(3):
        opt = PotusModel("full").optimize(timeline.data_of(design, d), path_offset=d)
        assert opt.q.tobytes() == out["q"][d].tobytes() and opt.lp.tobytes() == out["lp"][d].tobytes()
        assert np.ascontiguousarray(opt.mle("predicted_score")[-1]).tobytes() == out["predicted_score"][d, 0].tobytes()
        opt.close()
