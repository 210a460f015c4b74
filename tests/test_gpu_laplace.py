"""The Laplace approximation on the MI355X (potus_laplace: k_lap_hess, k_lap_sym, the dense Cholesky, k_lap_solve_*, k_lap_lp) against
tests/laplace_ref.py (torch autograd on the Stan transcription, the oracle's central differences, numpy's Cholesky and scipy's triangular
solve, the oracle's Philox), against potus_log_prob_grad / potus_constrain of the same handle, and against stand-alone handles for the
data sets of a potus_set_datasets_ex handle.

Bounds.  The Hessian: the device and the oracle difference the same function with the same step rule, so the device's distance from autograd
is the oracle's truncation error (measured in the test) plus the gradient gap of the two implementations over 2 h: at most twice the
oracle's.  The draws: a backward-stable Cholesky + triangular solve of P has a forward error of order D eps kappa_2(P) |X|; the factor 8
covers the two factorisations compared (numpy's and the device's) and the blocked order of the sums; every term comes from P_dev in the test."""
import ctypes as C
import re

import numpy as np
import pytest
from scipy.linalg import solve_triangular

import laplace_ref as lref
import optimize_ref as oref
import outcomes_ref
import psis_ref
import timeline_ref
from us_potus_model_amd import _abi, synthetic, timeline
from us_potus_model_amd.outcomes import outcomes_of_block
from us_potus_model_amd.sampler import Handle, PotusError, PotusModel

pytestmark = pytest.mark.gpu
OPTS = dict(seed=1843, cus_per_chain=1, twin=0)
VARIANTS = ("full", "no_mode_adjustment")
EV = np.array([100, 90, 80, 70, 60, 138])
EPS = 2.0 ** -52
KEYS = ("q", "lp", "lp_approx", "return_code", "log_det", "grad_norm", "min_pivot")
N_SMALL = 37                                     # draws of the shared calls: one tile of 64, ragged


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """The accessors hand out torch tensors: torch's GPU runtime comes up before this module's first library call (as bench.py does)."""
    import torch
    torch.cuda.init()


def raw(res, keys=KEYS):
    return b"".join(np.ascontiguousarray(res[k]).tobytes() for k in keys)


def status_of(fn):
    try:
        fn()
    except PotusError as e:
        return int(re.search(r"error (\d+)", str(e)).group(1))
    return 0


@pytest.fixture(scope="module")
def small():
    """Per variant: a plain handle, a fixed u, and ONE call per Jacobian setting at the read-only mode of optimize_ref.small_reference."""
    out = {}
    for v in VARIANTS:
        data = synthetic.small(v)
        h = Handle(data, v, chains=1, **OPTS)
        u = np.random.default_rng(2).standard_normal((1, N_SMALL, h.D))
        u.setflags(write=False)
        res = {j: h.laplace(oref.small_reference(v, bool(j))["q"], N_SMALL, u=u, precision=True, jacobian=j) for j in (0, 1)}
        out[v] = dict(data=data, h=h, u=u, res=res)
    yield out
    for v in VARIANTS:
        out[v]["h"].close()


# ------------------------------------------------------------------------------------------------ 1. the Hessian
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("jacobian", [0, 1])
def test_hessian(small, variant, jacobian):
    s, r = small[variant], lref.small_precision(variant, bool(jacobian))
    res = s["res"][jacobian]
    P = res["precision"][0]
    assert res["return_code"][0] == 0 and P.shape == (s["h"].D, s["h"].D)
    assert np.array_equal(P, P.T)                                      # exactly symmetric
    bound = 2.0 * np.abs(lref.small_precision_fd(variant, bool(jacobian), 1e-4) - r["P"]).max()
    err = np.abs(P - r["P"]).max()
    ev_dev, ev_ref = np.linalg.eigvalsh(P), np.linalg.eigvalsh(r["P"])
    print(f"{variant} jacobian={jacobian}: max|P_dev - P_ref| {err:.3e} <= {bound:.3e}; max|P| {np.abs(P).max():.1f}; "
          f"lambda_min {ev_dev[0]:.6f} (ref {ev_ref[0]:.6f}), lambda_max {ev_dev[-1]:.4f} (ref {ev_ref[-1]:.4f}); ||g|| at the mode {res['grad_norm'][0]:.2e}")
    assert err <= bound
    assert abs(ev_dev[0] - ev_ref[0]) <= bound and abs(ev_dev[-1] - ev_ref[-1]) <= bound
    assert res["grad_norm"][0] < 1e-8                                  # the reference mode is a mode for the device's gradient too


def test_hessian_jacobian_setting(small):
    f, n = small["full"], small["no_mode_adjustment"]
    assert raw(n["res"][0], KEYS + ("precision",)) == raw(n["res"][1], KEYS + ("precision",))       # no Jacobian term in that variant
    assert f["res"][0]["precision"].tobytes() != f["res"][1]["precision"].tobytes()


@pytest.mark.parametrize("variant", VARIANTS)
def test_workgroups_per_mode_do_not_change_the_bytes(small, variant, monkeypatch):
    s = small[variant]
    mode = oref.small_reference(variant, True)["q"]
    for g in ("1", "7", "300"):                                         # one workgroup; D = 292 / 260 is no multiple of 7; more workgroups than a few columns each
        monkeypatch.setenv("POTUS_LAPLACE_G", g)
        got = s["h"].laplace(mode, N_SMALL, u=s["u"], precision=True, jacobian=1)
        assert raw(got, KEYS + ("precision",)) == raw(s["res"][1], KEYS + ("precision",)), g


# ------------------------------------------------------------------------------------------------ 2. draws with the caller's u
def check_draws(h, mode, res, u, who):
    P = res["precision"][0]
    D = h.D
    L = np.linalg.cholesky(P)
    X = solve_triangular(L.T, u.T, lower=False).T
    ev = np.linalg.eigvalsh(P)
    kappa = ev[-1] / ev[0]
    bound = 8.0 * D * EPS * kappa * np.abs(X).max()
    err = np.abs(res["q"][0] - mode - X).max()
    print(f"{who}: D {D}, draws {u.shape[0]}, kappa_2 {kappa:.1f}, |X|max {np.abs(X).max():.3f}, |q - q^ - X|max {err:.3e} <= {bound:.3e}")
    assert err <= bound
    lp, _ = h.log_prob_grad(res["q"][0])
    assert lp.tobytes() == res["lp"][0].tobytes()
    want = -0.5 * (u ** 2).sum(1)
    assert np.all(np.abs(res["lp_approx"][0] - want) <= 1e-13 * np.abs(want))
    sign, logdet = np.linalg.slogdet(P)
    assert sign == 1.0 and abs(res["log_det"][0] - logdet) <= 1e-12 * abs(logdet)
    assert abs(res["min_pivot"][0] - (np.diag(L) ** 2).min()) <= 1e-9 * res["min_pivot"][0]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("jacobian", [0, 1])
def test_draws_with_the_callers_u(small, variant, jacobian):
    s = small[variant]
    check_draws(s["h"], oref.small_reference(variant, bool(jacobian))["q"], s["res"][jacobian], s["u"][0], f"{variant} jacobian={jacobian}")


@pytest.mark.parametrize("shape", ["tiny", "mid", "panel", "panel_and_a_row"])
def test_draws_on_other_block_counts(shape):
    """Tiny: D = 78, two blocks of 64, one ragged.  Mid: D = 598, ten blocks, three panels of the factorisation.  Draw counts 1, 17 and 65.
    Panel: D = 256 exactly, one full panel of four blocks and no ragged one.  Panel and a row: D = 257, the one-row block is the first that
    k_lap_solve_diag solves.  Their draw counts are 63, 64, 65 and 128: a workgroup of k_lap_solve_update owns 64 draws."""
    kw = dict(tiny=dict(S=3, T=8, N_state=20, N_national=8, P=4), mid=dict(S=9, T=40, N_state=120, N_national=40, P=12),
              panel=dict(S=5, T=20, N_state=90, N_national=22, P=6), panel_and_a_row=dict(S=5, T=20, N_state=91, N_national=22, P=6))[shape]
    data = synthetic.make(**kw)
    h = Handle(data, "full", chains=1, **OPTS)
    assert h.D == dict(tiny=78, mid=598, panel=256, panel_and_a_row=257)[shape]
    opt = h.optimize(np.zeros((1, h.D)), jacobian=1, tol_obj=0.0, tol_rel_obj=0.0, tol_grad=1e-4, tol_rel_grad=0.0, tol_param=0.0, iter=5000)
    assert opt["return_code"][0] == 3
    mode = opt["q"][0]
    for n in ((63, 64, 65, 128) if shape.startswith("panel") else (1, 17, 65)):
        u = np.random.default_rng(n).standard_normal((n, h.D))
        res = h.laplace(mode, n, u=u, precision=True)
        assert res["return_code"][0] == 0
        check_draws(h, mode, res, u, f"{shape}, {n} draws")
    h.close()


# ------------------------------------------------------------------------------------------------ 3. library normals and batching
@pytest.mark.parametrize("variant", VARIANTS)
def test_library_normals_and_batching(small, variant):
    s = small[variant]
    h, mode = s["h"], oref.small_reference(variant, True)["q"]
    lib = h.laplace(mode, N_SMALL, precision=True)
    P = lib["precision"][0]
    assert P.tobytes() == s["res"][1]["precision"][0].tobytes()
    # u of draw n, from the documented counters with the oracle's Philox, gives these draws through the caller's-u path
    u = np.stack([lref.library_normals(1843, n, h.D) for n in range(N_SMALL)])
    want = -0.5 * (u ** 2).sum(1)
    assert np.all(np.abs(lib["lp_approx"][0] - want) <= 1e-12 * np.abs(want))         # (the device's log / sincos against libm's)
    X = solve_triangular(np.linalg.cholesky(P).T, u.T, lower=False).T
    ev = np.linalg.eigvalsh(P)
    assert np.abs(lib["q"][0] - mode - X).max() <= 8.0 * h.D * EPS * (ev[-1] / ev[0]) * np.abs(X).max() + 1e-12 * np.abs(X).max()
    # 37 draws in one call = three calls with draw_offset 0 / 12 / 24
    parts = [h.laplace(mode, k, draw_offset=o) for o, k in ((0, 12), (12, 12), (24, 13))]
    for key in ("q", "lp", "lp_approx"):
        assert np.concatenate([p[key][0] for p in parts]).tobytes() == lib[key][0].tobytes(), key
    assert raw(h.laplace(mode, N_SMALL)) == raw(lib)                                 # the same call twice
    big = h.laplace(mode, 65)                                                       # a second tile of draws does not move the first
    assert np.ascontiguousarray(big["q"][0, :N_SMALL]).tobytes() == lib["q"][0].tobytes()
    assert np.ascontiguousarray(big["lp"][0, :N_SMALL]).tobytes() == lib["lp"][0].tobytes()
    other = Handle(s["data"], variant, chains=1, seed=1844, cus_per_chain=1, twin=0)  # the key is the handle's seed
    assert other.laplace(mode, 3)["q"].tobytes() != np.ascontiguousarray(lib["q"][:, :3]).tobytes()
    other.close()


# ------------------------------------------------------------------------------------------------ 4. the approximation itself
@pytest.mark.parametrize("variant", VARIANTS)
def test_log_ratio_and_pareto_k(small, variant):
    """1 000 draws with u from default_rng(1), Jacobian on.  The reference's log_ratio: numpy's Cholesky of the device's P, scipy's solve,
    the oracle's log density -- the draws and lp__ of the device against the host's, on the matrix both were given."""
    s = small[variant]
    r = oref.small_reference(variant, True)
    u = np.random.default_rng(1).standard_normal((1000, s["h"].D))
    la = PotusModel(variant).laplace(s["data"], mode=r["q"], draws=1000, u=u)
    assert np.ascontiguousarray(la.q[:N_SMALL]).tobytes() != s["res"][1]["q"][0].tobytes()       # (another u)
    want, _ = lref.log_ratio(r["obj"], r["q"], s["res"][1]["precision"][0], u)
    err = np.abs(la.log_ratio - want).max()
    print(f"{variant}: log_ratio mean {la.log_ratio.mean():.4f} sd {la.log_ratio.std():.4f} max {la.log_ratio.max():.3f} (host: {want.mean():.4f} / {want.std():.4f}); "
          f"max |device - host| {err:.2e}; log det P {la.log_det:.4f}")
    assert err <= 1e-8
    assert abs(la.log_ratio.mean() - want.mean()) <= 1e-8 and abs(la.log_ratio.std() - want.std()) <= 1e-8
    k = la.pareto_k
    _, k_ref = psis_ref.psis(-la.log_ratio, psis_ref.relative_eff(-la.log_ratio.reshape(1, -1)))
    print(f"{variant}: pareto k {k:.4f} (psis_ref {k_ref:.4f})")
    assert np.isfinite(k) and abs(k - k_ref) <= 1e-8 * max(1.0, abs(k_ref))
    ps = la.draws("predicted_score")
    T, S = int(s["data"]["T"]), int(s["data"]["S"])
    assert ps.shape == (1000, T, S) and la.draws("lp__").tobytes() == la.lp.tobytes()
    assert np.ascontiguousarray(ps[:, T - 1]).tobytes() == la.scores().cpu().numpy()[:, 0].tobytes()
    la.close()


# ------------------------------------------------------------------------------------------------ 5. NOT_PD
def test_an_indefinite_point_fails_its_mode_alone(small):
    s = small["full"]
    h = s["h"]
    bad = np.random.default_rng(3).uniform(-2, 2, h.D)                                # lambda_min(-H) = -4.93 there by autograd
    good = oref.small_reference("full", True)["q"]
    nan_mode = good.copy()
    nan_mode[5] = np.nan
    res = h.laplace(np.stack([bad, good, nan_mode]), N_SMALL, u=np.concatenate([s["u"]] * 3), precision=True, jacobian=1)
    assert res["return_code"].tolist() == [1, 0, 2]
    assert np.isnan(res["q"][0]).all() and np.isnan(res["lp"][0]).all() and np.isnan(res["lp_approx"][0]).all() and np.isnan(res["log_det"][0])
    assert np.isfinite(res["precision"][0]).all() and np.linalg.eigvalsh(res["precision"][0])[0] < 0 and np.isfinite(res["grad_norm"][0])
    assert np.isnan(res["q"][2]).all() and np.isnan(res["precision"][2]).all() and np.isnan(res["grad_norm"][2])
    for k in KEYS + ("precision",):
        assert np.ascontiguousarray(res[k][1:2]).tobytes() == s["res"][1][k].tobytes(), k
    out = h.laplace_summary(EV)
    assert out["n_draws"].tolist() == [0, N_SMALL, 0] and np.isnan(out["state"][0]).all() and np.isfinite(out["state"][1]).all()


# ------------------------------------------------------------------------------------------------ 6. data sets
def three_dates():
    """synthetic.small with three run dates that keep different polls and have different priors (tests/test_gpu_optimize.py's design)."""
    data = synthetic.small("full")
    Ns, Nn, S = int(data["N_state_polls"]), int(data["N_national_polls"]), int(data["S"])
    rng = np.random.default_rng(3)
    keep_s = np.stack([rng.uniform(size=Ns) < 0.5, rng.uniform(size=Ns) < 0.8, np.ones(Ns, bool)])
    keep_n = np.stack([rng.uniform(size=Nn) < 0.5, rng.uniform(size=Nn) < 0.8, np.ones(Nn, bool)])
    prior = np.tile(np.asarray(data["mu_b_prior"], dtype=np.float64), (3, 1))
    prior[0] += np.linspace(-0.3, 0.4, S)
    prior[1] -= 0.1
    return timeline.design_of(data, keep_s, keep_n, prior, np.full(3, float(data["mu_b_T_scale"])))


def test_data_sets_equal_stand_alone_handles(monkeypatch):
    design = three_dates()
    h = Handle(design["data"], "full", chains=3, **OPTS)
    timeline.set_design(h, design)
    tight = dict(jacobian=1, tol_obj=0.0, tol_rel_obj=0.0, tol_grad=1e-4, tol_rel_grad=0.0, tol_param=0.0, iter=5000)
    modes = h.optimize(np.zeros((3, h.D)), **tight)["q"]
    n = 17
    u = np.random.default_rng(4).standard_normal((3, n, h.D))
    many = h.laplace(modes, n, u=u, precision=True)
    rows, scores = h.laplace_rows_device().cpu().numpy().reshape(3, n, -1), h.laplace_scores((0, 3)).cpu().numpy()
    assert many["return_code"].tolist() == [0, 0, 0]
    assert status_of(lambda: h.laplace(modes[:2], n)) == 1                            # 2 modes over 3 data sets
    monkeypatch.setenv("POTUS_LAPLACE_MATRIX_BUDGET", "1")                            # one matrix at a time
    assert raw(h.laplace(modes, n, u=u, precision=True), KEYS + ("precision",)) == raw(many, KEYS + ("precision",))
    monkeypatch.delenv("POTUS_LAPLACE_MATRIX_BUDGET")
    lib = h.laplace(modes, n)
    for d in range(3):
        g = Handle(timeline.data_of(design, d), "full", chains=1, **OPTS)
        one = g.laplace(modes[d], n, u=u[d], precision=True)
        for k in KEYS + ("precision",):
            assert one[k].tobytes() == np.ascontiguousarray(many[k][d:d + 1]).tobytes(), (d, k)
        assert g.laplace_rows_device().cpu().numpy().tobytes() == np.ascontiguousarray(rows[d]).tobytes()
        assert g.laplace_scores((0, 3)).cpu().numpy().tobytes() == np.ascontiguousarray(scores[d:d + 1]).tobytes()
        assert raw(g.laplace(modes[d], n)) == raw({k: lib[k][d:d + 1] for k in KEYS})   # the library's u: the same draws for every mode
        g.close()
    assert np.abs(many["q"][0] - many["q"][2]).max() > 1e-3
    h.close()


# ------------------------------------------------------------------------------------------------ 7. downstream blocks
@pytest.mark.parametrize("variant", VARIANTS)
def test_downstream_blocks(small, variant):
    s = small[variant]
    h, data = s["h"], s["data"]
    T, S = int(data["T"]), int(data["S"])
    res = h.laplace(oref.small_reference(variant, True)["q"], N_SMALL, u=s["u"])
    rows = h.laplace_rows_device().cpu().numpy()
    assert rows.shape == (N_SMALL, h.n_cols)
    assert rows[:, 0].tobytes() == res["lp"][0].tobytes() and np.isnan(rows[:, 1:7]).all()
    assert np.ascontiguousarray(rows[:, 7:]).tobytes() == h.constrain(res["q"][0]).tobytes()
    a, b, _ = h.layout["predicted_score"]
    part = h.laplace_rows_device((a, b)).cpu().numpy()
    assert part.tobytes() == np.ascontiguousarray(rows[:, a:b]).tobytes()
    ps = part.reshape(N_SMALL, S, T).transpose(0, 2, 1)                               # predicted_score is T x S column-major
    for days in ((0, T), (T - 1, T), (3, 7)):
        x = h.laplace_scores(days).cpu().numpy()
        assert x.shape == (1, N_SMALL, days[1] - days[0], S)
        assert x[0].tobytes() == np.ascontiguousarray(ps[:, days[0]:days[1]]).tobytes(), days
    assert h.laplace_scores().cpu().numpy().tobytes() == h.laplace_scores((T - 1, T)).cpu().numpy().tobytes()
    out = h.laplace_summary(EV, (T - 3, T), ev_to_win=200)
    want = timeline_ref.summary(ps[:, T - 3:], data["state_weights"], EV, ev_to_win=200)
    assert out["n_draws"].tolist() == [N_SMALL]
    for key, mean_col in (("state", 2), ("national", 2), ("electoral_votes", None)):   # test_gpu_timeline._compare's tolerances
        err = np.abs(out[key][0] - np.asarray(want[key]))
        for j in range(err.shape[-1]):
            assert err[..., j].max() <= (1e-12 if j == mean_col else 1e-15), (key, j, err[..., j].max())
    blk = h.laplace_scores((0, T))[0].contiguous()
    o = outcomes_of_block(blk, data["state_weights"], EV)
    w = outcomes_ref.outcomes_vectorised(ps, outcomes_ref.normalised_weights(data["state_weights"]), EV)
    assert o.n_draws == N_SMALL
    for k in ("ev_hist", "tipping", "joint"):
        assert np.array_equal(getattr(o, k), w[k]), k
    ms = h.laplace_timing()
    assert ms["hessian_ms"] > 0 and ms["factor_ms"] > 0 and ms["solve_ms"] > 0 and ms["lp_ms"] > 0


# ------------------------------------------------------------------------------------------------ 8. refusals, an undisturbed run, R
def test_refusals_and_an_undisturbed_run(small):
    s = small["full"]
    h, data = s["h"], s["data"]
    mode = oref.small_reference("full", True)["q"]
    ARG, STATE, UNSUP = 1, 4, 6
    assert status_of(lambda: h.laplace(mode, -1)) == ARG
    for x in (0.0, -1e-4, float("inf"), float("nan")):
        assert status_of(lambda: h.laplace(mode, 3, h=x)) == ARG, x
    assert status_of(lambda: h.laplace(mode, 3, jacobian=2)) == ARG and status_of(lambda: h.laplace(mode, 3, draw_offset=-1)) == ARG
    L, o = h.L, h.laplace_opts()
    dp = C.POINTER(C.c_double)
    info = np.zeros(4)
    m = np.ascontiguousarray(mode)
    assert L.potus_laplace(h.h, C.byref(o), m.ctypes.data_as(dp), 0, None, 0, None, None, None, info.ctypes.data_as(dp), None) == ARG        # n_modes = 0
    assert L.potus_laplace(h.h, C.byref(o), None, 1, None, 0, None, None, None, info.ctypes.data_as(dp), None) == ARG                       # null mode
    assert L.potus_laplace(h.h, C.byref(o), m.ctypes.data_as(dp), 1, None, 0, None, None, None, None, None) == ARG                          # null info_out
    assert L.potus_laplace(12345, C.byref(o), m.ctypes.data_as(dp), 1, None, 0, None, None, None, info.ctypes.data_as(dp), None) == STATE
    assert L.potus_laplace_timing(None) == ARG
    hk = Handle(data, "full", chains=1, seed=1843, cus_per_chain=2, twin=0)
    assert hk.cus_per_chain == 2 and status_of(lambda: hk.laplace(mode, 3)) == UNSUP
    hk.close()
    hd = Handle(data, "full", chains=1, seed=1843, cus_per_chain=1, twin=0, metric=_abi.METRICS["dense_e"])
    assert status_of(lambda: hd.laplace(mode, 3)) == UNSUP
    hd.close()
    # the accessors before any potus_laplace, and after a call without draws; then their ranges
    import torch
    f = Handle(data, "full", chains=1, **OPTS)
    buf = torch.empty(4096, dtype=torch.float64, device="cuda:0")
    ev = np.ascontiguousarray(EV, dtype=np.float64)
    z = np.zeros(4096)
    i32 = np.zeros(8, np.int32)
    acc = lambda: (L.potus_laplace_write_array_device(f.h, 0, 8, C.c_void_p(buf.data_ptr())), L.potus_laplace_scores_device(f.h, 0, 1, C.c_void_p(buf.data_ptr())),
                   L.potus_laplace_summary(f.h, 0, 1, ev.ctypes.data_as(dp), 270, z.ctypes.data_as(dp), z.ctypes.data_as(dp), z.ctypes.data_as(dp),
                                           i32.ctypes.data_as(C.POINTER(C.c_int32))))
    assert acc() == (STATE, STATE, STATE)
    with pytest.raises(PotusError):
        f.laplace_scores()
    only_p = f.laplace(mode, 0, precision=True)                                         # the Hessian only
    assert only_p["precision"].tobytes() == s["res"][1]["precision"].tobytes() and only_p["q"].shape == (1, 0, f.D) and only_p["return_code"][0] == 0
    assert only_p["log_det"].tobytes() == s["res"][1]["log_det"].tobytes()
    assert acc() == (STATE, STATE, STATE)
    f.laplace(mode, 3)
    T = int(data["T"])
    assert status_of(lambda: f.laplace_rows_device((5, 5))) == ARG and status_of(lambda: f.laplace_rows_device((0, f.n_cols + 1))) == ARG
    assert status_of(lambda: f.laplace_scores((3, 3))) == ARG and status_of(lambda: f.laplace_scores((0, T + 1))) == ARG
    assert status_of(lambda: f.laplace_summary(EV, (-1, 2))) == ARG
    assert L.potus_laplace_scores_device(f.h, 0, 1, None) == STATE
    assert L.potus_laplace_scores_device(f.h, 0, 1, z.ctypes.data_as(C.c_void_p)) == ARG   # host memory is refused, not written
    assert status_of(lambda: f.laplace(mode, 3, h=0.0)) == ARG and acc()[0] == 0           # a refused call leaves the last rows alone
    f.close()
    # a sampling run with a refused and a successful call in its middle gives the bytes of an uninterrupted one
    run = dict(chains=2, num_warmup=20, num_samples=20, **OPTS)
    a, b = Handle(data, "full", **run), Handle(data, "full", **run)
    before = b.laplace(mode, 5)                                                         # before init
    for x in (a, b):
        x.init()
    a.run(40)
    b.run(20)
    assert status_of(lambda: b.laplace(mode, -2)) == ARG
    mid = b.laplace(mode, 5)
    b.run(20)
    assert raw(before) == raw(mid) == raw(h.laplace(mode, 5))
    assert a.draws().tobytes() == b.draws().tobytes() and a.chain_status() == b.chain_status()
    a.close()
    b.close()


def test_more_draws_than_the_summary_sorts_are_refused_by_the_summary_alone():
    data = synthetic.make(S=3, T=8, N_state=20, N_national=8, P=4)
    h = Handle(data, "full", chains=1, **OPTS)
    mode = h.optimize(np.zeros((1, h.D)), jacobian=1, tol_obj=0.0, tol_rel_obj=0.0, tol_grad=1e-4, tol_rel_grad=0.0, tol_param=0.0, iter=5000)["q"][0]
    res = h.laplace(mode, 16385)
    assert res["return_code"][0] == 0 and np.isfinite(res["lp"]).all()
    assert status_of(lambda: h.laplace_summary(np.array([3.0, 4.0, 5.0]))) == 6
    assert h.laplace_scores().shape == (1, 16385, 1, 3)
    h.close()


def test_r_entry_point(small):
    s = small["full"]
    h, u = s["h"], s["u"]
    mode = np.ascontiguousarray(oref.small_reference("full", False)["q"])
    n, D = N_SMALL, h.D
    want = h.laplace(mode, n, u=u, precision=True, jacobian=0, h=3e-5)
    q, lp, la, info, prec, st = np.zeros((n, D)), np.zeros(n), np.zeros(n), np.zeros(4), np.zeros((D, D)), (C.c_int * 1)(-1)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    h.L.potus_R_laplace((C.c_int * 1)(h.h), (C.c_int * 6)(0, 0, 1, n, 1, 1), (C.c_double * 1)(3e-5), dp(mode), dp(np.ascontiguousarray(u)), dp(q), dp(lp), dp(la),
                        dp(info), dp(prec), st)
    assert st[0] == 0
    assert q.tobytes() == want["q"].tobytes() and lp.tobytes() == want["lp"].tobytes() and la.tobytes() == want["lp_approx"].tobytes()
    assert prec.tobytes() == want["precision"].tobytes() and info[1] == want["log_det"][0] and info[0] == 0
    assert want["precision"].tobytes() != s["res"][0]["precision"].tobytes()              # (another h)
    lib = h.laplace(mode, n, jacobian=0, draw_offset=5)
    h.L.potus_R_laplace((C.c_int * 1)(h.h), (C.c_int * 6)(0, 5, 1, n, 0, 0), (C.c_double * 1)(1e-4), dp(mode), dp(q), dp(q), dp(lp), dp(la), dp(info), dp(prec), st)
    assert st[0] == 0 and q.tobytes() == lib["q"].tobytes() and lp.tobytes() == lib["lp"].tobytes()


def test_the_model_call_finds_its_own_mode(small):
    s = small["no_mode_adjustment"]
    la = PotusModel("no_mode_adjustment").laplace(s["data"], draws=65)
    r = oref.small_reference("no_mode_adjustment", True)
    assert la.grad_norm < 1e-2 and np.linalg.norm(la.mode - r["q"]) <= (la.grad_norm + 1e-9) / 0.95      # -Hessian >= I in this variant
    assert la.q.shape == (65, s["h"].D) and np.isfinite(la.log_ratio).all() and abs(la.log_ratio.mean()) < 0.1 and la.log_ratio.std() < 0.2
    sm = la.summary(EV)
    assert sm["n_draws"] == 65 and sm["state"].shape == (1, int(s["data"]["S"]), 4)
    la.close()


# ------------------------------------------------------------------------------------------------ 9. one real shape
def _identity_error(obj, mode, x, u):
    """max over the draws of |d . (-H) d - |u|^2| / |u|^2 with d = x - mode and (-H) d from two oracle gradients (Objective.hess_vec)."""
    worst = 0.0
    for xi, ui in zip(x, u):
        d = xi - mode
        uu = float(ui @ ui)
        worst = max(worst, abs(float(d @ obj.hess_vec(mode, d)) - uu) / uu)
    return worst


def test_real_shape_2016():
    """2016, full, D = 15 098: 236 blocks of 64 and 59 panels, one matrix of 1.8 GB.  No D x D matrix on the host: for three of 64 draws
    (x - q^) . (-H)(x - q^) is compared with |u|^2, the product by two oracle gradients.  Tolerance: ten times the same identity's error on the
    small design, there evaluated with numpy on the oracle's own central-difference matrix at the same h -- hess_vec's own step error dominates
    both and grows with |q^|."""
    from conftest import GOLD
    from us_potus_model_amd import dataprep
    r = oref.small_reference("full", True)
    us = np.random.default_rng(8).standard_normal((3, r["obj"].D))
    Xs = solve_triangular(np.linalg.cholesky(lref.small_precision_fd("full", True, 1e-4)).T, us.T, lower=False).T
    tol = 10.0 * _identity_error(r["obj"], r["q"], r["q"] + Xs, us)
    data = dataprep.load_npz(GOLD / "data_2016.npz")["data"]
    h = Handle(data, "full", chains=1, **OPTS)
    opt = h.optimize(np.zeros((1, h.D)), jacobian=1, tol_obj=0.0, tol_rel_obj=0.0, tol_grad=1e-2, tol_rel_grad=0.0, tol_param=0.0, iter=5000)
    assert opt["return_code"][0] == 3
    mode = opt["q"][0]
    u = np.random.default_rng(9).standard_normal((64, h.D))
    res = h.laplace(mode, 64, u=u)
    ms = h.laplace_timing()
    assert res["return_code"][0] == 0 and np.isfinite(res["q"]).all() and np.isfinite(res["lp"]).all()
    lp, _ = h.log_prob_grad(res["q"][0][:4])
    assert lp.tobytes() == np.ascontiguousarray(res["lp"][0][:4]).tobytes()
    err = _identity_error(oref.Objective(data, "full", True), mode, res["q"][0][:3], u[:3])
    print(f"2016: ||g|| at the mode {res['grad_norm'][0]:.2e}, log det P {res['log_det'][0]:.4f}, smallest pivot {res['min_pivot'][0]:.4f}; identity error {err:.3e} <= {tol:.3e} "
          f"(small design: {tol / 10:.3e}); stages {ms}")
    assert err <= tol
    h.close()
