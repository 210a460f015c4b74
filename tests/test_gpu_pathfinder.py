"""Pathfinder on the MI355X (potus_pathfinder, potus_pathfinder_path: opt_record in k_opt_lbfgs, k_pf_alpha, k_pf_elbo, k_pf_draws) against
tests/pathfinder_ref.py (numpy, the DENSE form: Sigma_l as a D x D matrix, slogdet, the multivariate-normal density), against
potus_optimize / potus_log_prob_grad / potus_constrain of the same handle, and against stand-alone handles for the data sets of a
potus_set_datasets_ex handle.  Designs: synthetic.small of both variants, as tests/test_gpu_laplace.py.

Bounds.  e_ref is the reference's own error: the spread between its dense and its low-rank form on the device's trajectory, measured by the
test per quantity and printed.  Both forms share numpy's Householder QR, so e_ref holds the conditioning of what each form inverts but not the
rounding of forming a value in another order; the device is held to 2 x e_ref -- one share for each side of the comparison, DESIGN.md
section 4n's convention -- plus that one rounding term, stated per quantity and asserted at l = 1, the first l with a full history, l* and L:
  mu         every entry is a sum of 2 j + 3 products: (2 J + 4) eps max|entry|
  phi        the same, and the 2 j sums Q'u of D terms, each through DEPTH additions (below): |d(Q'u)_m| <= DEPTH eps sum_i |Q_im u_i|, carried
             through |L~ - I|, |Q| and alpha^1/2 to first order (pathfinder_ref.phi_rounding, from the reference's own Q and L~): 1.5e-14 ..
             3.9e-14; measured at most 9.4e-15 (e_ref 8.3e-16 there, the first full history)
  log det    a sum of D logarithms whose partial sums pass through DEPTH = ceil(D / 512) + 14 additions on the device (a thread's strided
             share, six DPP steps, eight waves): DEPTH eps sum|log alpha|
  log q      the same with the sum u'u beside it: DEPTH eps (sum|log alpha| + u'u) / 2
  ELBO       log q's term plus the share of log p: what potus_log_prob_grad and the oracle differ by at the reference's own phi of every iterate,
             measured in the test on those points (2.9e-11 .. 5.1e-11 at |lp| = 5.2e4), not an a-priori 1e-11 |lp|
  alpha      every entry is a rational function of three sums of D terms in another order than numpy's: 8 D eps relative
  Q'Q - I    an entry is a dot product of two unit vectors, its rounding at most DEPTH eps by Cauchy-Schwarz, on both sides of the re-orthogonalised
             Gram-Schmidt's own O(eps): 2 DEPTH eps
The seeds are such that the reference's two highest ELBOs lie further apart than 10 x the ELBO's bound on every path (asserted), so l* is asserted too.
Measured on one MI355X (the largest over both variants, both paths and the four iterates): see DESIGN.md section 4o."""
import re

import numpy as np
import pytest

import outcomes_ref
import pathfinder_ref as pref
import timeline_ref
from oracle_lib import OracleModel
from us_potus_model_amd import synthetic, timeline
from us_potus_model_amd import _abi
from us_potus_model_amd.outcomes import outcomes_of_block
from us_potus_model_amd.sampler import Handle, PotusError, PotusModel

pytestmark = pytest.mark.gpu
OPTS = dict(seed=1843, cus_per_chain=1, twin=0)
VARIANTS = ("full", "no_mode_adjustment")
EV = np.array([100, 90, 80, 70, 60, 138])
EPS = 2.0 ** -52
J, ITER, M = 6, 40, 37
PF = dict(history_size=J, max_lbfgs_iters=ITER, num_draws=M)
KEYS = ("q", "lp", "lq", "elbo", "kept", "return_code", "iterations", "best_iteration")


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
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
    """Per variant: a plain handle and ONE potus_pathfinder call of two paths from given starts, with its trajectory."""
    out = {}
    for v in VARIANTS:
        data = synthetic.small(v)
        h = Handle(data, v, chains=1, **OPTS)
        q0 = np.random.default_rng(1).uniform(-1, 1, (2, h.D))
        res = h.pathfinder(q0, trajectory=True, num_elbo_draws=5, **PF)
        for a in res.values():
            a.setflags(write=False)
        out[v] = dict(data=data, h=h, q0=q0, res=res, oracle=OracleModel(data, v))
    yield out
    for v in VARIANTS:
        out[v]["h"].close()


# ------------------------------------------------------------------------------------------------ 1. the trajectory
@pytest.mark.parametrize("variant", VARIANTS)
def test_trajectory(small, variant):
    s = small[variant]
    h, res = s["h"], s["res"]
    opt = h.optimize(s["q0"], jacobian=1, iter=ITER)
    assert res["optimize_code"].tolist() == opt["return_code"].tolist() and res["iterations"].tolist() == opt["iterations"].tolist()
    for p in range(2):
        L = int(res["iterations"][p])
        assert 2 <= L <= ITER
        x, g = res["x"][p], res["g"][p]
        assert x[L].tobytes() == opt["q"][p].tobytes() and x[0].tobytes() == s["q0"][p].tobytes()
        assert np.isnan(x[L + 1:]).all() and np.isnan(g[L + 1:]).all()
        lp, gr = h.log_prob_grad(np.ascontiguousarray(x[:L + 1]))
        assert np.ascontiguousarray(g[:L + 1]).tobytes() == gr.tobytes()
        assert (np.diff(lp) > 0).all() and lp[L] == opt["lp"][p]


# ------------------------------------------------------------------------------------------------ 2. against the reference
def _check(name, dev, dense, low, floor, what):
    e_ref, err = float(np.abs(dense - low).max()), float(np.abs(dev - dense).max())
    print(f"  {name}: e_ref {e_ref:.2e} device {err:.2e} rounding term {floor:.2e}")
    assert err <= 2.0 * e_ref + floor, (name, what, err, e_ref, floor)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K", [1, 5])
def test_against_the_reference(small, variant, K):
    s = small[variant]
    h, res, D = s["h"], s["res"], s["h"].D
    log_p = lambda q: s["oracle"].log_prob_grad(np.ascontiguousarray(q))[0]
    rng = np.random.default_rng(10 + K)
    depth = -(-D // 512) + 14
    for p in range(2):
        L = int(res["iterations"][p])
        x, g = np.array(res["x"][p][:L + 1]), np.array(res["g"][p][:L + 1])
        ak = pref.alphas(x, g)
        al, kept, _ = ak
        ue, ud = rng.standard_normal((L, K, D)), rng.standard_normal((M, D))
        e_dense, e_low = pref.elbo(pref.dense, log_p, x, g, J, ue), pref.elbo(pref.low_rank, log_p, x, g, J, ue)
        lstar = pref.best(e_dense)
        # the ELBO's bound: log q's rounding and what the device's log density and the oracle's differ by at the reference's own points
        pts = np.concatenate([pref.low_rank(x, g, l, J, u=ue[l - 1], al_kept=ak)["phi"] for l in range(1, L + 1)])
        lp_share = float(np.abs(h.log_prob_grad(np.ascontiguousarray(pts))[0] - np.array([log_p(q) for q in pts])).max())
        lq_floor = depth * EPS * 0.5 * (np.abs(np.log(al)).sum(1).max() + (ue * ue).sum(2).max())
        e_ref_elbo = float(np.abs(e_dense[1:] - e_low[1:]).max())
        bound_elbo = 2.0 * e_ref_elbo + lp_share + lq_floor
        top = np.sort(e_dense[1:])[::-1]
        print(f"{variant} K={K} path {p}: ELBO e_ref {e_ref_elbo:.2e}, lp share {lp_share:.2e}, log q term {lq_floor:.2e}; l* {lstar} of {L}, top two {top[:2]}")
        assert np.isfinite(e_dense[1:]).all() and top[0] - top[1] > 10.0 * bound_elbo
        full = [l for l in range(1, L + 1) if len(pref.history(kept, l, J)) == J]
        assert full
        for l in sorted({1, full[0], lstar, L}):
            out = h.pathfinder_path(x, g, u_elbo=ue, u_draws=ud, want=l, num_elbo_draws=K, history_size=J, num_draws=M)
            assert out["kept"][0, :L + 1].tolist() == kept.astype(int).tolist() and out["iterations"][0] == L
            a_err = np.abs(out["alpha"][0] / al[l] - 1.0).max()
            print(f" l={l}: alpha rel err {a_err:.2e} (bound {8 * D * EPS:.2e})")
            assert a_err <= 8 * D * EPS
            dn, lo = pref.dense(x, g, l, J, u=ud, al_kept=ak), pref.low_rank(x, g, l, J, u=ud, al_kept=ak)
            sla = np.abs(np.log(al[l])).sum()
            _check("mu", out["mu"][0], dn["mu"], lo["mu"], (2 * J + 4) * EPS * np.abs(dn["mu"]).max(), l)
            _check("log_det", out["log_det"][0], dn["log_det"], lo["log_det"], depth * EPS * sla, l)
            _check("phi", out["phi"][0], dn["phi"], lo["phi"], pref.phi_rounding(lo, ud, depth), l)
            _check("lq", out["lq_want"][0], dn["lq"], lo["lq"], depth * EPS * 0.5 * (sla + (ud * ud).sum(1).max()), l)
            n = 2 * len(dn["hist"])
            qerr = np.abs(out["qtq"][0][:n, :n] - np.eye(n)).max()
            print(f"  |Q'Q - I| {qerr:.2e} (bound {2 * depth * EPS:.2e})")
            assert qerr <= 2 * depth * EPS and np.isnan(out["qtq"][0][n:]).all()
            err = float(np.abs(out["elbo"][0, 1:L + 1] - e_dense[1:]).max())
            print(f"  elbo: device {err:.2e} bound {bound_elbo:.2e}")
            assert err <= bound_elbo
            assert out["best_iteration"][0] == lstar
            if l == lstar:                                    # the draws themselves come from l*: the same bytes, and lp is the library's
                assert out["q"][0].tobytes() == out["phi"][0].tobytes() and out["lq"][0].tobytes() == out["lq_want"][0].tobytes()
                assert out["lp"][0].tobytes() == h.log_prob_grad(np.ascontiguousarray(out["q"][0]))[0].tobytes()


# ------------------------------------------------------------------------------------------------ 3. edges, on crafted trajectories
def test_edges(small):
    s = small["full"]
    h, D = s["h"], s["h"].D
    x0, g0 = np.array(s["res"]["x"][0]), np.array(s["res"]["g"][0])
    L0 = int(s["res"]["iterations"][0])
    rng = np.random.default_rng(20)
    ud = rng.standard_normal((5, D))
    kw = dict(history_size=3, num_elbo_draws=2, num_draws=5)
    # L = 1
    one = h.pathfinder_path(x0[:2], g0[:2], u_draws=ud, **kw)
    assert one["return_code"][0] == 0 and one["best_iteration"][0] == 1 and one["kept"][0].tolist() == [0, 1]
    want = pref.low_rank(x0[:2], g0[:2], 1, 3, u=ud)
    assert np.abs(one["q"][0] - want["phi"]).max() <= 1e-9 * max(1.0, np.abs(want["phi"]).max())
    # a repeated point (s = 0) and a pair with s'z < 0 in the middle: neither is kept, the history skips them
    x, g = x0[:7].copy(), g0[:7].copy()
    x = np.insert(x, 3, x[2], axis=0); g = np.insert(g, 3, g[2], axis=0)              # row 3 repeats row 2
    g[5] = g[4] + (g[4] - g[5])                                                      # pair 5: z -> -z
    _, kept, _ = pref.alphas(x, g)
    assert not kept[3] and not kept[5]
    out = h.pathfinder_path(x, g, u_draws=ud, want=6, **kw)
    assert out["kept"][0].tolist() == kept.astype(int).tolist()
    ref = pref.low_rank(x, g, 6, 3)
    assert ref["hist"] == pref.history(kept, 6, 3) and 3 not in ref["hist"] and 5 not in ref["hist"]
    assert np.abs(out["mu"][0] - ref["mu"]).max() <= 1e-9 * max(1.0, np.abs(ref["mu"]).max())
    # every pair rejected: Sigma = diag(1), the draws are x_L + g_L + u, byte for byte
    xr = x0[:4].copy()
    gr = g0[:4].copy()
    for l in range(1, 4):
        gr[l] = gr[l - 1] + (xr[l] - xr[l - 1])                                     # z = -s
    out = h.pathfinder_path(xr, gr, u_draws=ud, want=3, **kw)
    assert out["kept"][0].tolist() == [0, 0, 0, 0] and np.array_equal(out["alpha"][0], np.ones(D)) and out["log_det"][0] == 0.0
    ls = int(out["best_iteration"][0])
    assert ls >= 1 and out["q"][0].tobytes() == ((xr[ls] + gr[ls]) + ud).tobytes()
    lq = -0.5 * ((ud * ud).sum(1) + D * pref.LOG_2PI)
    assert np.abs(out["lq"][0] - lq).max() <= 4 * D * EPS * np.abs(lq).max()
    # more than J kept pairs: the oldest is dropped
    n = min(L0, 8)
    out = h.pathfinder_path(x0[:n + 1], g0[:n + 1], want=n, **kw)
    _, kept, _ = pref.alphas(x0[:n + 1], g0[:n + 1])
    assert kept[1:].sum() > 3
    ref = pref.low_rank(x0[:n + 1], g0[:n + 1], n, 3)
    assert len(ref["hist"]) == 3 and np.abs(out["mu"][0] - ref["mu"]).max() <= 1e-9 * max(1.0, np.abs(ref["mu"]).max())
    assert abs(out["log_det"][0] - ref["log_det"]) <= 1e-9 * max(1.0, abs(ref["log_det"]))


def test_a_path_without_an_elbo_fails_alone(small):
    """A trajectory around 1e4: the oracle's log density of its draws is -inf on the small full design (asserted), so the path's code is
    NO_ELBO and its draws are NaN; the other path of the call has the bytes it has alone."""
    s = small["full"]
    h, D = s["h"], s["h"].D
    x0, g0 = np.array(s["res"]["x"][0][:4]), np.array(s["res"]["g"][0][:4])
    xb = x0 + 1e4
    gb = g0.copy()
    kw = dict(history_size=3, num_elbo_draws=2, num_draws=5)
    alone = h.pathfinder_path(x0, g0, **kw)
    ref = pref.low_rank(xb, gb, 1, 3, u=np.zeros((1, D)))
    finite = np.isfinite(s["oracle"].log_prob_grad(np.ascontiguousarray(ref["phi"][0]))[0])
    both = h.pathfinder_path(np.stack([xb, x0]), np.stack([gb, g0]), **kw)
    assert not finite
    assert both["return_code"].tolist() == [1, 0] and both["best_iteration"][0] == 0
    assert np.isnan(both["q"][0]).all() and np.isnan(both["lp"][0]).all() and np.isinf(both["elbo"][0, 1:]).all()
    sm = h.pathfinder_summary(EV)
    assert sm["n_draws"].tolist() == [0, 5] and np.isnan(sm["state"][0]).all() and np.isfinite(sm["state"][1]).all()
    # path 1 of the pair is path_offset 1 alone
    again = h.pathfinder_path(x0, g0, path_offset=1, **kw)
    for k in ("q", "lp", "lq", "elbo"):
        assert np.ascontiguousarray(both[k][1:2]).tobytes() == again[k].tobytes(), k
    assert alone["elbo"].tobytes() != again["elbo"].tobytes()                          # (another path: other normals)


# ------------------------------------------------------------------------------------------------ 4. the library's normals
def test_library_normals(small):
    s = small["no_mode_adjustment"]
    h, D = s["h"], s["h"].D
    x, g = np.array(s["res"]["x"][1][:4]), np.array(s["res"]["g"][1][:4])
    kw = dict(history_size=J, num_elbo_draws=2, num_draws=3, path_offset=4, draw_offset=11)
    lib = h.pathfinder_path(x, g, **kw)
    ue = np.array([[pref.library_normals(1843, 4, D, l=l, k=k) for k in range(2)] for l in range(1, 4)])
    ud = np.array([pref.library_normals(1843, 4, D, draw=11 + n) for n in range(3)])
    mine = h.pathfinder_path(x, g, u_elbo=ue, u_draws=ud, **kw)
    # the oracle's Box-Muller and the device's agree to the last bits of sincos / log, not byte for byte (tests/test_gpu_laplace.py's bound)
    assert np.abs(lib["q"] - mine["q"]).max() <= 1e-12 * max(1.0, np.abs(mine["q"]).max())
    assert np.abs(lib["elbo"][0, 1:] - mine["elbo"][0, 1:]).max() <= 1e-9 * np.abs(mine["elbo"][0, 1:]).max()


# ------------------------------------------------------------------------------------------------ 5. equal bytes
@pytest.mark.parametrize("variant", VARIANTS)
def test_equal_bytes(small, variant, monkeypatch):
    s = small[variant]
    h, res = s["h"], s["res"]
    kw = dict(num_elbo_draws=5, **PF)
    assert raw(h.pathfinder(s["q0"], **kw)) == raw(res)                                        # the same call twice
    for G in ("1", "7", "300"):
        monkeypatch.setenv("POTUS_PATHFINDER_G", G)
        assert raw(h.pathfinder(s["q0"], **kw)) == raw(res), G
    monkeypatch.delenv("POTUS_PATHFINDER_G")
    # potus_pathfinder = potus_optimize's trajectory followed by potus_pathfinder_path
    L = res["iterations"]
    path = h.pathfinder_path(res["x"], res["g"], L=L, num_elbo_draws=5, history_size=J, num_draws=M)
    assert raw(path) == raw(res)
    # three library paths in one call against three calls with path_offset 0, 1, 2
    three = h.pathfinder(None, 3, **kw)
    for p in range(3):
        one = h.pathfinder(None, 1, path_offset=p, **kw)
        assert raw(one) == raw({k: three[k][p:p + 1] for k in KEYS}), p
    # 37 draws in one call against draw_offset 0 / 12 / 24
    x, g = res["x"][:1], res["g"][:1]
    whole = h.pathfinder_path(x, g, L=L[:1], num_elbo_draws=5, history_size=J, num_draws=M)
    for a, b in ((0, 12), (12, 24), (24, M)):
        part = h.pathfinder_path(x, g, L=L[:1], num_elbo_draws=5, history_size=J, num_draws=b - a, draw_offset=a)
        for k in ("q", "lp", "lq"):
            assert part[k].tobytes() == np.ascontiguousarray(whole[k][:, a:b]).tobytes(), (k, a)
        assert part["elbo"].tobytes() == whole["elbo"].tobytes()


def three_dates():
    """tests/test_gpu_laplace.py's design: synthetic.small with three run dates that keep different polls and have different priors."""
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
    kw = dict(num_elbo_draws=3, history_size=J, max_lbfgs_iters=25, num_draws=9)
    q0 = np.zeros((3, h.D))
    many = h.pathfinder(q0, **kw)
    rows, scores = h.pathfinder_rows_device().cpu().numpy().reshape(3, 9, -1), h.pathfinder_scores((0, 3)).cpu().numpy()
    assert many["return_code"].tolist() == [0, 0, 0] and status_of(lambda: h.pathfinder(q0[:2], **kw)) == 1
    for d in range(3):
        g = Handle(timeline.data_of(design, d), "full", chains=1, **OPTS)
        one = g.pathfinder(q0[:1], path_offset=d, **kw)
        assert raw(one) == raw({k: many[k][d:d + 1] for k in KEYS}), d
        assert g.pathfinder_rows_device().cpu().numpy().tobytes() == np.ascontiguousarray(rows[d]).tobytes()
        assert g.pathfinder_scores((0, 3)).cpu().numpy().tobytes() == np.ascontiguousarray(scores[d:d + 1]).tobytes()
        g.close()
    assert np.abs(many["q"][0] - many["q"][2]).max() > 1e-3
    # timeline.pathfinder is that call with the library's starts, and the summary per path
    lib = h.pathfinder(None, 3, **kw)
    sm = h.pathfinder_summary(EV)
    h.close()
    tl = timeline.pathfinder(design, "full", draws=9, ev=EV, seed=1843, **{k: v for k, v in kw.items() if k != "num_draws"})
    assert tl["lp"].tobytes() == lib["lp"].tobytes() and tl["lq"].tobytes() == lib["lq"].tobytes()
    assert tl["best_iteration"].ravel().tolist() == lib["best_iteration"].tolist() and tl["state"].shape == (3, 1) + sm["state"].shape[1:]
    assert tl["state"].tobytes() == sm["state"].tobytes() and tl["n_draws"].ravel().tolist() == [9, 9, 9]


# ------------------------------------------------------------------------------------------------ 6. the accessors
@pytest.mark.parametrize("variant", VARIANTS)
def test_downstream_blocks(small, variant):
    s = small[variant]
    h, data = s["h"], s["data"]
    T, S = int(data["T"]), int(data["S"])
    res = h.pathfinder(s["q0"], num_elbo_draws=5, **PF)
    rows = h.pathfinder_rows_device().cpu().numpy()
    assert rows.shape == (2 * M, h.n_cols)
    assert rows[:, 0].tobytes() == res["lp"].tobytes() and np.isnan(rows[:, 1:7]).all()
    assert np.ascontiguousarray(rows[:, 7:]).tobytes() == h.constrain(res["q"].reshape(2 * M, -1)).tobytes()
    a, b, _ = h.layout["predicted_score"]
    ps = rows[:, a:b].reshape(2, M, S, T).transpose(0, 1, 3, 2)                        # predicted_score is T x S column-major
    for days in ((0, T), (T - 1, T), (3, 7)):
        x = h.pathfinder_scores(days).cpu().numpy()
        assert x.shape == (2, M, days[1] - days[0], S)
        assert x.tobytes() == np.ascontiguousarray(ps[:, :, days[0]:days[1]]).tobytes(), days
    out = h.pathfinder_summary(EV, (T - 3, T), ev_to_win=200)
    assert out["n_draws"].tolist() == [M, M]
    for p in range(2):
        want = timeline_ref.summary(ps[p][:, T - 3:], data["state_weights"], EV, ev_to_win=200)
        for key, mean_col in (("state", 2), ("national", 2), ("electoral_votes", None)):  # test_gpu_timeline._compare's tolerances
            err = np.abs(out[key][p] - np.asarray(want[key]))
            for j in range(err.shape[-1]):
                assert err[..., j].max() <= (1e-12 if j == mean_col else 1e-15), (key, j, err[..., j].max())
    blk = h.pathfinder_scores((0, T)).reshape(2 * M, T, S).contiguous()
    o = outcomes_of_block(blk, data["state_weights"], EV)
    w = outcomes_ref.outcomes_vectorised(ps.reshape(2 * M, T, S), outcomes_ref.normalised_weights(data["state_weights"]), EV)
    assert o.n_draws == 2 * M
    for k in ("ev_hist", "tipping", "joint"):
        assert np.array_equal(getattr(o, k), w[k]), k
    ms = h.pathfinder_timing()
    assert ms["lbfgs_ms"] > 0 and ms["alpha_ms"] > 0 and ms["elbo_ms"] > 0 and ms["draws_ms"] > 0


# ------------------------------------------------------------------------------------------------ 7. refusals, an undisturbed run
def test_refusals_and_an_undisturbed_run(small):
    s = small["full"]
    h, data = s["h"], s["data"]
    ARG, STATE, UNSUP = 1, 4, 6
    q0 = s["q0"]
    for bad in (dict(history_size=0), dict(history_size=11), dict(num_elbo_draws=0), dict(num_elbo_draws=256), dict(num_draws=-1),
                dict(draw_offset=-1), dict(path_offset=-1), dict(max_lbfgs_iters=0), dict(lbfgs_history_size=21), dict(init_alpha=0.0), dict(tol_grad=-1.0)):
        assert status_of(lambda: h.pathfinder(q0, **{**dict(num_draws=3, max_lbfgs_iters=5), **bad})) == ARG, bad
    assert status_of(lambda: h.pathfinder(None, 0)) == ARG
    x, g = np.array(s["res"]["x"][0][:3]), np.array(s["res"]["g"][0][:3])
    assert status_of(lambda: h.pathfinder_path(x, g, L=[3], num_draws=3)) == ARG and status_of(lambda: h.pathfinder_path(x, g, L=[-1], num_draws=3)) == ARG
    assert status_of(lambda: h.pathfinder_path(x[:1], g[:1], num_draws=3)) == ARG
    assert h.L.potus_pathfinder_timing(None) == ARG
    assert h.L.potus_pathfinder(12345, None, None, 1, None, None, None, None, None, None, None, None) == STATE
    assert h.L.potus_pathfinder(h.h, None, None, 1, None, None, None, None, None, None, None, None) == ARG            # null info_out
    hk = Handle(data, "full", chains=1, seed=1843, cus_per_chain=2, twin=0)
    assert hk.cus_per_chain == 2 and status_of(lambda: hk.pathfinder(q0, num_draws=3)) == UNSUP and status_of(lambda: hk.pathfinder_path(x, g, num_draws=3)) == UNSUP
    hk.close()
    hd = Handle(data, "full", chains=1, seed=1843, cus_per_chain=1, twin=0, metric=_abi.METRICS["dense_e"])
    assert status_of(lambda: hd.pathfinder(q0, num_draws=3)) == UNSUP
    hd.close()
    f = Handle(data, "full", chains=1, **OPTS)
    with pytest.raises(PotusError):
        f.pathfinder_scores()
    import ctypes as C
    import torch
    buf = torch.empty(4096, dtype=torch.float64, device="cuda:0")
    assert f.L.potus_pathfinder_write_array_device(f.h, 0, 8, C.c_void_p(buf.data_ptr())) == STATE
    f.pathfinder(q0[:1], num_draws=0, max_lbfgs_iters=5)
    assert f.L.potus_pathfinder_write_array_device(f.h, 0, 8, C.c_void_p(buf.data_ptr())) == STATE   # a call without draws keeps no rows
    f.pathfinder(q0[:1], num_draws=3, max_lbfgs_iters=5)
    assert status_of(lambda: f.pathfinder(q0[:1], num_draws=3, history_size=0)) == ARG
    assert f.L.potus_pathfinder_write_array_device(f.h, 0, 8, C.c_void_p(buf.data_ptr())) == 0       # a refused call leaves the last rows alone
    assert status_of(lambda: f.pathfinder_rows_device((5, 5))) == ARG and status_of(lambda: f.pathfinder_scores((3, 3))) == ARG
    f.close()
    # a sampling run with a refused and a successful call in its middle gives the bytes of an uninterrupted one
    run = dict(chains=2, num_warmup=20, num_samples=20, **OPTS)
    a, b = Handle(data, "full", **run), Handle(data, "full", **run)
    kw = dict(num_elbo_draws=5, **PF)
    before = b.pathfinder(q0, **kw)
    for x_ in (a, b):
        x_.init()
    a.run(40)
    b.run(20)
    assert status_of(lambda: b.pathfinder(q0, num_elbo_draws=0)) == ARG
    mid = b.pathfinder(q0, **kw)
    b.run(20)
    assert raw(before) == raw(mid) == raw(s["res"])
    assert a.draws().tobytes() == b.draws().tobytes() and a.chain_status() == b.chain_status()
    a.close()
    b.close()


def test_r_entry_point(small):
    import ctypes as C
    s = small["full"]
    h, res = s["h"], s["res"]
    n, D, rows = 2, h.D, ITER + 1
    info, elbo, kept = np.zeros((n, 4), np.int32), np.zeros((n, rows)), np.zeros((n, rows), np.int32)
    q, lp, lq, st = np.zeros((n, M, D)), np.zeros((n, M)), np.zeros((n, M)), (C.c_int * 1)(-1)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int))
    h.L.potus_R_pathfinder((C.c_int * 1)(h.h), (C.c_int * 9)(J, 5, M, 0, 0, ITER, 5, n, 1), (C.c_double * 6)(1e-3, 1e-12, 1e4, 1e-8, 1e7, 1e-8),
                           dp(np.ascontiguousarray(s["q0"])), ip(info), dp(elbo), ip(kept), dp(q), dp(lp), dp(lq), st)
    assert st[0] == 0
    got = dict(q=q, lp=lp, lq=lq, elbo=elbo, kept=kept, return_code=info[:, 0], iterations=info[:, 1], best_iteration=info[:, 2])
    assert raw(got) == raw(res)


# ------------------------------------------------------------------------------------------------ 8. inits and a statistical check
def test_inits_and_state_means():
    """PotusModel.pathfinder on the no-mode small design (strictly log-concave): 1 000 draws over 4 paths.  pf.inits(4) are distinct draws, one
    per path; PotusModel.sample(inits=pf.inits(4)) runs, and its first saved warm-up rows -- positions included -- are the oracle's transitions
    from exactly those rows (the rule of tests/test_gpu_options.py: the tree exactly, values to rtol 1e-6).  The election-day state means are
    within 5 combined MCSE of that NUTS run, by the rule of test_posterior_parity_small: std / sqrt(ESS) for NUTS, and for Pathfinder's
    independent draws std / sqrt(n) of the pooled draws -- the spread between the paths is NOT in the denominator."""
    from us_potus_model_amd import diagnostics as dg
    v = "no_mode_adjustment"
    data = synthetic.small(v)
    pf = PotusModel(v).pathfinder(data, paths=4, draws=1000)
    try:
        assert pf.draws.shape[0] == 1000 and (pf.return_code == 0).all() and np.isfinite(pf.log_ratio).all()
        assert (pf.best_iteration >= 1).all() and np.isfinite(pf.elbo).all()
        print("l*", pf.best_iteration.tolist(), "of", pf.iterations.tolist(), "elbo", pf.elbo.tolist(), "k-hat", pf.pareto_k, "sd log ratio", pf.log_ratio.std())
        init = pf.inits(4, seed=0)
        assert init.shape == (4, pf.draws.shape[1]) and len({r.tobytes() for r in init}) == 4
        for c in range(4):
            assert (pf.draws[c * 250:(c + 1) * 250] == init[c]).all(1).sum() == 1        # chain c starts from a draw of path c
        T, S = int(data["T"]), int(data["S"])
        sc = pf.scores().cpu().numpy()[:, 0, :]                                          # election day
        fit = PotusModel(v).sample(data, seed=1843, chains=4, iter_warmup=300, iter_sampling=250, refresh=550, save_warmup=True, inits=init,
                                   cus_per_chain=1, twin=0)
        d = fit._hs[0].draws()
        assert d.shape[:2] == (4, 550)
        m = OracleModel(data, v)
        o = m.default_opts(num_warmup=300, num_samples=250, seed=1843, fast_grad=0, save_warmup=1)
        for c in range(4):
            ref = m.sample_chain(c + 1, o, q0=init[c])[0]
            assert np.array_equal(d[c, :3, 3:6], ref[:3, 3:6]) and d[c, 0, 2] == ref[0, 2], c
            assert np.allclose(d[c, :3, 7:], ref[:3, 7:], rtol=1e-6, atol=1e-7) and np.allclose(d[c, :3, 0], ref[:3, 0], rtol=1e-6), c
        a, b, _ = fit._hs[0].layout["predicted_score"]
        post = np.ascontiguousarray(d[:, 300:, 7:]).reshape(1000, -1)
        nuts = fit._hs[0].constrain(post, a, b).reshape(4, 250, S, T)[..., T - 1]         # [chain, draw, state]
        z = np.zeros(S)
        for j in range(S):
            se = np.hypot(nuts[:, :, j].std() / np.sqrt(dg.ess_mean(nuts[:, :, j])), sc[:, j].std() / np.sqrt(sc.shape[0]))
            z[j] = abs(nuts[:, :, j].mean() - sc[:, j].mean()) / se
        for hh in fit._hs:
            hh.close()
        print("state means: NUTS", nuts.reshape(-1, S).mean(0), "Pathfinder", sc.mean(0), "z", z)
        assert (z <= 5.0).all()
    finally:
        pf.close()
