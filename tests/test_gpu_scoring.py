"""The scoring rules of the joint forecast on the MI355X (potus_fscore.hpp) against the restatement tests/scoring_ref.py.

Every score within |got - want| <= 1e-10 + 1e-9 |want| of the restatement (the bar potus_diagnostics and the sorted-run tests hold theirs to); pit_lo and
pit_hi are integer ratios and EQUAL.  Byte equality wherever the same draws arrive in the same order.  The built blocks sit on a grid of 2^-20
with weights on a grid of 2^-10, so that the national vote of a draw is exact in any summation order and a result that equals a draw ties exactly."""
import ctypes as C
import functools

import numpy as np
import pytest

import outcomes_ref
import scoring_ref as ref
from conftest import second_device
from test_gpu_scenario import _canonical, _ev_for, _fit, _grid_weights
from us_potus_model_amd import _abi, scoring as fs, timeline
from us_potus_model_amd.sampler import Handle, PotusError, run_many

pytestmark = pytest.mark.gpu
DP, I32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
TILE = 128                                                                 # FS_TILE of potus_fscore.hpp


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def _block(rng, n, nd, S, rho=0.8):
    """Correlated scores around one half (correlation rho <= 0.9 between the states), on the grid of 2^-20."""
    L = np.linalg.cholesky(rho * np.ones((S, S)) + (1 - rho) * np.eye(S))
    x = 0.5 + 0.04 * rng.normal(size=(n, nd, S)) @ L.T + 0.02 * rng.normal(size=(1, nd, S))
    return np.clip(np.round(x * 2.0 ** 20), 1, 2 ** 20 - 1) / 2.0 ** 20


def _actual(rng, S, w, ev):
    y = np.round((0.5 + 0.05 * rng.normal(size=S)) * 2.0 ** 20) / 2.0 ** 20
    return ref.full_actual(y, w, ev)


def _use(S, m):
    u = np.ones(S, np.int32)
    if m < S:
        u[np.linspace(0, S - 1, S - m).astype(int) if S - m > 1 else [S // 2]] = 0
    assert u.sum() == m
    return u


def _device(ps, w, ev, actual, use=None, vs_p=0.5):
    import torch
    return fs.score_of_block(torch.tensor(np.ascontiguousarray(ps), device="cuda:0"), w, ev, actual, use=use, vs_p=vs_p)


def _close(got, want, what, worst=None):
    """NaN where the restatement has NaN, and nowhere else; the tolerance everywhere else."""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(np.isnan(got) != np.isnan(want))[:4])
    ok = ~np.isnan(want)
    err, tol = np.abs(got[ok] - want[ok]), 1e-10 + 1e-9 * np.abs(want[ok])
    if err.size:
        k = int(np.argmax(err / tol))
        print(f"{what}: worst |got - want| {err[k]:.3e} at |want| {abs(want[ok][k]):.3e} ({err[k] / tol[k]:.2e} of the tolerance)")
        assert (err <= tol).all(), (what, float(err[k]), float(want[ok][k]))


def _assert_scores(got, uni, multi, what):
    for k, name in enumerate(ref.UNI):
        if name.startswith("pit"):
            assert np.array_equal(got.uni[..., k], uni[..., k], equal_nan=True), (what, name)
        else:
            _close(got.uni[..., k], uni[..., k], f"{what} {name}")
    for k, name in enumerate(fs.MULTI):
        _close(got.multi[..., k], multi[..., k], f"{what} {name}")


def _bytes(r):
    return r.uni.tobytes(), r.multi.tobytes()


# (draws, S, used states, days): every draw count the issue names around the tile of 128, S = 1, 2, 51, 63, m = 1, S - 1, S
CASES = [(1, 1, 1, 1), (2, 2, 1, 1), (2, 2, 2, 3), (TILE - 1, 51, 50, 1), (TILE, 63, 63, 1), (TILE + 1, 2, 2, 3), (TILE + 1, 51, 1, 1),
         (2 * TILE + 1, 63, 62, 1), (2 * TILE + 1, 51, 51, 1), (5 * TILE + 3, 51, 50, 3), (5 * TILE + 3, 2, 1, 1), (TILE, 1, 1, 3)]


@functools.lru_cache(maxsize=None)
def _case(n, S, m, nd):
    """The block, its arguments and the restatement's scores: computed once, shared, read-only."""
    rng = np.random.default_rng(100000 * n + 100 * S + 10 * m + nd)
    ps, w, ev = _block(rng, n, nd, S), _grid_weights(rng, S), _ev_for(S).astype(np.float64)
    actual, use = _actual(rng, S, w, ev), _use(S, m)
    uni, multi = ref.scores(ps, w, ev, actual, use)
    for a in (ps, w, ev, actual, use, uni, multi):
        a.setflags(write=False)
    return ps, w, ev, actual, use, uni, multi


@pytest.mark.parametrize("n,S,m,nd", CASES)
def test_built_blocks_equal_the_restatement(n, S, m, nd):
    ps, w, ev, actual, use, uni, multi = _case(n, S, m, nd)
    assert w.sum() == 1.0
    got = _device(ps, w, ev, actual, use)
    what = f"n={n} S={S} m={m} days={nd}"
    assert got.n_draws == n and got.uni.shape == (nd, S + 2, 7) and got.multi.shape == (nd, 3)
    _assert_scores(got, uni, multi, what)
    assert np.isnan(multi[:, 2]).all() == (n <= m) and np.isfinite(got.multi[:, :2]).all()
    assert np.isfinite(got.uni[..., [0, 1, 2, 4, 5, 6]]).all() and (m > 1 or (got.variogram == 0.0).all())
    assert _bytes(_device(ps, w, ev, actual, use)) == _bytes(got), what
    # a day alone has the bytes it has inside the range
    if nd > 1:
        one = _device(ps[:, 1:2], w, ev, actual, use)
        assert one.uni.tobytes() == got.uni[1:2].tobytes() and one.multi.tobytes() == got.multi[1:2].tobytes(), what


def test_more_tile_jobs_than_workgroups():
    """5 * 128 + 3 draws are 21 tiles of pairs a day; 200 days are 4200 tile jobs for the 4096 workgroups of the launch.  The days repeat the three of
    the case above, which the restatement has checked: every day must hold the bytes of its day there."""
    n, S, m, nd = 5 * TILE + 3, 2, 1, 1
    ps, w, ev, actual, use, uni, multi = _case(n, S, m, nd)
    rng = np.random.default_rng(77)
    three = np.concatenate([ps, _block(rng, n, 2, S)], axis=1)
    base = _device(three, w, ev, actual, use)
    assert base.uni[:1].tobytes() == _device(ps, w, ev, actual, use).uni.tobytes()
    _assert_scores(_device(ps, w, ev, actual, use), uni, multi, "one day of the three")
    days = 200
    assert days * 21 > 4096
    many = _device(three[:, np.arange(days) % 3], w, ev, actual, use)
    for t in range(days):
        assert many.uni[t].tobytes() == base.uni[t % 3].tobytes() and many.multi[t].tobytes() == base.multi[t % 3].tobytes(), t


def test_ties():
    """Duplicated draws, a result that equals a draw in every state, a constant column: distances of exactly 0, pit_lo < pit_hi, and the
    univariate dss NaN for the constant column alone with crps = |x - y|."""
    rng = np.random.default_rng(5)
    n, S = TILE + 37, 5
    ps, w, ev = _block(rng, n, 2, S), _grid_weights(rng, S), _ev_for(S).astype(np.float64)
    ps[1::3] = ps[0]                                                       # every third draw is draw 0, in both days
    ps[:, :, 3] = 0.4375                                                   # a constant column
    y = ps[0, 0].copy()                                                    # the result is draw 0 of day 0 in every state but the constant one
    y[3] = 0.5
    actual = ref.full_actual(y, w, ev)
    x0, free = ps[:, 0], [0, 1, 2, 4, S + 1]                               # (the votes of draw 0 are the result's: 0.4375 and 0.5 both lose state 3)
    assert (np.sqrt(((x0[:, None] - x0[None]) ** 2).sum(-1)) == 0).sum() > n and (x0[:, free[:4]] == actual[free[:4]]).all(axis=1).sum() > 1
    uni, multi = ref.scores(ps, w, ev, actual)
    got = _device(ps, w, ev, actual)
    _assert_scores(got, uni, multi, "ties")
    assert (got.pit[0, free, 0] < got.pit[0, free, 1]).all()
    assert np.isnan(got.dss[:, 3]).all() and np.isfinite(np.delete(got.dss, 3, axis=1)).all()
    assert np.array_equal(got.crps[:, 3], [0.0625, 0.0625]) and (got.pit[:, 3] == 1.0).all()
    assert np.isnan(got.dss_joint).all() and np.isfinite(got.energy).all() and np.isfinite(got.variogram).all()     # a constant state: no factor
    # without the constant state the joint score is there
    u = np.array([1, 1, 1, 0, 1], np.int32)
    got_u = _device(ps, w, ev, actual, use=u)
    uni_u, multi_u = ref.scores(ps, w, ev, actual, u)
    _assert_scores(got_u, uni_u, multi_u, "ties, the constant state left out")
    assert np.isfinite(got_u.multi).all() and got_u.uni.tobytes() == got.uni.tobytes()


def test_fewer_draws_than_used_states():
    rng = np.random.default_rng(6)
    for n, S in ((51, 51), (20, 63), (1, 2)):
        ps, w, ev = _block(rng, n, 1, S), _grid_weights(rng, S), _ev_for(S).astype(np.float64)
        actual = _actual(rng, S, w, ev)
        got = _device(ps, w, ev, actual)                                   # status OK
        assert np.isnan(got.dss_joint).all() and np.isfinite(got.energy).all() and np.isfinite(got.variogram).all()
        assert np.isfinite(np.delete(got.uni, 3, axis=-1)).all() and (n == 1 or np.isfinite(got.dss[:, :S + 1]).all())
        _assert_scores(got, *ref.scores(ps, w, ev, actual), f"n={n} <= m={S}")


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_value_that_is_not_finite_spoils_its_day_alone(bad):
    rng = np.random.default_rng(7)
    n, S = 2 * TILE + 5, 7
    ps, w, ev = _block(rng, n, 3, S), _grid_weights(rng, S), _ev_for(S).astype(np.float64)
    actual = _actual(rng, S, w, ev)
    clean = _device(ps, w, ev, actual)
    assert np.isfinite(clean.uni).all() and np.isfinite(clean.multi).all()
    dirty = ps.copy()
    dirty[n // 2, 1, 2] = bad
    for use, joint_nan in ((None, True), (np.array([1, 1, 0, 1, 1, 1, 1], np.int32), False)):
        ref_clean = _device(ps, w, ev, actual, use=use)
        got = _device(dirty, w, ev, actual, use=use)
        for t in (0, 2):
            assert got.uni[t].tobytes() == ref_clean.uni[t].tobytes() and got.multi[t].tobytes() == ref_clean.multi[t].tobytes(), t
        assert np.isnan(got.uni[1, [2, S, S + 1]]).all()
        others = [0, 1, 3, 4, 5, 6]
        assert got.uni[1, others].tobytes() == ref_clean.uni[1, others].tobytes()
        if joint_nan:
            assert np.isnan(got.multi[1]).all()
        else:
            assert got.multi[1].tobytes() == ref_clean.multi[1].tobytes()
        uni, multi = ref.scores(dirty, w, ev, actual, use)
        assert np.array_equal(np.isnan(got.uni), np.isnan(uni)) and np.array_equal(np.isnan(got.multi), np.isnan(multi))


def test_other_orders_of_the_variogram_score():
    rng = np.random.default_rng(8)
    ps5 = _block(rng, 300, 1, 5)
    w5, ev5 = _grid_weights(rng, 5), _ev_for(5).astype(np.float64)
    a5 = _actual(rng, 5, w5, ev5)
    for p in (1.0, 2.0, 0.75):
        got = _device(ps5, w5, ev5, a5, vs_p=p)
        want = np.array([ref.variogram(ps5[:, 0], a5[:5], p)])
        _close(got.variogram, want, f"variogram score of order {p}")


# ---- fitted draws
@pytest.fixture(scope="module")
def fitted(cases):
    data, variant = cases["small_full"]
    h = _fit(data, variant, ns=80)
    ps = _canonical(h)
    w = outcomes_ref.normalised_weights(h.data["state_weights"])
    yield h, ps, w
    h.close()


def _result_for(ps, rng):
    """a result near the forecast: the election-day median of every state, moved by about one posterior sd"""
    x = ps[:, -1]
    return np.clip(np.median(x, axis=0) + x.std(axis=0) * rng.normal(size=x.shape[1]), 0.01, 0.99)


def test_a_short_fit_equals_the_restatement(fitted):
    h, ps, w = fitted
    S, T = int(h.data["S"]), int(h.data["T"])
    ev = _ev_for(S).astype(np.float64)
    y = _result_for(ps, np.random.default_rng(9))
    use = np.ones(S, np.int32)
    use[S - 1] = 0
    d0, d1 = T - 3, T
    got = h.forecast_scores(ev, y, days=(d0, d1), use=use)
    assert got.n_draws == len(ps) == 320 and got.days == (d0, d1)
    actual = ref.full_actual(y, w, ev)
    assert np.array_equal(got.actual, actual)
    uni, multi = ref.scores(ps[:, d0:d1], w, ev, actual, use)
    _assert_scores(got, uni, multi, "small_full, the last three days")
    assert abs(got.rmse() - np.sqrt(np.mean((ps[:, -1].mean(0) - y)[:S - 1] ** 2))) <= 1e-12
    # the device entry on the extracted block, and a day alone
    blk = _device(ps[:, d0:d1], h.data["state_weights"], ev, actual, use)   # (the weights as the handle has them: normalised once)
    assert _bytes(blk) == _bytes(got)
    one = h.forecast_scores(ev, y, days=(T - 2, T - 1), use=use)
    assert one.uni.tobytes() == got.uni[1:2].tobytes() and one.multi.tobytes() == got.multi[1:2].tobytes()
    # against(): a forecast scored against itself
    d = got.against(h.forecast_scores(ev, y, days=(d0, d1), use=use))
    # (NaN - NaN where a column has no variance: the states of this small posterior are all decided, every draw has the same electoral votes)
    assert all(((v == 0) | np.isnan(v)).all() for v in d.values()) and np.array_equal(np.isnan(d["dss"]), np.isnan(got.dss))


def test_pooled_handles_give_the_bytes_of_one_handle(cases):
    data, variant = cases["small_full"]
    nw, ns = 60, 40
    kw = dict(num_warmup=nw, num_samples=ns, seed=9, cus_per_chain=1, twin=0)
    one = Handle(data, variant, chains=4, **kw)
    one.init()
    one.run(nw + ns)
    a = Handle(data, variant, chains=2, **kw)
    b = Handle(data, variant, chains=2, chain_id_offset=2, device=second_device(), **kw)
    a.init()
    b.init()
    run_many([a, b], nw + ns)
    S, T = int(data["S"]), int(data["T"])
    ev, y = _ev_for(S).astype(np.float64), _result_for(_canonical(one), np.random.default_rng(10))
    r1, r2 = fs.score([one], ev, y, days=(T - 2, T)), fs.score([a, b], ev, y, days=(T - 2, T))
    assert r1.n_draws == r2.n_draws == 4 * ns and _bytes(r1) == _bytes(r2)
    for h in (one, a, b):
        h.close()


def test_saved_warmup_rows_are_left_out(cases):
    data, variant = cases["small_full"]
    nw, ns = 60, 50
    h = _fit(data, variant, chains=2, nw=nw, ns=ns, seed=7, save_warmup=1)
    assert h.draws_saved() == nw + ns
    S, T = int(data["S"]), int(data["T"])
    ps = _canonical(h, first=nw)
    w, ev = outcomes_ref.normalised_weights(data["state_weights"]), _ev_for(S).astype(np.float64)
    y = _result_for(ps, np.random.default_rng(11))
    got = h.forecast_scores(ev, y, days=(T - 1, T))
    assert got.n_draws == 2 * ns
    assert _bytes(got) == _bytes(_device(ps[:, -1:], data["state_weights"], ev, ref.full_actual(y, w, ev)))
    h.close()


def test_the_approximations_are_scored_against_nuts_day_for_day(fitted, cases):
    """Laplace, Pathfinder and ADVI .forecast_scores: the scores of score_of_block on their draws' block, labelled with the days of the design, so
    that .against() a NUTS result of the same days gives the differences score by score (and refuses other days)."""
    from us_potus_model_amd.sampler import PotusModel
    h, ps, w = fitted
    data, variant = cases["small_full"]
    S, T = int(data["S"]), int(data["T"])
    ev = _ev_for(S).astype(np.float64)
    y = _result_for(ps, np.random.default_rng(15))
    use = np.ones(S, np.int32)
    use[0] = 0
    nuts_last, nuts_three = h.forecast_scores(ev, y, use=use), h.forecast_scores(ev, y, use=use, days=(T - 3, T))
    assert nuts_last.days == (T - 1, T) and nuts_last.uni.tobytes() == nuts_three.uni[2:].tobytes()        # the default: election day alone
    model = PotusModel(variant)
    fits = (model.laplace(data, draws=200), model.pathfinder(data, paths=2, draws=200),
            model.variational(data, iter=400, eval_elbo=100, output_samples=200))
    for a in fits:
        name = type(a).__name__
        for days, nuts in ((None, nuts_last), ((T - 3, T), nuts_three)):
            got = a.forecast_scores(ev, y, days=days, use=use)
            assert got.days == nuts.days and got.uni.shape == nuts.uni.shape and np.isfinite(got.multi).all(), name
            blk = fs.score_of_block(a.scores(days).contiguous(), data["state_weights"], ev, y, use=use)
            assert blk.days == (0, nuts.uni.shape[0]) and _bytes(blk) == _bytes(got), name
            d = got.against(nuts)
            assert set(d) == set(fs.SCORES) and np.array_equal(d["energy"], got.energy - nuts.energy) and np.array_equal(d["crps"], got.crps - nuts.crps), name
            print(f"{name} against NUTS, days {got.days}: energy {d['energy']}, rmse {got.rmse():.5f} / {nuts.rmse():.5f}")
        with pytest.raises(ValueError, match="same days"):
            a.forecast_scores(ev, y, use=use).against(nuts_three)
        a.close()


# ---- run dates as data sets
def _two_dates():
    from test_gpu_timeline import drop_set
    from us_potus_model_amd import synthetic
    data = synthetic.small("full")
    ks, kn, _, _ = drop_set(data)
    Ns, Nn = int(data["N_state_polls"]), int(data["N_national_polls"])
    prior = np.tile(np.asarray(data["mu_b_prior"], dtype=np.float64), (2, 1))
    return timeline.design_of(data, np.stack([np.ones(Ns, bool), ks]), np.stack([np.ones(Nn, bool), kn]), prior, np.full(2, data["mu_b_T_scale"]))


def _fit_dates(design, q0=None, cpd=2, nw=40, ns=30):
    h = Handle(design["data"], "full", chains=2 * cpd, num_warmup=nw, num_samples=ns, seed=1843, cus_per_chain=1, twin=0)
    timeline.set_design(h, design)
    h.init(q0)
    h.run(nw + ns)
    return h


def test_every_run_date_equals_its_slice_and_a_failed_chain_fails_its_date_alone():
    design = _two_dates()
    data = design["data"]
    S, T = int(data["S"]), int(data["T"])
    D = _abi.num_params(data, "full")
    q0 = 0.1 * np.random.default_rng(11).standard_normal((4, D))
    ev = _ev_for(S).astype(np.float64)
    h = _fit_dates(design, q0)
    t = timeline.Timeline(h, design, 2)
    x = h.timeline_scores_device((T - 2, T))                               # [dates, draws, days, S]
    y = _result_for(x[0].cpu().numpy(), np.random.default_rng(12))
    got = t.forecast_scores(ev, y, days=(T - 2, T))
    assert got.uni.shape == (2, 2, S + 2, 7) and got.multi.shape == (2, 2, 3) and got.n_draws.tolist() == [60, 60]
    assert np.isfinite(got.multi).all()
    for d in range(2):
        alone = fs.score_of_block(x[d].contiguous(), data["state_weights"], ev, y)
        assert alone.uni.tobytes() == got.uni[d].tobytes() and alone.multi.tobytes() == got.multi[d].tobytes(), d
    assert t.forecast_scores(ev, y).uni.tobytes() == got.uni[:, 1:].tobytes()                # the default: election day alone
    ms = fs.last_timing()
    assert all(np.isfinite(v) and v > 0 for v in ms), ms
    h.close()
    bad_q0 = q0.copy()
    bad_q0[3] = 1e308                                                      # a non-finite log density: an error status of chain 3, run date 1
    bad = _fit_dates(design, bad_q0)
    assert bad.chain_status()[0][3] != 0
    r = timeline.Timeline(bad, design, 2).forecast_scores(ev, y, days=(T - 2, T))
    assert r.n_draws.tolist() == [60, 0] and np.isnan(r.uni[1]).all() and np.isnan(r.multi[1]).all()
    assert r.uni[0].tobytes() == got.uni[0].tobytes() and r.multi[0].tobytes() == got.multi[0].tobytes()
    bad.close()


# ---- refusals, the .C() entry, timings
def test_refusals(fitted, cases):
    import torch
    h, ps, w = fitted
    data, variant = cases["small_full"]
    S, T = int(data["S"]), int(data["T"])
    L = h.L
    ev = _ev_for(S).astype(np.float64)
    actual = ref.full_actual(_result_for(ps, np.random.default_rng(13)), w, ev)
    use = np.ones(S, np.int32)
    before = h.forecast_scores(ev, actual, days=(T - 1, T))
    uni, multi = np.zeros((T, S + 2, 7)), np.zeros((T, 3))
    ids = (C.c_int * 1)(h.h)

    def message():
        buf = C.create_string_buffer(512)
        L.potus_last_error(buf, 512)
        return buf.value.decode()

    def pooled(d0=T - 1, d1=T, ev_=ev, actual_=actual, use_=use, p=0.5, out=uni):
        return L.potus_forecast_scores(ids, 1, d0, d1, None if ev_ is None else ev_.ctypes.data_as(DP), 270, None if actual_ is None else actual_.ctypes.data_as(DP),
                                       None if use_ is None else use_.ctypes.data_as(I32), p, None if out is None else out.ctypes.data_as(DP),
                                       multi.ctypes.data_as(DP), None)
    for k, v, word in ((1, np.nan, "not finite"), (S, np.inf, "not finite"), (S + 1, np.nan, "not finite"), (0, 1.5, "outside [0, 1]"), (S, -0.1, "outside [0, 1]")):
        a = actual.copy()
        a[k] = v
        assert pooled(actual_=a) == 1 and word in message() and f"actual[{k}]" in message()
    assert pooled(use_=np.zeros(S, np.int32)) == 1 and "use is all zero" in message()
    for p in (0.0, -1.0, 2.5, np.nan):
        assert pooled(p=p) == 1 and "vs_p" in message() and "(0, 2]" in message()
    for d0, d1 in ((-1, 3), (0, T + 1), (4, 4), (5, 2)):
        assert pooled(d0=d0, d1=d1) == 1 and "bad day range" in message()
    for kw in (dict(ev_=None), dict(actual_=None), dict(use_=None), dict(out=None)):
        assert pooled(**kw) == 1 and "null" in message()
    assert pooled() == 0
    m = Handle(data, variant, chains=2, num_warmup=5, num_samples=5, cus_per_chain=1, twin=0)
    ys, yn = np.asarray(data["n_democrat_state"])[None], np.asarray(data["n_democrat_national"])[None]
    m.set_datasets(np.repeat(ys, 2, 0), np.repeat(yn, 2, 0))
    m.init()
    m.run(10)
    with pytest.raises(PotusError, match="error 4.*slice the chains per data set"):
        fs.score([m], ev, actual)
    m.close()
    # too many draws for a pooled posterior: refused from the options, before the device is touched
    big = Handle(data, variant, chains=2, num_warmup=1, num_samples=8193, cus_per_chain=1, twin=0)
    with pytest.raises(PotusError, match="error 6.*16386 draws.*at most 16384"):
        fs.score([big], ev, actual)
    big.close()

    def device(dev, ptr, n=4, S_=S, nd=1):
        w_, e_, a_, u_ = np.full(S_, 1.0 / S_), np.ones(S_), np.full(S_ + 2, 0.5), np.ones(S_, np.int32)
        return L.potus_forecast_scores_device(dev, C.c_void_p(ptr), n, nd, S_, w_.ctypes.data_as(DP), e_.ctypes.data_as(DP), 270, a_.ctypes.data_as(DP),
                                              u_.ctypes.data_as(I32), 0.5, uni.ctypes.data_as(DP), multi.ctypes.data_as(DP))
    t64 = torch.full((4, 1, 64), 0.5, dtype=torch.float64, device="cuda:0")
    assert device(0, t64.data_ptr(), S_=64) == 6 and "S = 64" in message()
    t = torch.full((4, 1, S), 0.5, dtype=torch.float64, device="cuda:0")
    assert device(0, t.data_ptr(), n=16385) == 6 and "16385 draws" in message() and "16384" in message()
    assert device(0, t.data_ptr(), n=0) == 1 and "0 draws" in message()
    assert device(0, t.data_ptr(), nd=0) == 1 and "bad day range" in message()
    assert device(0, None) == 1 and "null" in message()
    host = np.full((4, 1, S), 0.5)
    assert device(0, host.ctypes.data) == 1 and "not device memory" in message()
    assert device(0, t.data_ptr()) == 0
    after = h.forecast_scores(ev, actual, days=(T - 1, T))
    assert _bytes(before) == _bytes(after)


def test_r_entry_point_gives_the_numbers_of_the_c_call(fitted):
    h, ps, w = fitted
    S, T = int(h.data["S"]), int(h.data["T"])
    ev = _ev_for(S).astype(np.float64)
    actual = ref.full_actual(_result_for(ps, np.random.default_rng(14)), w, ev)
    use = np.ones(S, np.int32)
    use[0] = 0
    want = fs.score([h], ev, actual, days=(T - 2, T), use=use, vs_p=1.0)
    uni, multi, nn, st = np.full(2 * (S + 2) * 7, -1.0), np.full(2 * 3, -1.0), np.full(1, -1.0), C.c_int(-1)
    f = h.L.potus_R_forecast_scores
    f((C.c_int * 1)(h.h), C.byref(C.c_int(1)), (C.c_int * 3)(T - 2, T, 270), ev.ctypes.data_as(DP), actual.ctypes.data_as(DP), use.ctypes.data_as(C.POINTER(C.c_int)),
      C.byref(C.c_double(1.0)), uni.ctypes.data_as(DP), multi.ctypes.data_as(DP), nn.ctypes.data_as(DP), C.byref(st))
    assert st.value == 0 and nn[0] == want.n_draws
    assert uni.tobytes() == want.uni.tobytes() and multi.tobytes() == want.multi.tobytes()
    st = C.c_int(-1)
    f((C.c_int * 1)(h.h), C.byref(C.c_int(1)), (C.c_int * 3)(3, 3, 270), ev.ctypes.data_as(DP), actual.ctypes.data_as(DP), use.ctypes.data_as(C.POINTER(C.c_int)),
      C.byref(C.c_double(1.0)), uni.ctypes.data_as(DP), multi.ctypes.data_as(DP), nn.ctypes.data_as(DP), C.byref(st))
    assert st.value == 1


def test_event_timings_are_positive():
    ps, w, ev, actual, use, uni, multi = _case(2 * TILE + 1, 51, 51, 1)
    _device(ps, w, ev, actual, use)
    ms = fs.last_timing()
    assert len(ms) == 4 and all(np.isfinite(v) and v > 0 for v in ms), ms
