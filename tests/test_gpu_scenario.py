"""Conditional forecasts and the covariance of the state scores on the MI355X (potus_scenario.hpp) against the restatement tests/scenario_ref.py.

Counts and n_kept EQUAL.  Means: bit-equal on built blocks (grid values sum exactly in any order, one division), within 4 n 2^-53 max|x| on
fitted draws (a sum of n terms, both sides float64).  Covariances within 2 (n + 2) 2^-53 sqrt(v_i v_j), n = n_kept, v the reference's variances:
each of the n products is rounded once, the accumulation adds at most n 2^-53 relative to sum |d_i d_j| <= (n - 1) sqrt(v_i v_j), and the factor
2 covers the float64 reference's own error (at n = 4099 the bound is 9e-13).  Byte equality wherever the same draws arrive in the same order."""
import ctypes as C

import numpy as np
import pytest

import outcomes_ref
import scenario_ref as ref
from conftest import second_device
from test_gpu_outcomes import DAY_RANGES_254
from us_potus_model_amd import outcomes as oc, scenario as sc
from us_potus_model_amd.sampler import Handle, PotusError, run_many

pytestmark = pytest.mark.gpu
DP, I32, LL = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
INF = float("inf")
COUNTS = ("ev_hist", "tipping", "joint")
U = 2.0 ** -53


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


# ---- the generators of tests/test_gpu_outcomes.py
def _grid_weights(rng, S):
    """multiples of 2^-10 that sum to one: with scores on the same grid the national vote is exact in any summation order"""
    return (rng.multinomial(1024 - S, np.full(S, 1.0 / S)) + 1) / 1024.0


def _integer_ev(rng, S, total):
    return (rng.multinomial(total - S, np.full(S, 1.0 / S)) + 1).astype(np.int64)


def _built_block(rng, nd, ndays, S):
    ps = rng.integers(0, 1025, (nd, ndays, S)) / 1024.0
    ps[::7, :, S - 1] = ps[::7, :, 0]                     # tied states
    if S > 2:
        ps[3::11, :, 1] = ps[3::11, :, 2]
    flat = ps.reshape(nd * ndays, S)
    flat[1::13] = 0.5                                     # national vote exactly one half, every state tied
    flat[2::17] = 0.75                                    # all Democratic
    flat[5::19] = 0.25                                    # all Republican
    return ps


def _ev_for(S):
    base = np.arange(3, 3 + S)
    ev = np.floor(base * (538.0 / base.sum())).astype(np.int64)
    ev[0] += 538 - ev.sum()
    return ev


def _bounds(given, S):
    lo, hi = sc.parse_given(given, S)
    return lo, hi


def _device(ps, w, ev, given=None, day=-1, W=270):
    import torch
    return sc.scenario_of_block(torch.tensor(ps, device="cuda:0"), w, ev, given=given, day=day, ev_to_win=W)


def _cov_bound(want):
    v = np.diagonal(want["cov"], axis1=1, axis2=2)
    return 2.0 * (want["n_kept"] + 2) * U * np.sqrt(v[:, :, None] * v[:, None, :])


def _assert_counts(got, want, what=""):
    assert got.n_kept == want["n_kept"] and got.n_draws == want["n_draws"], (what, got.n_kept, want["n_kept"])
    assert got.outcomes.n_draws == want["n_kept"]
    for k in COUNTS:
        g = getattr(got.outcomes, k)
        assert g.shape == want[k].shape and g.dtype == np.int64 and np.array_equal(g, want[k]), (what, k)


def _assert_cov(got, want, what=""):
    err, bound = np.abs(got.cov - want["cov"]), _cov_bound(want)
    ratio = err / bound
    print(f"{what}: n_kept {want['n_kept']}, max |cov - ref| / bound: states {float(ratio[:, :-1, :-1].max()):.3f}, national row {float(ratio[:, -1, :].max()):.3f}")
    assert (err <= bound).all(), (what, float((err / bound).max()))
    assert np.array_equal(got.cov, got.cov.transpose(0, 2, 1)), what               # symmetric bit for bit


def _bytes(r):
    return (r.n_kept, r.n_draws, r.mean.tobytes(), r.cov.tobytes()) + tuple(getattr(r.outcomes, k).tobytes() for k in COUNTS)


TIGHT = {0: "win", 1: "lose", "national": (0.46875, 0.53125)}
LOOSE = {0: "win"}
KEPT = {(3, 1000, 1): (27, 469), (15, 260, 2): (20, 127), (17, 4099, 2): (302, 1929), (33, 515, 3): (39, 239), (47, 131, 1): (13, 62),
        (51, 777, 5): (93, 361), (63, 300, 2): (44, 144)}


# 1. built blocks through potus_scenario_device: columns S + 1 = 4, 16, 18, 34, 48, 52, 64 -- every NT and both exact tile edges
@pytest.mark.parametrize("S,nd,ndays", sorted(KEPT))
def test_built_blocks_equal_the_restatement(S, nd, ndays):
    rng = np.random.default_rng(1000 * S + nd)
    ps, w = _built_block(rng, nd, ndays, S), _grid_weights(rng, S)
    ev = _integer_ev(rng, S, 538)
    assert w.sum() == 1.0
    for name, given in (("tight", TIGHT), ("loose", LOOSE), ("none", None)):
        what = f"S={S} nd={nd} days={ndays} {name}"
        lo, hi = _bounds(given, S)
        want = ref.scenario(ps, w, ndays - 1, lo, hi, ev=ev)
        if given is not None:                                        # a generator change is loud
            assert want["n_kept"] == KEPT[(S, nd, ndays)][name == "loose"], (what, want["n_kept"])
            x = np.concatenate([ps[:, -1], want["nat_cond"][:, None]], axis=1)
            assert ((x == lo[None, :]) | (x == hi[None, :])).any(), "no draw on a bound: the half-open rule is not exercised"
        else:
            assert want["n_kept"] == nd
        got = _device(ps, w, ev, given)
        _assert_counts(got, want, what)
        assert got.mean.tobytes() == want["mean"].tobytes(), (what, float(np.abs(got.mean - want["mean"]).max()))
        _assert_cov(got, want, what)
        assert got.probability == want["n_kept"] / nd
        again = _device(ps, w, ev, given)
        assert _bytes(again) == _bytes(got), what
        if given is None:
            o = oc.outcomes_of_block(__import__("torch").tensor(ps, device="cuda:0"), w, ev)
            for k in COUNTS:
                assert np.array_equal(getattr(got.outcomes, k), getattr(o, k)), (what, k)
    # the moments alone: no electoral votes, no counts
    m = _device(ps, w, None, LOOSE)
    assert m.outcomes is None and m.n_kept == KEPT[(S, nd, ndays)][1]


# 2. degenerate keeps
def test_no_draw_kept():
    rng = np.random.default_rng(2)
    S = 5
    ps, w, ev = _built_block(rng, 300, 2, S), _grid_weights(rng, S), _integer_ev(rng, S, 538)
    got = _device(ps, w, ev, {2: (2.0, None)})
    assert got.n_kept == 0 and got.n_draws == 300 and got.probability == 0.0
    assert np.isnan(got.mean).all() and np.isnan(got.cov).all() and got.mean.shape == (2, S + 1) and got.cov.shape == (2, S + 1, S + 1)
    assert all(not getattr(got.outcomes, k).any() for k in COUNTS)


def test_one_draw_kept():
    rng = np.random.default_rng(3)
    S, nd = 17, 700
    ps, w, ev = rng.integers(0, 513, (nd, 2, S)) / 1024.0, _grid_weights(rng, S), _integer_ev(rng, S, 538)
    ps[611, 1, 4] = 0.9375
    got = _device(ps, w, ev, {4: (0.75, None)})
    want = ref.scenario(ps, w, 1, *_bounds({4: (0.75, None)}, S), ev=ev)
    assert got.n_kept == 1 == want["n_kept"]
    assert np.array_equal(got.mean[:, :S], ps[611]) and got.mean.tobytes() == want["mean"].tobytes()
    assert np.isnan(got.cov).all()
    _assert_counts(got, want)


def test_condition_on_the_first_day_of_three():
    rng = np.random.default_rng(4)
    S, nd = 33, 1500
    ps, w, ev = _built_block(rng, nd, 3, S), _grid_weights(rng, S), _integer_ev(rng, S, 538)
    given = {0: "win", "national": (None, 0.515625)}
    want = ref.scenario(ps, w, 0, *_bounds(given, S), ev=ev)
    last = ref.keep_mask(ps[:, 2], w, *_bounds(given, S))[0]
    assert 100 < want["n_kept"] < nd and not np.array_equal(last, want["keep"])     # the day matters
    got = _device(ps, w, ev, given, day=0)
    _assert_counts(got, want)
    assert got.mean.tobytes() == want["mean"].tobytes()
    _assert_cov(got, want, "first day of three")


# 3. fitted draws through potus_scenario
def _fit(data, variant, chains=4, nw=60, ns=40, seed=5, **kw):
    h = Handle(data, variant, chains=chains, num_warmup=nw, num_samples=ns, seed=seed, cus_per_chain=1, twin=0, **kw)
    h.init()
    h.run(nw + ns)
    return h


def _canonical(h, first=0):
    """[draw, T, S] of the handle's saved rows from `first` on, chain after chain (write_array: [iteration, chain, t + T s])"""
    S, T = int(h.data["S"]), int(h.data["T"])
    a, b, _ = h.layout["predicted_score"]
    n = h.draws_saved()
    return np.ascontiguousarray(h.write_array(a, b, n)[first:].transpose(1, 0, 2).reshape((n - first) * h.opts.chains, S, T).transpose(0, 2, 1))


@pytest.fixture(scope="module")
def fitted(cases):
    out = {}
    for name, ns in (("small_full", 150), ("2016", 40)):
        data, variant = cases[name]
        h = _fit(data, variant, ns=ns)
        ps = _canonical(h)
        w = outcomes_ref.normalised_weights(h.data["state_weights"])
        out[name] = (h, ps, w, ref.nat_of(ps[:, -1], w))
    yield out
    for h, *_ in out.values():
        h.close()


def _in_play(ps):
    """(state whose election-day win share is closest to one half, that share)"""
    share = (ps[:, -1] > 0.5).mean(0)
    i = int(np.argmin(np.abs(share - 0.5)))
    return i, float(share[i])


def _condition(ps, nat):
    """from the restatement's own numbers: the state whose election-day win share is closest to one half is won, the national vote lies
    in (q25, q75] of the reference nat.  The six states of the synthetic small_full posterior are all decided (every win share is 0 or 1:
    printed below), so "won" keeps nothing or everything there; the state's score is then asked to lie above its own median instead --
    still a state and a national condition at once, still a kept share in [0.05, 0.6]."""
    i, share = _in_play(ps)
    q25, q75 = (float(q) for q in np.quantile(nat, [0.25, 0.75]))
    state = "win" if 0.05 <= share <= 0.95 else (float(np.median(ps[:, -1, i])), None)
    print(f"state {i}: win share {share:.4f} -> {state}; national in ({q25:.6f}, {q75:.6f}]")
    return i, {i: state, "national": (q25, q75)}, (q25, q75)


def _assert_generic(ps, nat, bounds):
    for b in (0.5,) + tuple(bounds):
        assert np.abs(nat - b).min() > 1e-9, f"a national vote within 1e-9 of {b}: change the seed, not the margin"
    srt = np.sort(ps, axis=2)
    assert (np.diff(srt, axis=2) > 0).all(), "two states of one draw have equal scores: change the seed"


@pytest.mark.parametrize("name", ["small_full", "2016"])
def test_fitted_draws_equal_the_restatement(fitted, name):
    h, ps, w, nat_T = fitted[name]
    S, T = int(h.data["S"]), int(h.data["T"])
    ev = _ev_for(S)
    i, given, q = _condition(ps, nat_T)
    lo, hi = _bounds(given, S)
    want = ref.scenario(ps, w, T - 1, lo, hi, ev=ev)
    n, nd = want["n_kept"], len(ps)
    assert 0.05 <= n / nd <= 0.6, n / nd
    _assert_generic(ps[want["keep"]], want["nat"], ())               # what the counts of the kept draws hang on, every day
    _assert_generic(ps[:, -1:], nat_T, q)                            # what the keep mask hangs on
    got = h.scenario(ev, given=given)
    _assert_counts(got, want, name)
    assert got.days == (0, T) and got.cond_day == T - 1
    x_max = max(float(np.abs(ps).max()), float(np.abs(want["nat"]).max()))
    err = float(np.abs(got.mean - want["mean"]).max())
    print(f"{name}: kept {n} of {nd}; max |mean - ref| {err:.3e}, bound {4 * n * U * x_max:.3e}")
    assert err <= 4 * n * U * x_max
    _assert_cov(got, want, name)
    # a day sub-range equals the rows of the whole range; (3, 9) leaves the condition day out: it is then cut on its own
    for d0, d1 in ((3, 9), (T - 2, T)):
        sub = sc.scenario([h], ev, given=given, days=(d0, d1))
        assert sub.n_kept == n and sub.mean.tobytes() == got.mean[d0:d1].tobytes() and sub.cov.tobytes() == got.cov[d0:d1].tobytes(), (d0, d1)
        for k in COUNTS:
            assert np.array_equal(getattr(sub.outcomes, k), getattr(got.outcomes, k)[d0:d1]), (d0, d1, k)
    if T == 254:
        # k_oc_days at the edges of its tiles of 64 days, the condition day outside the range every time (cut as a one-day block of its own):
        # election day for the ranges that end before it, day 0 -- state i above its median there -- for the two that hold it
        first = {i: (float(np.median(ps[:, 0, i])), None)}
        want0 = ref.scenario(ps, w, 0, *_bounds(first, S), ev=ev)
        full0 = sc.scenario([h], ev, given=first, day=0)
        assert 0 < want0["n_kept"] < nd
        _assert_counts(full0, want0, "2016, condition on day 0")
        for d0, d1 in DAY_RANGES_254:
            g, cd, full = (given, T - 1, got) if d1 < T else (first, 0, full0)
            assert not d0 <= cd < d1
            sub = sc.scenario([h], ev, given=g, day=cd, days=(d0, d1))
            assert sub.n_kept == full.n_kept and sub.days == (d0, d1) and sub.cond_day == cd
            assert sub.mean.tobytes() == full.mean[d0:d1].tobytes() and sub.cov.tobytes() == full.cov[d0:d1].tobytes(), (d0, d1)
            for k in COUNTS:
                assert np.array_equal(getattr(sub.outcomes, k), getattr(full.outcomes, k)[d0:d1]), (d0, d1, k)


@pytest.mark.parametrize("name", ["small_full", "2016"])
def test_one_win_condition_ties_to_potus_outcomes(fitted, name):
    h, ps, w, nat_T = fitted[name]
    S, T = int(h.data["S"]), int(h.data["T"])
    ev = _ev_for(S)
    i, share = _in_play(ps)
    full = h.outcomes(ev, days=(T - 1, T))
    cond = h.scenario(ev, given={i: "win"}, days=(T - 1, T))
    assert cond.n_kept == full.joint[0, i, i] == round(share * len(ps)) and full.n_draws == cond.n_draws == len(ps)
    assert name != "2016" or 0 < cond.n_kept < full.n_draws
    assert np.array_equal(np.diagonal(cond.outcomes.joint[0]), full.joint[0, :, i])
    assert np.array_equal(cond.outcomes.win_probability(), full.conditional(i)[S:S + 1])
    # win and lose partition the draws, and their counts add up to the unconditional ones
    lose = h.scenario(ev, given={i: "lose"}, days=(T - 1, T))
    assert cond.n_kept + lose.n_kept == full.n_draws
    for k in COUNTS:
        assert np.array_equal(getattr(cond.outcomes, k) + getattr(lose.outcomes, k), getattr(full, k)), k


@pytest.mark.parametrize("name", ["small_full", "2016"])
def test_unconditional_correlation_equals_corrcoef(fitted, name):
    h, ps, w, nat_T = fitted[name]
    S, T = int(h.data["S"]), int(h.data["T"])
    r = h.scenario(days=(T - 1, T))
    assert r.outcomes is None and r.n_kept == r.n_draws == len(ps) and r.probability == 1.0
    x = np.concatenate([ps[:, -1], nat_T[:, None]], axis=1)
    want = np.corrcoef(x, rowvar=False)
    assert np.abs(r.cor() - want).max() <= 1e-12
    assert np.abs(r.sd() - x.std(0, ddof=1)).max() <= 1e-12 * x.std(0, ddof=1).max()


# 4. pooling: one handle of four chains = two handles of two, byte for byte
def test_pooled_handles_give_the_bytes_of_one_handle(cases):
    data, variant = cases["small_full"]
    nw, ns = 60, 80
    kw = dict(num_warmup=nw, num_samples=ns, seed=9, cus_per_chain=1, twin=0)
    one = Handle(data, variant, chains=4, **kw)
    one.init()
    one.run(nw + ns)
    a = Handle(data, variant, chains=2, **kw)
    b = Handle(data, variant, chains=2, chain_id_offset=2, device=second_device(), **kw)
    a.init()
    b.init()
    run_many([a, b], nw + ns)
    assert np.concatenate([a.draws(), b.draws()]).tobytes() == one.draws().tobytes()
    S = int(data["S"])
    ev = _ev_for(S)
    ps = _canonical(one)
    w = outcomes_ref.normalised_weights(data["state_weights"])
    i, given, _ = _condition(ps, ref.nat_of(ps[:, -1], w))
    for g in (given, None):
        r1, r2, r3 = sc.scenario([one], ev, given=g), sc.scenario([a, b], ev, given=g), sc.scenario([one], ev, given=g)
        assert r1.n_draws == 4 * ns and (g is None or 0 < r1.n_kept < 4 * ns)
        assert _bytes(r1) == _bytes(r2) == _bytes(r3), g
    for h in (one, a, b):
        h.close()


def test_saved_warmup_rows_are_left_out(cases):
    data, variant = cases["small_full"]
    nw, ns = 60, 50
    h = _fit(data, variant, chains=2, nw=nw, ns=ns, seed=7, save_warmup=1)
    assert h.draws_saved() == nw + ns and h.post_warmup_saved() == ns
    S, T = int(data["S"]), int(data["T"])
    ps = _canonical(h, first=nw)
    w, ev = outcomes_ref.normalised_weights(data["state_weights"]), _ev_for(S)
    i, given, _ = _condition(ps, ref.nat_of(ps[:, -1], w))
    want = ref.scenario(ps[:, -2:], w, 1, *_bounds(given, S), ev=ev)
    got = h.scenario(ev, given=given, days=(T - 2, T))
    assert got.n_draws == 2 * ns and 0 < got.n_kept < 2 * ns
    _assert_counts(got, want)
    assert np.abs(got.mean - want["mean"]).max() <= 4 * want["n_kept"] * U
    _assert_cov(got, want, "save_warmup")
    h.close()


def test_event_timings_of_outcomes_and_scenario_are_positive(cases):
    """The HIP-event slots of the two getters after one call each on two chains x ten draws: a span that was recorded and read is finite and > 0."""
    data, variant = cases["small_full"]
    h = _fit(data, variant, chains=2, nw=20, ns=10, seed=7)
    ev = _ev_for(int(data["S"]))
    h.outcomes(ev)
    ms = oc.last_timing()
    assert np.isfinite(ms[2]) and ms[2] > 0, ms             # the counting kernel
    h.scenario(ev)
    ms = sc.last_timing()
    assert np.isfinite(ms[3]) and ms[3] > 0, ms             # the moments
    assert np.isfinite(ms[4]) and ms[4] > 0, ms             # the counts
    h.close()


# 5. refusals: a status with a message, never a fault, and the handle stays usable
def test_refusals(fitted, cases):
    import torch
    h = fitted["small_full"][0]
    data, variant = cases["small_full"]
    S, T = int(data["S"]), int(data["T"])
    ev = _ev_for(S)
    before = h.scenario(ev, given={0: "win"}, days=(T - 3, T))
    g = _fit(cases["small_nomode"][0], "no_mode_adjustment", chains=2, nw=5, ns=5)
    with pytest.raises(PotusError, match="another posterior"):
        sc.scenario([h, g], ev)
    with pytest.raises(PotusError, match="listed twice"):
        sc.scenario([h, h], ev)
    e = Handle(data, variant, chains=2, num_warmup=5, num_samples=5)
    e.init()
    with pytest.raises(PotusError, match="error 4.*at least one saved post-warm-up draw"):
        sc.scenario([e], ev)
    m = Handle(data, variant, chains=2, num_warmup=5, num_samples=5, cus_per_chain=1, twin=0)
    ys, yn = np.asarray(data["n_democrat_state"])[None], np.asarray(data["n_democrat_national"])[None]
    m.set_datasets(np.repeat(ys, 2, 0), np.repeat(yn, 2, 0))
    m.init()
    m.run(10)
    with pytest.raises(PotusError, match="error 4.*slice the chains per data set"):
        sc.scenario([m], ev)

    L = h.L
    ids = (C.c_int * 1)(h.h)
    free_lo, free_hi = np.full(S + 1, -INF), np.full(S + 1, INF)
    e32 = np.ascontiguousarray(ev, dtype=np.int32)
    hist = np.zeros((T, 539), np.int64)

    def pooled(cd=T - 1, lo=free_lo, hi=free_hi, d0=0, d1=T, ev_=e32, want_hist=False):
        return L.potus_scenario(ids, 1, cd, None if lo is None else lo.ctypes.data_as(DP), None if hi is None else hi.ctypes.data_as(DP), d0, d1,
                                None if ev_ is None else ev_.ctypes.data_as(I32), 270, None, None, None, None,
                                hist.ctypes.data_as(LL) if want_hist else None, None, None)

    def message():
        buf = C.create_string_buffer(512)
        L.potus_last_error(buf, 512)
        return buf.value.decode()
    bad = free_lo.copy()
    bad[S] = np.nan
    assert pooled(lo=bad) == 1 and "NaN" in message()
    bad = free_hi.copy()
    bad[1] = np.nan
    assert pooled(hi=bad) == 1 and "NaN" in message()
    lo2, hi2 = free_lo.copy(), free_hi.copy()
    lo2[2], hi2[2] = 0.5, 0.5
    assert pooled(lo=lo2, hi=hi2) == 1 and "empty" in message()
    lo2[2] = 0.6
    assert pooled(lo=lo2, hi=hi2) == 1 and "empty" in message()
    assert pooled(lo=None) == 1 and "together" in message()
    for cd in (-1, T):
        assert pooled(cd=cd) == 1 and "condition day" in message()
    for d0, d1 in ((-1, 3), (0, T + 1), (4, 4), (5, 2)):
        assert pooled(d0=d0, d1=d1) == 1 and "days" in message()
    assert pooled(ev_=None, want_hist=True) == 1 and "ev is null" in message()
    big = e32.copy()
    big[0] += 2048 - 538
    assert pooled(ev_=big) == 6 and "2047" in message()
    assert pooled() == 0 and pooled(ev_=None, lo=None, hi=None) == 0                      # every output pointer may be null
    # the device call: S = 64, a block that is not device memory of the device named, a device that is not there
    host = np.full((4, 1, S), 0.5)
    w = outcomes_ref.normalised_weights(data["state_weights"])

    def device(dev, ptr, S_=S, w_=w):
        return L.potus_scenario_device(dev, C.c_void_p(ptr), 4, 1, S_, w_.ctypes.data_as(DP), 0, None, None, None, 270, None, None, None, None, None, None)
    t64 = torch.full((4, 1, 64), 0.5, dtype=torch.float64, device="cuda:0")
    assert device(0, t64.data_ptr(), 64, np.full(64, 1 / 64)) == 6 and "S = 64" in message()
    assert device(0, host.ctypes.data) == 1 and "not device memory" in message()
    assert device(99, host.ctypes.data) == 2 and "no HIP device" in message()
    if torch.cuda.device_count() >= 2:
        t = torch.full((4, 1, S), 0.5, dtype=torch.float64, device="cuda:1")
        assert device(0, t.data_ptr()) == 1 and "not device memory" in message()
    t = torch.full((4, 1, S), 0.5, dtype=torch.float64, device="cuda:0")
    assert device(0, t.data_ptr()) == 0
    after = h.scenario(ev, given={0: "win"}, days=(T - 3, T))
    assert _bytes(before) == _bytes(after)
    for x in (g, e, m):
        x.close()


# 6. the .C() entry point gives the numbers of potus_scenario
def test_r_entry_point_gives_the_numbers_of_potus_scenario(fitted):
    h, ps, w, nat_T = fitted["small_full"]
    S, T = int(h.data["S"]), int(h.data["T"])
    ev = _ev_for(S)
    i, given, q = _condition(ps, nat_T)
    lo, hi = _bounds(given, S)
    e32 = np.ascontiguousarray(ev, dtype=np.int32)
    f = h.L.potus_R_scenario
    for moments, counts, days in ((1, 1, (0, T)), (1, 0, (T - 2, T)), (0, 1, (2, 5))):
        want = sc.scenario([h], ev, given=given, days=days)
        n = days[1] - days[0]
        nn, mean, cov = np.full(2, -1.0), np.full(n * (S + 1), -1.0), np.full(n * (S + 1) ** 2, -1.0)
        hist, tip, joint = np.full(n * 539, -1.0), np.full(n * (S + 1), -1.0), np.full(n * (S + 2) ** 2, -1.0)
        st = C.c_int(-1)
        f((C.c_int * 1)(h.h), C.byref(C.c_int(1)), (C.c_int * 7)(T - 1, days[0], days[1], 270, 1, moments, counts), lo.ctypes.data_as(DP), hi.ctypes.data_as(DP),
          e32.ctypes.data_as(C.POINTER(C.c_int)), nn.ctypes.data_as(DP), mean.ctypes.data_as(DP), cov.ctypes.data_as(DP), hist.ctypes.data_as(DP),
          tip.ctypes.data_as(DP), joint.ctypes.data_as(DP), C.byref(st))
        assert st.value == 0 and nn[0] == want.n_kept and nn[1] == want.n_draws
        if moments:
            assert mean.tobytes() == want.mean.tobytes() and cov.tobytes() == want.cov.tobytes()
        else:
            assert (mean == -1.0).all() and (cov == -1.0).all()                           # left alone when not asked for
        if counts:
            assert np.array_equal(hist, want.outcomes.ev_hist.reshape(-1)) and np.array_equal(tip, want.outcomes.tipping.reshape(-1))
            assert np.array_equal(joint, want.outcomes.joint.reshape(-1))
        else:
            assert (hist == -1.0).all() and (tip == -1.0).all() and (joint == -1.0).all()
    # no bounds given: every draw is kept, whatever lo and hi hold
    st = C.c_int(-1)
    f((C.c_int * 1)(h.h), C.byref(C.c_int(1)), (C.c_int * 7)(T - 1, 0, T, 270, 0, 0, 0), lo.ctypes.data_as(DP), hi.ctypes.data_as(DP),
      e32.ctypes.data_as(C.POINTER(C.c_int)), nn.ctypes.data_as(DP), mean.ctypes.data_as(DP), cov.ctypes.data_as(DP), hist.ctypes.data_as(DP),
      tip.ctypes.data_as(DP), joint.ctypes.data_as(DP), C.byref(st))
    assert st.value == 0 and nn[0] == nn[1] == len(ps)
    st = C.c_int(-1)
    f((C.c_int * 1)(h.h), C.byref(C.c_int(1)), (C.c_int * 7)(T - 1, 3, 3, 270, 1, 1, 1), lo.ctypes.data_as(DP), hi.ctypes.data_as(DP),
      e32.ctypes.data_as(C.POINTER(C.c_int)), nn.ctypes.data_as(DP), mean.ctypes.data_as(DP), cov.ctypes.data_as(DP), hist.ctypes.data_as(DP),
      tip.ctypes.data_as(DP), joint.ctypes.data_as(DP), C.byref(st))
    assert st.value == 1
