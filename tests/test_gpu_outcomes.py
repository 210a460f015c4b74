"""Joint election outcomes on the MI355X (potus_outcomes.hpp) against the restatement tests/outcomes_ref.py: every count EQUAL.  Built blocks
(ties, a national vote of exactly one half, all states one way, S = 3 / 51 / 63, odd draw counts, 1 and 254 days, votes that cannot reach the
bar), fitted draws, consistency with potus_posterior_summary, pooling over handles, refusals, the .C() path and the p-values of the 2016
backtest.  There is no tolerance to choose: the outputs are counts."""
import ctypes as C

import numpy as np
import pytest

import outcomes_ref as ref
from conftest import GOLD, readme_golden, second_device
from us_potus_model_amd import dataprep, outcomes as oc
from us_potus_model_amd.sampler import Handle, PotusError, run_many

pytestmark = pytest.mark.gpu
DP, I32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
KEYS = ("ev_hist", "tipping", "joint", "below_actual")
# day ranges of the 254 days of the 2016 design for k_oc_days, which cuts them in tiles of 64: one tile less a day, exactly, and a day; the
# same from day 1; the last 65 and 64 days; two days across the edge of the second tile
DAY_RANGES_254 = ((0, 63), (0, 64), (0, 65), (1, 65), (189, 254), (190, 254), (127, 129))


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


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


def _assert_equal(got, want, what=""):
    assert got.n_draws == want["n_draws"], what
    for k in KEYS:
        g, w = getattr(got, k), want[k]
        assert (g is None) == (w is None), (what, k)
        if w is not None:
            assert g.shape == w.shape and g.dtype == np.int64, (what, k, g.shape, w.shape)
            assert np.array_equal(g, w), (what, k, int(np.abs(g - w).sum()))


def _device(ps, w, ev, W=270, actual=None):
    import torch
    return oc.outcomes_of_block(torch.tensor(ps, device="cuda:0"), w, ev, actual=actual, ev_to_win=W)


# 4. built blocks through potus_outcomes_device
@pytest.mark.parametrize("S,nd,ndays,total,W", [
    (3, 1, 1, 538, 270),          # one draw
    (3, 1000, 1, 538, 270),
    (51, 777, 5, 538, 270),       # a draw count that is no multiple of 64 or of a workgroup's chunk
    (51, 37, 254, 538, 270),      # every day of the 2016 design
    (63, 300, 2, 538, 270),       # the most states the library takes
    (51, 500, 3, 200, 270),       # the votes cannot reach the bar: no tipping point, never an electoral-college win
    (63, 129, 1, 2047, 1024),     # the histogram's cap
])
def test_built_blocks_equal_the_restatement(S, nd, ndays, total, W):
    rng = np.random.default_rng(1000 * S + nd)
    ps, w, ev = _built_block(rng, nd, ndays, S), _grid_weights(rng, S), _integer_ev(rng, S, total)
    assert w.sum() == 1.0 and ev.sum() == total
    actual = rng.integers(0, 1025, S) / 1024.0           # on the grid: `x < actual` meets equality
    want = ref.outcomes(ps, w, ev, W, actual)
    assert nd * ndays < 2 or (want["nat"] == 0.5).any()
    assert (want["tipping"][:, S] > 0).all() == (total < W)
    got = _device(ps, w, ev, W, actual)
    _assert_equal(got, want, f"S={S} nd={nd} days={ndays}")
    assert got.ev_hist.shape == (ndays, total + 1)
    assert (got.ev_hist.sum(1) == nd).all() and (got.tipping.sum(1) == nd).all()
    # without `actual`: the same counts, no below_actual
    _assert_equal(_device(ps, w, ev, W), dict(want, below_actual=None))


# 8. no cap on the draws from a tile or a sorted run
def test_more_than_16384_draws():
    rng = np.random.default_rng(8)
    S, nd = 51, 20011
    ps, w, ev = _built_block(rng, nd, 1, S), _grid_weights(rng, S), _integer_ev(rng, S, 538)
    actual = rng.integers(0, 1025, S) / 1024.0
    want = ref.outcomes(ps, w, ev, 270, actual)
    a = _device(ps, w, ev, 270, actual)
    _assert_equal(a, want)
    b = _device(ps, w, ev, 270, actual)
    assert all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in KEYS)


def _fit(data, variant, chains=4, nw=60, ns=40, seed=5, **kw):
    h = Handle(data, variant, chains=chains, num_warmup=nw, num_samples=ns, seed=seed, cus_per_chain=1, twin=0, **kw)
    h.init()
    h.run(nw + ns)
    return h


def _predicted_score(h, first=0):
    """[draw, T, S] of the handle's saved rows from `first` on (write_array: [iteration, chain, t + T s])"""
    S, T = int(h.data["S"]), int(h.data["T"])
    a, b, _ = h.layout["predicted_score"]
    n = h.draws_saved()
    return h.write_array(a, b, n)[first:].reshape((n - first) * h.opts.chains, S, T).transpose(0, 2, 1)


def _ev_for(S):
    base = np.arange(3, 3 + S)
    ev = np.floor(base * (538.0 / base.sum())).astype(np.int64)
    ev[0] += 538 - ev.sum()
    return ev


def _assert_generic(ps, nat):
    """What makes the comparison independent of floating-point order: asserted on the restatement's own numbers, loudly."""
    assert np.abs(nat - 0.5).min() > 1e-9, "a national vote within 1e-9 of one half: change the seed, not the margin"
    srt = np.sort(ps, axis=2)
    assert (np.diff(srt, axis=2) > 0).all(), "two states of one draw have equal scores: change the seed"


@pytest.fixture(scope="module")
def fitted(cases):
    out = {}
    for name, ns in (("small_full", 150), ("2016", 40)):
        data, variant = cases[name]
        out[name] = _fit(data, variant, ns=ns)
    yield out
    for h in out.values():
        h.close()


# 5. fitted draws through potus_outcomes, all days
@pytest.mark.parametrize("name", ["small_full", "2016"])
def test_fitted_draws_equal_the_restatement(fitted, name):
    h = fitted[name]
    S = int(h.data["S"])
    ps = _predicted_score(h)
    w, ev = ref.normalised_weights(h.data["state_weights"]), _ev_for(S)
    actual = np.clip(ps[:, -1].mean(0) + 0.01 * np.cos(np.arange(S)), 0, 1)
    want = ref.outcomes(ps, w, ev, 270, actual)
    _assert_generic(ps, want["nat"])
    got = h.outcomes(ev, actual=actual)
    _assert_equal(got, want, name)
    assert got.days == (0, int(h.data["T"]))
    # a day range gives the rows of the whole range
    sub = oc.outcomes([h], ev, actual=actual, days=(3, 9))
    for k in KEYS:
        assert np.array_equal(getattr(sub, k), want[k][3:9]), k
    last = h.outcomes(ev, days=(int(h.data["T"]) - 1, int(h.data["T"])))
    assert np.array_equal(last.joint[0], want["joint"][-1]) and last.below_actual is None
    if int(h.data["T"]) == 254:                          # k_oc_days at the edges of its tiles of 64 days
        for d0, d1 in DAY_RANGES_254:
            sub = oc.outcomes([h], ev, actual=actual, days=(d0, d1))
            assert sub.days == (d0, d1) and sub.n_draws == got.n_draws
            for k in KEYS:
                assert np.array_equal(getattr(sub, k), want[k][d0:d1]), (d0, d1, k)


# 6. consistency with potus_posterior_summary on the same handle (save_warmup = 0: both pool the same rows)
@pytest.mark.parametrize("name", ["small_full", "2016"])
def test_consistent_with_posterior_summary(fitted, name):
    h = fitted[name]
    S = int(h.data["S"])
    ev = _ev_for(S)
    o = h.outcomes(ev)
    sm = h.posterior_summary(ev.astype(np.float64))
    n = o.n_draws
    assert n == h.opts.chains * h.draws_saved()
    diag = np.diagonal(o.joint, axis1=1, axis2=2)                                   # [T, S + 2]
    assert np.array_equal(diag[:, :S] / n, sm["state"][:, :, 3])
    k = np.arange(o.ev_hist.shape[1])
    mean = (o.ev_hist * k).sum(1) / n
    assert np.abs(mean - sm["electoral_votes"][:, 0]).max() <= 1e-12 * np.abs(sm["electoral_votes"][:, 0]).max()
    assert np.array_equal(o.ev_hist[:, 270:].sum(1) / n, sm["electoral_votes"][:, 4])
    assert np.array_equal(diag[:, S] / n, sm["electoral_votes"][:, 4])
    assert np.array_equal(diag[:, S + 1] / n, sm["national"][:, 3])
    assert (o.ev_hist.sum(1) == n).all() and (o.tipping.sum(1) == n).all()
    assert np.array_equal(o.joint, o.joint.transpose(0, 2, 1))
    assert np.array_equal(o.win_probability(), sm["electoral_votes"][:, 4])


def test_saved_warmup_rows_are_left_out(cases):
    data, variant = cases["small_full"]
    nw, ns = 60, 50
    h = _fit(data, variant, chains=2, nw=nw, ns=ns, seed=7, save_warmup=1)
    assert h.draws_saved() == nw + ns and h.post_warmup_saved() == ns
    S = int(data["S"])
    ps = _predicted_score(h, first=nw)
    w, ev = ref.normalised_weights(data["state_weights"]), _ev_for(S)
    want = ref.outcomes(ps, w, ev, 270)
    _assert_generic(ps, want["nat"])
    got = h.outcomes(ev)
    assert got.n_draws == 2 * ns
    _assert_equal(got, want)
    h.close()


# 7. pooled handles give the bytes of one handle; a repeated call gives the same bytes
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
    ev = _ev_for(int(data["S"]))
    actual = np.full(int(data["S"]), 0.5)
    r1, r2, r3 = oc.outcomes([one], ev, actual=actual), oc.outcomes([a, b], ev, actual=actual), oc.outcomes([one], ev, actual=actual)
    assert r1.n_draws == r2.n_draws == 4 * ns
    for k in KEYS:
        assert getattr(r1, k).tobytes() == getattr(r2, k).tobytes() == getattr(r3, k).tobytes(), k
    assert oc.outcomes([b, a], ev, actual=actual).joint.tobytes() == r1.joint.tobytes()      # counts do not depend on the order either
    for h in (one, a, b):
        h.close()


# 9. refusals: a status with a message, never a fault, and the handle stays usable
def test_refusals(fitted, cases):
    import torch
    h = fitted["small_full"]
    data, variant = cases["small_full"]
    S, T = int(data["S"]), int(data["T"])
    ev = _ev_for(S)
    before = h.outcomes(ev)
    g = _fit(cases["small_nomode"][0], "no_mode_adjustment", chains=2, nw=5, ns=5)
    with pytest.raises(PotusError, match="another posterior"):
        oc.outcomes([h, g], ev)
    with pytest.raises(PotusError, match="listed twice"):
        oc.outcomes([h, h], ev)
    e = Handle(data, variant, chains=2, num_warmup=5, num_samples=5)
    e.init()
    with pytest.raises(PotusError, match="error 4.*at least one saved post-warm-up draw"):
        oc.outcomes([e], ev)
    wu = Handle(data, variant, chains=2, num_warmup=20, num_samples=5, save_warmup=1)
    wu.init()
    wu.run(10)                                                                           # ten rows saved, all of them warm-up
    with pytest.raises(PotusError, match="error 4.*at least one saved post-warm-up draw"):
        oc.outcomes([wu], ev)
    m = Handle(data, variant, chains=2, num_warmup=5, num_samples=5, cus_per_chain=1, twin=0)
    ys, yn = np.asarray(data["n_democrat_state"])[None], np.asarray(data["n_democrat_national"])[None]
    m.set_datasets(np.repeat(ys, 2, 0), np.repeat(yn, 2, 0))
    m.init()
    m.run(10)
    with pytest.raises(PotusError, match="error 4.*slice the chains per data set"):
        oc.outcomes([m], ev)

    L = h.L
    ids = (C.c_int * 1)(h.h)

    def pooled(d0=0, d1=T, ev_=ev, W=270, actual=None):
        e32 = np.ascontiguousarray(ev_, dtype=np.int32)
        return L.potus_outcomes(ids, 1, d0, d1, e32.ctypes.data_as(I32), W, None if actual is None else actual.ctypes.data_as(DP),
                                None, None, None, None, None)

    def message():
        buf = C.create_string_buffer(512)
        L.potus_last_error(buf, 512)
        return buf.value.decode()
    for d0, d1 in ((-1, 3), (0, T + 1), (4, 4), (5, 2)):
        assert pooled(d0, d1) == 1 and "days" in message()
    neg = ev.copy()
    neg[2] = -1
    assert pooled(ev_=neg) == 1 and "negative" in message()
    big = ev.copy()
    big[0] += 2048 - 538
    assert pooled(ev_=big) == 6 and "2047" in message()
    assert pooled(W=0) == 1 and "ev_to_win" in message()
    bad = np.full(S, 0.5)
    bad[1] = 1.5
    assert pooled(actual=bad) == 1 and "outside [0, 1]" in message()
    assert pooled() == 0                                                                  # every output pointer may be null
    # a block that is not device memory of the device named
    host = np.full((4, 1, S), 0.5)
    w = ref.normalised_weights(data["state_weights"])
    e32 = np.ascontiguousarray(ev, dtype=np.int32)
    assert L.potus_outcomes_device(0, C.c_void_p(host.ctypes.data), 4, 1, S, w.ctypes.data_as(DP), e32.ctypes.data_as(I32), 270, None,
                                   None, None, None, None, None) == 1 and "not device memory" in message()
    assert L.potus_outcomes_device(99, C.c_void_p(host.ctypes.data), 4, 1, S, w.ctypes.data_as(DP), e32.ctypes.data_as(I32), 270, None,
                                   None, None, None, None, None) == 2 and "no HIP device" in message()
    if torch.cuda.device_count() >= 2:
        t = torch.full((4, 1, S), 0.5, dtype=torch.float64, device="cuda:1")
        assert L.potus_outcomes_device(0, C.c_void_p(t.data_ptr()), 4, 1, S, w.ctypes.data_as(DP), e32.ctypes.data_as(I32), 270, None,
                                       None, None, None, None, None) == 1 and "not device memory" in message()
    after = h.outcomes(ev)
    assert all(getattr(before, k) is None or getattr(before, k).tobytes() == getattr(after, k).tobytes() for k in KEYS)
    for x in (g, e, wu, m):
        x.close()


# 10. the .C() entry point gives the counts of potus_outcomes
def test_r_entry_point_gives_the_counts_of_potus_outcomes(fitted):
    h = fitted["small_full"]
    S, T = int(h.data["S"]), int(h.data["T"])
    ev = _ev_for(S)
    actual = np.linspace(0.3, 0.7, S)
    f = h.L.potus_R_outcomes
    for given, days in ((1, (0, T)), (0, (2, 5))):
        want = oc.outcomes([h], ev, actual=actual if given else None, days=days)
        n = days[1] - days[0]
        hist, tip, joint, below = np.zeros(n * 539), np.zeros(n * (S + 1)), np.zeros(n * (S + 2) ** 2), np.full(n * S, -1.0)
        nd, st = np.zeros(1), C.c_int(-1)
        e32 = np.ascontiguousarray(ev, dtype=np.int32)
        f((C.c_int * 1)(h.h), C.byref(C.c_int(1)), (C.c_int * 4)(days[0], days[1], 270, given), e32.ctypes.data_as(C.POINTER(C.c_int)),
          actual.ctypes.data_as(DP), hist.ctypes.data_as(DP), tip.ctypes.data_as(DP), joint.ctypes.data_as(DP), below.ctypes.data_as(DP),
          nd.ctypes.data_as(DP), C.byref(st))
        assert st.value == 0 and nd[0] == want.n_draws
        assert np.array_equal(hist, want.ev_hist.reshape(-1)) and np.array_equal(tip, want.tipping.reshape(-1))
        assert np.array_equal(joint, want.joint.reshape(-1))
        if given:
            assert np.array_equal(below, want.below_actual.reshape(-1))
        else:
            assert (below == -1.0).all()                                                  # left alone without `actual`
    st = C.c_int(-1)
    f((C.c_int * 1)(h.h), C.byref(C.c_int(1)), (C.c_int * 4)(3, 3, 270, 0), e32.ctypes.data_as(C.POINTER(C.c_int)), actual.ctypes.data_as(DP),
      hist.ctypes.data_as(DP), tip.ctypes.data_as(DP), joint.ctypes.data_as(DP), below.ctypes.data_as(DP), nd.ctypes.data_as(DP), C.byref(st))
    assert st.value == 1


# 11. p-values of the 2016 backtest against the certified result
def test_p_values_of_the_2016_backtest(fitted):
    """README.Rmd:1519-1540.  Every state of the design is compared, DC among them: the `filter(state != 'DC')` of README.Rmd:1645 belongs
    to the calibration plot, not to the computation."""
    h = fitted["2016"]
    meta = dataprep.load_npz(GOLD / "data_2016.npz")["meta"]
    states, ev = [str(s) for s in meta["states"]], np.asarray(meta["ev_state"], dtype=np.int64)
    assert ev.sum() == 538
    _, rows = readme_golden(2016)
    act = {r["state"]: float(r["actual"]) for r in rows if r["state"] != "--"}
    actual = np.array([act[s] for s in states])
    T = int(h.data["T"])
    o = oc.outcomes([h], ev, actual=actual, days=(T - 1, T), states=states)
    ps = _predicted_score(h)[:, -1:, :]
    want = ref.outcomes(ps, ref.normalised_weights(h.data["state_weights"]), ev, 270, actual)
    _assert_equal(o, want)
    n = o.n_draws
    assert np.array_equal(o.p_values(), ref.p_values(want["below_actual"][0], n))
    assert np.array_equal(o.p_values(), (2.0 * (ps[:, 0] < actual).sum(0) + 1.0) / (2.0 * n + 2.0))
    sm = h.posterior_summary(ev.astype(np.float64))
    out = o.outside_ci(sm)
    assert np.array_equal(out, (actual > sm["state"][T - 1, :, 1]) | (actual < sm["state"][T - 1, :, 0]))
    tp = o.tipping_point()
    assert tp and tp[0][0] in states and abs(sum(p for _, p in tp) - 1.0) < 1e-12
    print("2016, 4 x 40 draws: tipping point", tp[:5], "EV", o.ev_summary(), "split", o.popular_vote_split(),
          "outside the 95 % interval:", [s for s, x in zip(states, out) if x])
