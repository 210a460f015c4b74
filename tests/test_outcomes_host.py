"""CPU tests of the joint-outcomes layer: the restatement (tests/outcomes_ref.py) on cases worked by hand, its vectorised twin, the host-side
derivations of us_potus_model_amd/outcomes.py on built counts, the refusals that need no device, and the names of the new entry points in the
header, the R shim and sampler.EXPORTS."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import outcomes_ref as ref
from us_potus_model_amd import outcomes as oc, sampler

ROOT = Path(__file__).resolve().parent.parent
EV3, W3 = [3, 4, 5], [0.25, 0.25, 0.5]


def test_new_names_are_declared_exported_and_wrapped():
    new = {"potus_outcomes", "potus_outcomes_device", "potus_outcomes_timing", "potus_R_outcomes"}
    hdr = (ROOT / "include" / "potus_hmc.h").read_text()
    assert new <= set(re.findall(r"\b(potus_[A-Za-z_0-9]+)\s*\(", hdr))
    assert new <= set(sampler.EXPORTS)
    r = (ROOT / "R" / "potus_sampling.R").read_text()
    assert '"potus_R_outcomes"' in r and "potus_outcomes <- function" in r and "potus_tipping_point <- function" in r
    L = sampler.load_library()
    assert all(hasattr(L, nm) for nm in new)
    import us_potus_model_amd as pkg
    # (the package attribute `outcomes` stays the module; its function is re-exported as joint_outcomes)
    assert pkg.outcomes is oc and pkg.joint_outcomes is oc.outcomes and pkg.outcomes_of_block is oc.outcomes_of_block and pkg.Outcomes is oc.Outcomes
    assert hasattr(sampler.Handle, "outcomes") and hasattr(sampler.StanFit, "outcomes")
    # potus_set_datasets' list of pooled calls that refuse names the new one
    assert re.search(r"calls that pool all chains \([^)]*potus_outcomes[^)]*\) refuse", hdr.replace("\n *", ""))


# ---- the restatement, by eye
def test_popular_vote_loss_orders_ascending():
    # nat = 0.15 + 0.1375 + 0.2 = 0.4875: a loss.  Ascending: state 2 (5 votes), state 1 (9 >= 7) -> state 1.  dem_ev = 3 + 4 = 7: a win
    # of the electoral college without the popular vote
    assert ref.item([0.6, 0.55, 0.4], W3, EV3, 7) == (7, pytest.approx(0.4875), False, 1)


def test_popular_vote_win_orders_descending():
    # nat = 0.175 + 0.075 + 0.3 = 0.55: a win.  Descending: state 0 (3), state 2 (8 >= 7) -> state 2.  dem_ev = 3 + 5
    assert ref.item([0.7, 0.3, 0.6], W3, EV3, 7) == (8, pytest.approx(0.55), True, 2)


def test_tie_is_broken_by_index_in_both_orders():
    # ascending (nat = 0.4): state 2 (5), then the tied states 0 and 1 in index order: state 0 (8 >= 7)
    assert ref.item([0.6, 0.6, 0.2], W3, EV3, 7)[2:] == (False, 0)
    # descending (nat = 0.52): state 0 (3), state 1 (7 >= 7)
    assert ref.item([0.6, 0.6, 0.2], [0.4, 0.4, 0.2], EV3, 7)[2:] == (True, 1)


def test_no_tipping_point_when_the_votes_cannot_reach_the_bar():
    assert ref.item([0.7, 0.3, 0.6], W3, EV3, 13)[3] == 3
    assert ref.item([0.7, 0.3, 0.6], W3, EV3, 12)[3] == 1          # the last state of the descending order


def test_national_vote_of_exactly_one_half_is_not_a_win():
    dem, nat, pop, tip = ref.item([0.5, 0.5, 0.5], W3, EV3, 7)
    assert nat == 0.5 and pop is False and dem == 0 and tip == 1   # all tied, ascending branch: states 0, 1 in index order


def test_counts_of_a_small_block_by_eye():
    ps = np.array([[[0.6, 0.55, 0.4]], [[0.7, 0.3, 0.6]], [[0.5, 0.5, 0.5]]])     # the three draws above, one day
    r = ref.outcomes(ps, W3, EV3, 7, actual=[0.65, 0.5, 0.45])
    assert r["n_draws"] == 3
    assert r["ev_hist"][0].tolist() == [1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0]
    assert r["tipping"][0].tolist() == [0, 2, 1, 0]
    # indicators: state 0, 1, 2, electoral college, popular vote.  Draw 1: (1, 1, 0, 1, 0); draw 2: (1, 0, 1, 1, 1); draw 3: none
    assert r["joint"][0].tolist() == [[2, 1, 1, 2, 1], [1, 1, 0, 1, 0], [1, 0, 1, 1, 1], [2, 1, 1, 2, 1], [1, 0, 1, 1, 1]]
    assert r["below_actual"][0].tolist() == [2, 1, 1]
    assert ref.p_values(r["below_actual"][0], 3).tolist() == [5 / 8, 3 / 8, 3 / 8]


def _random_block(rng, nd, ndays, S, ties=True):
    ps = rng.integers(0, 1025, (nd, ndays, S)) / 1024.0
    if ties:
        ps[::3, :, 1] = ps[::3, :, 0]
        ps[1::5] = 0.5
    return ps


@pytest.mark.parametrize("S,W", [(3, 7), (7, 20), (7, 1000)])
def test_vectorised_restatement_equals_the_loop(S, W):
    rng = np.random.default_rng(S + W)
    ps = _random_block(rng, 40, 3, S)
    w = ref.normalised_weights(rng.integers(1, 9, S))
    ev = rng.integers(0, 9, S)
    act = rng.integers(0, 1025, S) / 1024.0
    a, b = ref.outcomes(ps, w, ev, W, act), ref.outcomes_vectorised(ps, w, ev, W, act)
    for k in ("ev_hist", "tipping", "joint", "below_actual"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["ev_hist"].sum(1) == 40).all() and (a["tipping"].sum(1) == 40).all()
    assert np.array_equal(a["joint"], a["joint"].transpose(0, 2, 1))


# ---- the derivations of outcomes.py, on built counts
def _built(actual=True):
    rng = np.random.default_rng(11)
    S = 5
    ps = _random_block(rng, 200, 2, S, ties=False)
    ps[:, :, 4] = 0.25                                               # state 4 is never won: conditioning on it is undefined
    w = ref.normalised_weights([1, 2, 3, 2, 1])
    ev = np.array([3, 10, 20, 7, 4])
    act = np.array([0.4, 0.5, 0.6, 0.1, 0.9]) if actual else None
    r = ref.outcomes(ps, w, ev, 23, act)
    o = oc.Outcomes(r["ev_hist"], r["tipping"], r["joint"], r["below_actual"], r["n_draws"], ev, 23, (0, 2), act, states=list("ABCDE"))
    return ps, w, ev, act, r, o


def test_derivations_on_built_counts():
    ps, w, ev, act, r, o = _built()
    n, S = 200, 5
    dem = ((ps[:, 1] > 0.5) * ev).sum(1)
    nat = (ps[:, 1] * w).sum(1)
    assert o.ev_distribution().tolist() == (np.bincount(dem, minlength=45) / n).tolist()
    s = o.ev_summary()
    assert s["mean"] == pytest.approx(dem.mean(), rel=1e-14) and s["prob"] == (dem >= 23).mean()
    for key, p in (("median", 0.5), ("low", 0.025), ("high", 0.975)):
        assert s[key] == pytest.approx(np.quantile(dem, p), rel=1e-12), key
    assert o.win_probability().tolist() == [(((ps[:, t] > 0.5) * ev).sum(1) >= 23).mean() for t in (0, 1)]
    a, b = o.popular_vote_split()
    assert a == ((nat > 0.5) & (dem < 23)).mean() and b == ((nat <= 0.5) & (dem >= 23)).mean()
    c = o.conditional("B")
    assert c.shape == (S + 2,) and c[1] == 1.0
    won_b = ps[:, 1, 1] > 0.5
    assert c[0] == ((ps[:, 1, 0] > 0.5) & won_b).sum() / won_b.sum() and c[S] == ((dem >= 23) & won_b).sum() / won_b.sum()
    assert np.isnan(o.conditional("E")).all() and np.isnan(o.conditional(4, day=0)).all()      # never true: NaN, not a division error
    assert o.conditional("ec")[S] == 1.0 and o.index("popular") == S + 1
    tp = o.tipping_point()
    assert [x[1] for x in tp] == sorted((x[1] for x in tp), reverse=True) and sum(x[1] for x in tp) == pytest.approx(1.0)
    assert {x[0] for x in tp} <= set("ABCDE") and tp[0][0] == "ABCDE"[int(np.argmax(r["tipping"][1, :S]))]
    assert o.tipping_point(day=0, states=[10, 11, 12, 13, 14])[0][0] in (10, 11, 12, 13, 14)


def test_p_values_and_outside_ci():
    ps, w, ev, act, r, o = _built()
    below = (ps[:, 1] < act).sum(0)
    assert o.p_values().tolist() == ((2 * below + 1) / (2 * 200 + 2)).tolist()
    assert o.p_values(day=0).tolist() == ((2 * (ps[:, 0] < act).sum(0) + 1) / 402).tolist()
    state = np.zeros((2, 5, 4))
    state[1, :, 0], state[1, :, 1] = [0.3, 0.5, 0.61, 0.0, 0.2], [0.5, 0.6, 0.7, 0.1, 0.8]      # low, high on the range's last day
    assert o.outside_ci(dict(state=state)).tolist() == [False, False, True, False, True]
    state[0, :, 0], state[0, :, 1] = 0.0, 1.0
    assert not o.outside_ci(dict(state=state), day=0).any()
    o2 = _built(actual=False)[5]
    with pytest.raises(ValueError, match="without `actual`"):
        o2.p_values()
    with pytest.raises(ValueError, match="without `actual`"):
        o2.outside_ci(dict(state=state))


# ---- refusals that need no device
def test_python_argument_refusals():
    with pytest.raises(ValueError, match="integers"):
        oc._integer_ev([3, 4.5, 5], 3)
    with pytest.raises(ValueError, match="negative"):
        oc._integer_ev([3, -4, 5], 3)
    with pytest.raises(ValueError, match="at most 2047"):
        oc._integer_ev([1000, 1000, 48], 3)
    with pytest.raises(ValueError, match="shape"):
        oc._integer_ev([3, 4], 3)
    assert oc._integer_ev([3.0, 4.0, 5.0], 3).dtype == np.int32 and oc._integer_ev([1000, 1000, 47], 3).sum() == 2047
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        oc._actual([0.5, 1.5, 0.2], 3)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        oc._actual([0.5, np.nan, 0.2], 3)
    import torch
    with pytest.raises(TypeError, match="on the GPU"):
        oc.outcomes_of_block(torch.zeros((4, 1, 3), dtype=torch.float64), W3, EV3)


def test_library_refuses_bad_arguments_before_touching_a_device():
    L = sampler.load_library()
    DP, I32, LL = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
    w = np.array(W3)
    act = np.array([0.5, 0.5, 0.5])
    fake = C.c_void_p(4096)                                          # never dereferenced: every call below is refused first

    def call(n_draws=10, n_days=1, S=3, ev=(3, 4, 5), W=7, actual=None, block=fake, weights=w):
        e = np.array(ev, dtype=np.int32)
        return L.potus_outcomes_device(0, block, n_draws, n_days, S, weights.ctypes.data_as(DP), e.ctypes.data_as(I32), W,
                                       None if actual is None else actual.ctypes.data_as(DP), None, None, None, None, None)

    def message():
        buf = C.create_string_buffer(512)
        L.potus_last_error(buf, 512)
        return buf.value.decode()
    assert call(ev=(3, -4, 5)) == 1 and "negative" in message()
    assert call(ev=(1000, 1000, 48)) == 6 and "2047" in message()
    assert call(W=0) == 1 and "ev_to_win" in message()
    assert call(actual=np.array([0.5, 1.25, 0.5])) == 1 and "outside [0, 1]" in message()
    assert call(actual=np.array([0.5, np.nan, 0.5])) == 1
    assert call(n_draws=0) == 1 and "at least one" in message()
    assert call(n_days=0) == 1
    assert call(S=64, ev=(1,) * 64, weights=np.ones(64)) == 6 and "lanes" in message()
    assert call(block=None) == 1
    assert call(weights=np.array([0.5, np.inf, 0.5])) == 1 and "finite" in message()
    ids = (C.c_int * 1)(-7)
    e = np.array(EV3, dtype=np.int32)
    assert L.potus_outcomes(ids, 1, 0, 1, e.ctypes.data_as(I32), 7, act.ctypes.data_as(DP), None, None, None, None, None) == 4
    assert "bad handle" in message()
    assert L.potus_outcomes(None, 0, 0, 1, e.ctypes.data_as(I32), 7, None, None, None, None, None, None) == 1
    assert L.potus_outcomes_timing(None) == 1
