"""CPU tests of the posterior predictive check: the numpy restatement (tests/ppc_ref.py) against a toy with an analytic predictive distribution,
the host side of us_potus_model_amd.ppc against the restatement, the refusals that need no device, and the names of the new entry points in
the header, the R shim and sampler.EXPORTS."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
from scipy import stats

import ppc_ref
from us_potus_model_amd import ppc, sampler, synthetic

ROOT = Path(__file__).resolve().parent.parent


def _toy(seed, weighted):
    """N polls of n trials under a beta posterior of the share: replicates by numpy, outcomes from the exact beta-binomial predictive distribution.
    weighted: the draws come from Beta(a0, b0), the importance weights turn it into Beta(a1, b1), the distribution the outcomes follow."""
    rng = np.random.default_rng(seed)
    N, S, n = 400, 4000, 40
    a1, b1 = 12.0, 9.0
    a0, b0 = (9.0, 8.0) if weighted else (a1, b1)
    p = rng.beta(a0, b0, size=(N, S))
    yrep = rng.binomial(n, p).astype(np.float64)
    y = stats.betabinom.rvs(n, a1, b1, size=N, random_state=rng).astype(np.float64)
    lw = None
    if weighted:
        lw = stats.beta.logpdf(p, a1, b1) - stats.beta.logpdf(p, a0, b0)
        lw -= np.log(np.exp(lw).sum(axis=1, keepdims=True))
    return n, a1, b1, yrep, y, lw


@pytest.mark.parametrize("weighted", [False, True])
def test_reference_pit_is_uniform_on_a_beta_binomial_toy(weighted):
    n, a, b, yrep, y, lw = _toy(11, weighted)
    lo, eq = ppc_ref.pit_sums(yrep, y, lw)
    # the sums estimate the analytic predictive CDF: 6 Monte-Carlo sd (effective sample size S / 3 at worst for these weights)
    S_eff = yrep.shape[1] if lw is None else 1.0 / np.exp(2.0 * lw).sum(axis=1).max()
    F0, F1 = stats.betabinom.cdf(y - 1, n, a, b), stats.betabinom.cdf(y, n, a, b)
    assert np.abs(lo - F0).max() < 6 * 0.5 / np.sqrt(S_eff) and np.abs(lo + eq - F1).max() < 6 * 0.5 / np.sqrt(S_eff)
    u = ppc_ref.randomised(lo, eq, seed=3)
    assert stats.kstest(u, "uniform").pvalue > 0.01
    h = ppc_ref.pit_hist(lo, eq, 10)
    assert abs(h.sum() - 1.0) < 1e-12 and np.abs(h - 0.1).max() < 5 * np.sqrt(0.09 / len(y))
    assert abs(ppc_ref.coverage(lo, eq, 0.5) - 0.5) < 5 * np.sqrt(0.25 / len(y))
    assert abs(ppc_ref.coverage(lo, eq, 0.95) - 0.95) < 5 * np.sqrt(0.05 / len(y))


def test_pit_sums_at_the_ends_of_the_support():
    rng = np.random.default_rng(5)
    n = 7
    yrep = rng.binomial(n, 0.4, size=(3, 500)).astype(np.float64)
    lw = rng.normal(size=(3, 500))
    lw -= np.log(np.exp(lw).sum(axis=1, keepdims=True))
    for w in (None, lw):
        lo, eq = ppc_ref.pit_sums(yrep, np.array([0.0, n, 3.0]), w)
        assert lo[0] == 0.0 and abs(lo[1] + eq[1] - 1.0) < 1e-12 and 0 < lo[2] < lo[2] + eq[2] < 1
    # a weight of -inf counts as 0, NaN weights give NaN
    lw2 = lw.copy()
    lw2[0, :10] = -np.inf
    lw2[1, 3] = np.nan
    lo, eq = ppc_ref.pit_sums(yrep, np.array([2.0, 2.0, 2.0]), lw2)
    w0 = np.exp(lw[0])
    assert lo[0] == pytest.approx((w0[10:] * (yrep[0, 10:] < 2)).sum(), rel=1e-13) and np.isnan(lo[1]) and np.isnan(eq[1]) and np.isfinite(lo[2])


def test_histogram_sums_to_one_with_degenerate_polls():
    """y below every replicate without a tie (lo = eq = 0), above every one (lo = 1), a NaN poll (n = 0): the mass stays 1 over the polls left."""
    lo, eq = np.array([0.0, 1.0, 0.25, np.nan, 0.0]), np.array([0.0, 0.0, 0.5, np.nan, 1.0])
    for bins in (1, 4, 10):
        h = ppc_ref.pit_hist(lo, eq, bins)
        assert abs(h.sum() - 1.0) < 1e-15 and (h >= 0).all()
        assert np.allclose(h, ppc.pit_hist(lo, eq, bins), rtol=0, atol=1e-15)
    h = ppc_ref.pit_hist(lo, eq, 4)
    # poll 0 in the first bin, poll 1 in the last, poll 2 over the two middle bins, poll 4 uniform
    assert np.allclose(h, np.array([1 + 0.25, 0.5 + 0.25, 0.5 + 0.25, 1 + 0.25]) / 4)
    assert ppc_ref.coverage(lo, eq, 0.5) == pytest.approx(ppc.pit_coverage(lo, eq, 0.5)) == pytest.approx((0 + 0 + 1 + 0.5) / 4)


def test_group_restatement_on_three_polls_by_hand():
    # two draws; polls 0 and 2 in group 1, poll 1 in group 0, a fourth poll with n = 0 and a fifth with label -1 are in no sum; group 2 unused
    n = np.array([100.0, 50.0, 10.0, 0.0, 20.0])
    y = np.array([55.0, 20.0, 10.0, 0.0, 3.0])
    a1 = np.array([[0.5, 0.6], [0.4, 0.4], [0.9, 1.0], [0.5, 0.5], [0.2, 0.2]])
    a2 = a1 * a1
    a2[0, 1] = 0.37                                             # draw 1 of poll 0: overdispersed, v = 100 * .24 + 9900 * .01 = 123
    yrep = np.array([[50.0, 66.0], [20.0, 25.0], [8.0, 10.0], [0.0, 0.0], [4.0, 4.0]])
    T, cnt = ppc_ref.group_sums(yrep, a1, a2, y, n, [1, 0, 1, 1, -1], 3)
    assert cnt.tolist() == [1, 2, 0]
    r00, r01 = (55 - 50) / 5.0, (55 - 60) / np.sqrt(123.0)      # poll 0 realised
    q00, q01 = 0.0, (66 - 60) / np.sqrt(123.0)                  # poll 0 replicated
    r20, q20 = (10 - 9) / np.sqrt(0.9), (8 - 9) / np.sqrt(0.9)  # poll 2, draw 0; draw 1 has v = 0: residual 0
    assert np.allclose(T[1, 0, 0], [r00 + r20, r01]) and np.allclose(T[1, 0, 1], [q00 + q20, q01])
    assert np.allclose(T[1, 1, 0], [r00 ** 2 + r20 ** 2, r01 ** 2]) and np.allclose(T[1, 1, 1], [q20 ** 2, q01 ** 2])
    assert T[1, 2].tolist() == [[65.0, 65.0], [58.0, 76.0]]
    v1 = np.sqrt(50 * 0.4 * 0.6)
    assert np.allclose(T[0, 0], [[0.0, 0.0], [0.0, 5 / v1]]) and T[0, 2].tolist() == [[20.0, 20.0], [20.0, 25.0]]
    tab = ppc_ref.group_table(T, cnt)
    # group 0 (one poll): draw 0 is an exact tie in all three statistics, draw 1 is above
    assert tab[0, :, 2:].tolist() == [[1, 1, 0, 0.75]] * 3
    assert tab[1, 0, 2:].tolist() == [1, 0, 1, 0.5] and tab[1, 2, 2:].tolist() == [1, 0, 1, 0.5] and tab[1, 1, 2:].tolist() == [1, 0, 1, 0.5]
    assert tab[1, 2, 0] == 65.0 and tab[1, 2, 1] == 67.0
    assert np.isnan(tab[2, :, [0, 1, 5]]).all() and (tab[2, :, 2:5] == 0).all()
    assert ppc_ref.near_ties(T).sum() == 0


def test_groupings_from_the_data_list():
    d = synthetic.small("full")
    g = ppc.groupings(d, "full")
    N, Ns = d["N_state_polls"] + d["N_national_polls"], d["N_state_polls"]
    assert list(g) == list(ppc.BY)
    assert (g["state"][0][Ns:] == d["S"]).all() and g["state"][1][-1] == "S" and len(g["state"][1]) == d["S"] + 1
    assert (g["state"][0][:Ns] == np.asarray(d["state"]) - 1).all()
    assert (g["month"][0] == np.concatenate([d["day_state"], d["day_national"]]) // 30).all() and len(g["month"][1]) == g["month"][0].max() + 1
    assert (g["pollster"][0] == np.concatenate([d["poll_state"], d["poll_national"]]) - 1).all() and len(g["pollster"][1]) == d["P"]
    assert (g["all"][0] == 0).all() and all(v[0].dtype == np.int32 and v[0].shape == (N,) for v in g.values())
    assert list(ppc.groupings(synthetic.small("no_mode_adjustment"), "no_mode_adjustment")) == ["pollster", "state", "month", "all"]
    with pytest.raises(ValueError, match="by ="):
        ppc.groupings(d, "full", ("pollster", "house"))


def test_flag_and_tables():
    out = np.zeros((3, 3, 6))
    out[:, :, 5] = [[0.5, 0.004, 0.5], [0.999, 0.5, 0.5], [0.001, 0.001, 0.001]]
    t = ppc._group_table(out, [8, 5, 4], ["a", "b", "c"])
    P = ppc.Ppc(np.zeros((2, 4)), np.zeros(2), {"pollster": t}, 100, True, 0, np.zeros(4), None, None)
    assert P.flag(0.01, 5) == [("pollster", "b", "bias", 0.999, 5), ("pollster", "a", "dispersion", 0.004, 8)]
    assert len(P.flag(0.01, 4)) == 5 and P.flag(0.001, 5) == []


def test_new_names_are_declared_exported_and_wrapped():
    new = {"potus_poll_rep_device", "potus_ppc_pit_device", "potus_ppc_groups_device", "potus_ppc", "potus_ppc_timing", "potus_R_ppc"}
    hdr = (ROOT / "include" / "potus_hmc.h").read_text()
    assert new <= set(re.findall(r"\b(potus_[A-Za-z_0-9]+)\s*\(", hdr))
    assert new <= set(sampler.EXPORTS)
    r = (ROOT / "R" / "potus_sampling.R").read_text()
    assert '"potus_R_ppc"' in r and "potus_ppc <- function" in r
    L = sampler.load_library()
    assert all(hasattr(L, nm) for nm in new)
    assert hasattr(sampler.Handle, "ppc") and hasattr(sampler.StanFit, "ppc") and hasattr(sampler.Handle, "poll_rep_device")


def test_refusals_that_need_no_device():
    L = sampler.load_library()
    buf = C.create_string_buffer(512)
    x, k = np.zeros(8), np.zeros(2)
    dp, i32 = x.ctypes.data_as(C.POINTER(C.c_double)), C.POINTER(C.c_int32)
    ids = (C.c_int * 1)(12345)
    lab, ng, cnt = np.zeros(2, np.int32), np.ones(1, np.int32), np.zeros(1, np.int64)
    llp = cnt.ctypes.data_as(C.POINTER(C.c_longlong))
    for args, msg in (((ids, 1, 1, 0, None, 0, None, None, dp, None, None), b"null output"),
                      ((ids, 1, 2, 0, None, 0, None, dp, dp, None, None), b"integrate = 2"),
                      ((ids, 1, 1, -1, None, 0, None, dp, dp, None, None), b"rep = -1"),
                      ((ids, 1, 1, 1024, None, 0, None, dp, dp, None, None), b"rep = 1024"),
                      ((ids, 1, 1, 0, None, 1, None, dp, dp, dp, llp), b"groupings"),
                      ((ids, 1, 1, 0, None, 0, None, dp, dp, None, None), b"bad handle")):
        assert L.potus_ppc(*args) != 0
        L.potus_last_error(buf, 512)
        assert msg in buf.value, buf.value
    # the stage entry points: sizes, flags and labels are checked before the device is opened
    v = C.c_void_p(x.ctypes.data)
    assert L.potus_ppc_pit_device(0, v, dp, None, 2, 1, 3, dp) != 0                       # fewer than four draws
    assert L.potus_ppc_pit_device(0, None, dp, None, 2, 1, 4, dp) != 0
    lab[1] = 1
    for flags, acc, out, labels in ((3, None, dp, lab), (1, None, dp, np.zeros(2, np.int32)), (2, v, None, np.zeros(2, np.int32)), (4, v, dp, np.zeros(2, np.int32))):
        assert L.potus_ppc_groups_device(0, v, v, v, dp, dp, labels.ctypes.data_as(i32), 1, 2, 1, 4, acc, flags, out, llp) != 0
        L.potus_last_error(buf, 512)
        assert b"potus_ppc_groups_device" in buf.value
    assert L.potus_ppc_timing(None) != 0
