"""Exact cross-validation on the MI355X (potus_crossval.hpp): k_cv_loglik against potus_log_lik_device (bytes), scipy and quadrature,
k_cv_reduce against logsumexp, blocking, a failed chain, refusals, the .C() path, exact leave-one-out in one launch against PSIS-LOO, and
crossval.kfold / Timeline.lfo end to end.  The fixture is the four-data-set design of tests/test_gpu_timeline.py."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import stats
from scipy.special import expit, logsumexp

import psis_ref
from test_gpu_timeline import CPD, N_DS, NS, NW, OPTS, fit, small_design
from us_potus_model_amd import _abi, crossval, loo as loo_mod, synthetic, timeline
from us_potus_model_amd.sampler import Handle, PotusError

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ND = CPD * NS                                      # 100 draws per data set: not a multiple of 64
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def held_of(design):
    """Data set 0: everything (in-sample); 1: the polls it dropped; 2: all polls (it saw none); 3: nothing."""
    ks, kn = design["keep_state"], design["keep_national"]
    hs = np.stack([np.ones_like(ks[0]), ~ks[1], np.ones_like(ks[0]), np.zeros_like(ks[0])])
    hn = np.stack([np.ones_like(kn[0]), ~kn[1], np.ones_like(kn[0]), np.zeros_like(kn[0])])
    return hs, hn


def polls_of(data):
    """(y, n, sigma) per poll: state polls, then national polls."""
    y, n = (a.astype(float) for a in loo_mod.poll_vectors(data))
    Ns, Nn = int(data["N_state_polls"]), int(data["N_national_polls"])
    sig = np.concatenate([np.full(Ns, float(data["sigma_measure_noise_state"])), np.full(Nn, float(data["sigma_measure_noise_national"]))])
    return y, n, sig


def canonical(h, *names):
    """[data set][column][draw of the data set, chain after chain] of the named output blocks, from write_array."""
    x = np.concatenate([h.write_array(h.layout[k][0], h.layout[k][1], NS) for k in names], axis=2)       # [iteration, chain, column]
    return x.reshape(NS, N_DS, CPD, -1).transpose(1, 3, 2, 0).reshape(N_DS, x.shape[2], ND)


@pytest.fixture(scope="module")
def cv():
    design = small_design()
    h = fit(design, CPD, NW, NS)
    hs, hn = held_of(design)
    held = np.concatenate([hs, hn], axis=1)
    pairs = [(d, k) for d in range(N_DS) for k in np.flatnonzero(held[d])]
    ll = {g: h.cv_log_lik_device(hs, hn, integrate=g).cpu().numpy() for g in (False, True)}
    lpd, cnt = h.cv_lpd(hs, hn, True)
    logit_pi = canonical(h, "logit_pi_democrat_state", "logit_pi_democrat_national")
    noise = canonical(h, "raw_measure_noise_state", "raw_measure_noise_national")
    for a in (ll[False], ll[True], lpd, logit_pi, noise):
        a.setflags(write=False)
    yield dict(h=h, design=design, hs=hs, hn=hn, held=held, pairs=pairs, ll=ll, lpd=lpd, cnt=cnt, logit_pi=logit_pi, noise=noise)
    h.close()


def test_in_sample_values_are_the_bytes_of_log_lik_device(cv):
    import torch
    design, Np = cv["design"], cv["h"].n_polls
    assert cv["h"].chain_status()[0] == [0] * (N_DS * CPD)
    assert [p for p in cv["pairs"] if p[0] == 0] == [(0, k) for k in range(Np)] and cv["ll"][True].shape == (len(cv["pairs"]), ND)
    g = Handle(timeline.data_of(design, 0), "full", chains=CPD, num_warmup=NW, num_samples=NS, chain_id_offset=0, **OPTS)
    g.init()
    g.run(NW + NS)
    for integrate in (False, True):
        t = torch.empty((Np, CPD, NS), dtype=torch.float64, device="cuda:0")
        g.log_lik_device(0, Np, t, integrate=integrate)
        want = t.cpu().numpy().reshape(Np, ND)
        got = cv["ll"][integrate][:Np]
        print(f"integrate={integrate}: max |cv - log_lik_device| = {np.abs(got - want).max():.3e}")
        assert np.ascontiguousarray(got).tobytes() == want.tobytes()
        # a plain handle counts as one data set
        one = g.cv_log_lik_device(np.ones((1, cv["hs"].shape[1])), np.ones((1, cv["hn"].shape[1])), integrate=integrate).cpu().numpy()
        assert one.tobytes() == want.tobytes()
    lpd1, cnt1 = g.cv_lpd(np.ones((1, cv["hs"].shape[1])), np.ones((1, cv["hn"].shape[1])), True)
    assert cnt1.tolist() == [ND] and lpd1[0].tobytes() == np.ascontiguousarray(cv["lpd"][0]).tobytes()
    g.close()


def test_plain_values_equal_scipy_on_the_logit_pi_columns(cv):
    y, n, _ = polls_of(cv["design"]["data"])
    worst = 0.0
    for j, (d, k) in enumerate(cv["pairs"]):
        if d in (1, 2):
            ref = stats.binom.logpmf(y[k], n[k], expit(cv["logit_pi"][d, k]))   # the real y and n: the data set's own are 0
            worst = max(worst, np.abs(cv["ll"][False][j] - ref).max())
    assert sum(d == 1 for d, _ in cv["pairs"]) > 0
    print(f"largest |device - scipy| over the pairs of data sets 1 and 2: {worst:.2e}")
    assert worst < 1e-9


def test_integrated_values_equal_quadrature(cv):
    y, n, sig = polls_of(cv["design"]["data"])
    Ns = int(cv["design"]["data"]["N_state_polls"])
    eta = cv["logit_pi"] - sig[None, :, None] * cv["noise"]
    rng = np.random.default_rng(1)
    pairs = cv["pairs"]
    sample = set(rng.integers(0, len(pairs), 60).tolist())
    for d in range(3):
        mine = [j for j, (dd, _) in enumerate(pairs) if dd == d]
        sample |= {mine[0], mine[-1]}                                           # the first and last pair of each data set
        sample |= {j for j in mine if pairs[j][1] >= Ns}                        # every national poll
        sample |= {j for j in mine if pairs[j][1] == int(np.argmax(n))}         # the poll with the largest n
    worst = 0.0
    for j in sorted(sample):
        d, k = pairs[j]
        i = int(rng.integers(0, ND))
        worst = max(worst, abs(cv["ll"][True][j, i] - psis_ref.log_lik_quad(y[k], n[k], eta[d, k, i], sig[k])))
    print(f"largest |device - quad| over {len(sample)} (pair, draw) cells: {worst:.2e}")
    assert worst < 1e-9


def test_integrated_value_of_a_held_out_outlier_poll_with_a_large_sample():
    """One more fold: a state poll of synthetic.small edited to 38 800 of 40 000 (97 %, about 3.5 logits from its state) and held out by the data
    set that is scored on it.  sigma^2 n = 64 and a mismatch beyond 2.2 logits is where undamped Newton steps from 0 oscillate: before the
    bracketed mode search of loo_poll_ll this "exact predictive density" of exactly the poll cross-validation exists to flag was off by orders.
    Every draw of the pair against quadrature (psis_ref.log_lik_quad: brentq for the mode) on the row's own logit_pi column."""
    data = dict(synthetic.small("full"))
    k = 11
    n2, nd = np.array(data["n_two_share_state"]), np.array(data["n_democrat_state"])
    n2[k], nd[k] = 40_000, 38_800
    data["n_two_share_state"], data["n_democrat_state"] = n2, nd
    Ns, Nn = int(data["N_state_polls"]), int(data["N_national_polls"])
    keep_s, keep_n = np.ones((2, Ns), bool), np.ones((2, Nn), bool)
    keep_s[1, k] = False
    design = timeline.design_of(data, keep_s, keep_n, np.tile(np.asarray(data["mu_b_prior"], float), (2, 1)), np.full(2, data["mu_b_T_scale"]))
    h = Handle(design["data"], "full", chains=2 * CPD, num_warmup=NW, num_samples=NS, **OPTS)
    timeline.set_design(h, design)
    h.init()
    h.run(NW + NS)
    assert h.chain_status()[0] == [0] * (2 * CPD)
    ll = h.cv_log_lik_device(~keep_s, ~keep_n, integrate=True).cpu().numpy()
    assert ll.shape == (1, ND)
    lay = h.layout
    x = np.concatenate([h.write_array(lay[c][0] + k, lay[c][0] + k + 1, NS) for c in ("logit_pi_democrat_state", "raw_measure_noise_state")], axis=2)
    x = x[:, CPD:].transpose(1, 0, 2).reshape(ND, 2)                    # the draws of data set 1, chain after chain
    sig = float(data["sigma_measure_noise_state"])
    eta = x[:, 0] - sig * x[:, 1]
    mismatch = eta - np.log(38_800 / 1_200)
    assert np.abs(mismatch).min() > 2.5, mismatch                       # every draw is in the regime in question
    worst = max(abs(ll[0, i] - psis_ref.log_lik_quad(38_800, 40_000, eta[i], sig)) for i in range(ND))
    print(f"held-out outlier poll: eta - logit(y / n) in [{mismatch.min():.2f}, {mismatch.max():.2f}]; largest |device - quad| over {ND} draws: {worst:.2e}")
    assert worst < 1e-9
    h.close()


_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np, torch
torch.cuda.init()
from test_gpu_timeline import CPD, NS, NW, fit, small_design
from test_gpu_crossval import held_of
design = small_design()
h = fit(design, CPD, NW, NS)
hs, hn = held_of(design)
lpd, cnt = h.cv_lpd(hs, hn, True)
np.save({out!r}, lpd)
h.close()
"""


def test_reduce_equals_logsumexp_repeats_bytes_and_ignores_the_blocking(cv, tmp_path):
    h, lpd, held = cv["h"], cv["lpd"], cv["held"]
    assert cv["cnt"].tolist() == [ND] * N_DS and lpd.shape == (N_DS, h.n_polls, 2)
    assert np.isnan(lpd[~held]).all() and np.isfinite(lpd[held]).all()
    blk = cv["ll"][True]
    got = np.array([lpd[d, k] for d, k in cv["pairs"]])
    err0 = np.abs(got[:, 0] - (logsumexp(blk, axis=1) - np.log(ND))).max()
    err1 = np.abs(got[:, 1] - (logsumexp(2.0 * blk, axis=1) - np.log(ND))).max()
    print(f"max |lpd - logsumexp|: {err0:.2e}, second slot {err1:.2e}")
    assert err0 < 1e-12 and err1 < 1e-12
    ms = h.cv_timing()
    again, _ = h.cv_lpd(cv["hs"], cv["hn"], True)
    assert again.tobytes() == lpd.tobytes()
    assert ms["loglik_ms"] > 0 and ms["reduce_ms"] > 0
    assert h.cv_log_lik_device(cv["hs"], cv["hn"], True).cpu().numpy().tobytes() == blk.tobytes()
    # 30 pairs per block: data set 2's 95 pairs fall into at least three blocks.  The library reads the variable in the child's environment.
    out = tmp_path / "lpd.npy"
    code = _CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), out=str(out))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=str(ROOT),
                       env=dict(os.environ, POTUS_CV_BLOCK_BUDGET=str(30 * ND * 8)))
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.load(out).tobytes() == lpd.tobytes()


def test_a_failed_chain_fails_its_data_set_alone(cv):
    design = cv["design"]
    D = _abi.num_params(design["data"], "full")
    q0 = 0.1 * np.random.default_rng(11).standard_normal((N_DS * CPD, D))
    good = fit(design, CPD, 40, 20, q0)
    want, _ = good.cv_lpd(cv["hs"], cv["hn"], True)
    good.close()
    bad_q0 = q0.copy()
    bad_q0[5] = 1e308                                                           # a non-finite log density: an error status of chain 5, data set 2
    bad = fit(design, CPD, 40, 20, bad_q0)
    status = bad.chain_status()[0]
    assert status[5] != 0 and [s for c, s in enumerate(status) if c != 5] == [0] * 7
    got, cnt = bad.cv_lpd(cv["hs"], cv["hn"], True)
    assert cnt.tolist() == [40, 40, 0, 40]
    assert np.isnan(got[2]).all()
    keep = [0, 1, 3]
    assert got[keep].tobytes() == want[keep].tobytes() and np.isfinite(got[0]).all()
    blk = bad.cv_log_lik_device(cv["hs"], cv["hn"], True).cpu().numpy()
    ds = np.array([d for d, _ in cv["pairs"]])
    assert np.isnan(blk[ds == 2]).all() and np.isfinite(blk[ds != 2]).all()
    bad.close()


def test_refusals_and_the_empty_case(cv):
    h, hs, hn = cv["h"], cv["hs"], cv["hn"]
    L = h.L
    n, ms, mn = h._cv_masks(hs, hn)
    lpd, cnt = np.zeros((N_DS, h.n_polls, 2)), np.zeros(N_DS, np.int32)
    args = (ms.ctypes.data_as(IP), mn.ctypes.data_as(IP))
    out = (lpd.ctypes.data_as(DP), cnt.ctypes.data_as(IP))
    assert L.potus_cv_lpd(h.h, None, args[1], 1, *out) == 1 and L.potus_cv_lpd(h.h, args[0], None, 1, *out) == 1
    assert L.potus_cv_lpd(h.h, *args, 1, None, out[1]) == 1 and L.potus_cv_lpd(h.h, *args, 1, out[0], None) == 1
    assert L.potus_cv_lpd(h.h, *args, 2, *out) == 1
    assert L.potus_cv_log_lik_device(h.h, *args, 1, None, None) == 1
    assert L.potus_cv_log_lik_device(h.h, None, None, 1, None, C.byref(C.c_longlong())) == 1
    assert not lpd.any()                                                        # no refusal wrote anything
    np_ = C.c_longlong(-1)
    assert L.potus_cv_log_lik_device(h.h, *args, 1, None, C.byref(np_)) == 0 and np_.value == len(cv["pairs"])
    data = cv["design"]["data"]
    one_s, one_n = np.ones((1, hs.shape[1])), np.ones((1, hn.shape[1]))
    e = Handle(data, "full", chains=2, num_warmup=5, num_samples=5, cus_per_chain=1, twin=0)
    with pytest.raises(PotusError, match="error 4.*not initialised"):
        e.cv_lpd(one_s, one_n)
    e.init()
    with pytest.raises(PotusError, match="error 4.*no post-warm-up draws"):
        e.cv_lpd(one_s, one_n)
    e.close()
    w = Handle(data, "full", chains=2, num_warmup=5, num_samples=5, save_warmup=1, cus_per_chain=1, twin=0)
    w.init()
    w.run(5)                                                                    # warm-up rows only
    with pytest.raises(PotusError, match="error 4.*no post-warm-up draws"):
        w.cv_lpd(one_s, one_n)
    w.run(5)
    assert w.cv_log_lik_device(one_s, one_n).shape == (h.n_polls, 2 * 5)        # ... and they are left out once there are draws
    w.close()
    dn = Handle(data, "full", chains=2, num_warmup=5, num_samples=5, metric=_abi.METRIC_DENSE)
    with pytest.raises(PotusError, match="error 6.*dense"):
        dn.cv_lpd(one_s, one_n)
    dn.close()
    with pytest.raises(ValueError, match="data sets"):
        h.cv_lpd(one_s, one_n)
    # all-zero masks: no error, no pair, every cell NaN
    got, cnt = h.cv_lpd(np.zeros_like(hs), np.zeros_like(hn))
    assert np.isnan(got).all() and got.shape == (N_DS, h.n_polls, 2) and cnt.tolist() == [ND] * N_DS
    assert tuple(h.cv_log_lik_device(np.zeros_like(hs), np.zeros_like(hn)).shape) == (0, ND)


def test_r_entry_point_gives_the_bytes_of_potus_cv_lpd(cv):
    h = cv["h"]
    _, ms, mn = h._cv_masks(cv["hs"], cv["hn"])
    lpd, cnt, st = np.zeros((N_DS, h.n_polls, 2)), np.zeros(N_DS, np.int32), C.c_int(-1)
    ip = C.POINTER(C.c_int)
    h.L.potus_R_cv_lpd(C.byref(C.c_int(h.h)), ms.ctypes.data_as(ip), mn.ctypes.data_as(ip), C.byref(C.c_int(1)), lpd.ctypes.data_as(DP),
                       cnt.ctypes.data_as(ip), C.byref(st))
    assert st.value == 0 and lpd.tobytes() == cv["lpd"].tobytes() and cnt.tolist() == cv["cnt"].tolist()


def test_exact_loo_in_one_launch_agrees_with_psis_loo():
    """Exact leave-one-out of 6 state polls and 2 national polls -- 8 single-poll folds in one launch -- against PSIS-LOO of the full fit,
    under the tolerance of test_gpu_loo.test_exact_loo_by_refitting_agrees: 4 sqrt(var_exact + var_psis), required below 0.1.
    The polls are picked from the PSIS-LOO of the 4-chain, 300 + 500 fit of tests/test_gpu_loo.py.  Measured with 4 chains x 500 draws on
    both sides, all 8 polls agreed (largest |difference| 0.035) but the tolerance of state poll 67 was 0.160, above the cap; so both sides
    are compared on 24 chains x 500 draws (the chains run side by side, the wall time stays), the polls unchanged."""
    import torch
    NW7, NS7, SEED, CH = 300, 500, 4242, 24
    data = synthetic.small("full")
    Ns, Nn = int(data["N_state_polls"]), int(data["N_national_polls"])

    def full_fit(chains):
        h = Handle(data, "full", chains=chains, num_warmup=NW7, num_samples=NS7, seed=SEED, cus_per_chain=1, twin=0)
        h.init()
        h.run(NW7 + NS7)
        return h
    h = full_fit(4)
    k4 = loo_mod.loo([h], integrate=True).pareto_k
    h.close()
    rng = np.random.default_rng(8)                                              # the choice is fixed before any result is looked at
    picks = list(rng.choice([i for i in range(Ns) if k4[i] < 0.5], 6, replace=False)) + \
        list(rng.choice([i for i in range(Ns, Ns + Nn) if k4[i] < 0.5], 2, replace=False))
    h = full_fit(CH)
    r = loo_mod.loo([h], integrate=True)
    ll = torch.empty((h.n_polls, CH, NS7), dtype=torch.float64, device="cuda:0")
    h.log_lik_device(0, h.n_polls, ll, integrate=True)
    ll = ll.cpu().numpy()
    h.close()
    held = np.zeros((8, Ns + Nn), bool)
    held[np.arange(8), picks] = True
    tl = timeline.fit(timeline.design_of(data, ~held[:, :Ns], ~held[:, Ns:]), "full", chains_per_date=CH, num_warmup=NW7, num_samples=NS7, seed=SEED)
    assert tl.handle.chain_status()[0] == [0] * (8 * CH)
    blk = tl.handle.cv_log_lik_device(held[:, :Ns], held[:, Ns:], True).cpu().numpy()      # [8, draws]: fold j's pair is poll picks[j]
    lpd, cnt = tl.handle.cv_lpd(held[:, :Ns], held[:, Ns:], True)
    tl.close()
    assert cnt.tolist() == [CH * NS7] * 8 and blk.shape == (8, CH * NS7)
    worst_tol = 0.0
    fails = []
    for j, i in enumerate(picks):
        l = blk[j].reshape(CH, NS7)
        exact = lpd[j, i, 0]
        assert abs(exact - (logsumexp(l) - np.log(l.size))) < 1e-12
        w = np.exp(l - l.max())
        var_exact = w.var() / (w.mean() ** 2 * l.size * psis_ref.relative_eff(l))          # delta method
        lw, _ = psis_ref.psis(ll[i], r.r_eff[i])
        p = np.exp(ll[i].reshape(-1) - ll[i].max())
        W = np.exp(lw)
        E = (W * p).sum()
        var_psis = (W * W * (p / E - 1) ** 2).sum() / r.r_eff[i]
        tol = 4 * np.sqrt(var_exact + var_psis)
        worst_tol = max(worst_tol, tol)
        print(f"poll {i} ({'national' if i >= Ns else 'state'}): exact {exact:.4f}, PSIS {r.pointwise[i, 0]:.4f}, k {r.pareto_k[i]:.2f} (4 chains: {k4[i]:.2f}), "
              f"difference {exact - r.pointwise[i, 0]:+.4f}, tolerance {tol:.4f}")
        if not abs(exact - r.pointwise[i, 0]) < tol:
            fails.append(int(i))
    assert worst_tol < 0.1
    assert not fails, fails


def test_kfold_end_to_end_and_lfo(cv):
    data = cv["design"]["data"]
    kf = crossval.kfold(data, "full", K=3, by="pollster", chains_per_fold=2, num_warmup=NW, num_samples=NS, seed=1843)
    N = cv["h"].n_polls
    assert kf.elpd.shape == kf.mcse.shape == kf.fold.shape == (N,) and np.isfinite(kf.elpd).all() and np.isfinite(kf.mcse).all() and (kf.mcse > 0).all()
    assert np.array_equal(kf.fold, crossval.folds(data, 3, "pollster")) and kf.n_draws.tolist() == [2 * NS] * 3
    assert kf.rhat_max.shape == kf.ess_bulk_min.shape == (3,) and np.isfinite(kf.rhat_max).all()
    assert kf.elpd_kfold == kf.elpd.sum() and kf.se > 0 and kf.timing["loglik_ms"] > 0
    print(kf, "per fold:", [round(float(kf.elpd[kf.fold == d].sum()), 2) for d in range(3)])
    rows = loo_mod.loo_compare(kf.as_loo(), kf.as_loo())
    assert rows[1]["elpd_diff"] == 0.0 and rows[1]["se_diff"] == 0.0
    # leave-future-out on the fixture: date 2 saw no poll and date 3 keeps them all, so date 2 is scored on every poll
    t = timeline.Timeline(cv["h"], cv["design"], CPD)
    out = t.lfo()
    hs, hn = timeline.lfo_masks(cv["design"])
    by_hand, cnt = cv["h"].cv_lpd(hs, hn, True)
    assert out["lpd"].tobytes() == by_hand.tobytes() and out["n_draws"].tolist() == cnt.tolist()
    assert out["n_held"].tolist() == [0, 0, N, 0] and out["elpd"][[0, 1, 3]].tolist() == [0.0, 0.0, 0.0]
    assert out["elpd"][2] == by_hand[2, :, 0].sum() and np.isfinite(out["elpd"][2])
    assert np.ascontiguousarray(by_hand[2]).tobytes() == np.ascontiguousarray(cv["lpd"][2]).tobytes()   # the same pairs as the fixture's data set 2
