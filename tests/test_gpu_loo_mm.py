"""Moment matching for PSIS-LOO on the MI355X (potus_loo_mm.hpp): every stage against its reference -- the pass under
an affine map against the CPU oracle, the weighted moments against math.fsum, PSIS of general ratios against tests/loo_mm_ref.py -- and
the whole call against the numpy restatement run on the device's own draws, decision by decision; then what the call promises about
bytes, its refusals and the .C() path."""
import ctypes as C
import math

import numpy as np
import pytest

import loo_mm_ref as ref
import psis_ref
from oracle_lib import OracleModel
from us_potus_model_amd import loo as loo_mod, synthetic
from us_potus_model_amd.sampler import Handle, PotusError

pytestmark = pytest.mark.gpu
SEED = 4242
NW, NS = 300, 500
VARIANTS = ("full", "no_mode_adjustment")
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
SHIFT = 1.5          # logits the planted outlier is moved from where the design put it
PLAIN_POLLS = (38, 74, 18)   # plain-form polls of the 3-chain fit with k-hat > 0.7, an accepted T2 step each (74: two more rounds, rejected), reference margins 0.14, 0.03, 0.30


def outlier_data(variant):
    """synthetic.small with the state poll of the largest n moved SHIFT logits: a poll no draw predicts, in the integrated form too."""
    data = dict(synthetic.small(variant))
    n, y = np.asarray(data["n_two_share_state"]), np.asarray(data["n_democrat_state"]).copy()
    i = int(np.argmax(n))
    p = y[i] / n[i]
    y[i] = int(round(n[i] / (1.0 + np.exp(-(np.log(p / (1.0 - p)) + SHIFT)))))
    data["n_democrat_state"] = y
    return data, i


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def _fit(data, variant, chains=4, ns=NS, **kw):
    kw.setdefault("cus_per_chain", 1)
    kw.setdefault("twin", 0)
    h = Handle(data, variant, chains=chains, num_warmup=NW, num_samples=ns, seed=SEED, **kw)
    h.init()
    h.run(NW + ns)
    return h


@pytest.fixture(scope="module")
def fits():
    out = {v: _fit(outlier_data(v)[0], v) for v in VARIANTS}
    out["three"] = _fit(outlier_data("full")[0], "full", chains=3, ns=167)
    yield out
    for h in out.values():
        h.close()


@pytest.fixture(scope="module")
def loos(fits):
    return {(k, integ): loo_mod.loo([h], integrate=integ) for k, h in fits.items() for integ in (False, True)}


def _block(h):
    """the post-warm-up draws [chains][n][7 + D] on the GPU"""
    import torch
    return torch.tensor(np.ascontiguousarray(h.draws()[:, -h.post_warmup_saved():, :]), device=f"cuda:{h.opts.device}")


class Oracle:
    """log_prob and one poll's log-likelihood at unconstrained points, on the CPU oracle"""

    def __init__(self, h):
        self.m, self.data, self.lay = OracleModel(h.data, h.variant), h.data, h.layout
        self.Ns = int(h.data["N_state_polls"])
        self.y, self.n = (a.astype(float) for a in loo_mod.poll_vectors(h.data))

    def log_prob(self, th):
        return np.array([self.m.log_prob_grad(q)[0] for q in np.atleast_2d(th)])

    def log_lik(self, k, integrate):
        nat = k >= self.Ns
        j = k - self.Ns if nat else k
        c = self.lay["logit_pi_democrat_national" if nat else "logit_pi_democrat_state"][0] - 7 + j
        z = self.lay["raw_measure_noise_national" if nat else "raw_measure_noise_state"][0] - 7 + j
        sig = float(self.data["sigma_measure_noise_national" if nat else "sigma_measure_noise_state"])

        def f(th):
            th = np.atleast_2d(th)
            with np.errstate(all="ignore"):
                lpi = np.array([self.m.write_array(q)[c] for q in th])
                if integrate:
                    return psis_ref.log_lik_integrated(self.y[k], self.n[k], lpi - sig * th[:, z], sig)
                return psis_ref.log_lik_plain(self.y[k], self.n[k], lpi)
        return f


def _ratios(h, blk, a, b, polls, sel, integrate, lp0=True):
    import torch
    Cn, n = blk.shape[0], blk.shape[1]
    B = len(polls)
    lp, ll = (torch.full((B, Cn, n), float("nan"), dtype=torch.float64, device=blk.device) for _ in range(2))
    l0 = torch.full((Cn, n), float("nan"), dtype=torch.float64, device=blk.device)
    a, b = (np.ascontiguousarray(x, dtype=np.float64).reshape(B, h.D) for x in (a, b))
    pl, sl = (np.ascontiguousarray(x, dtype=np.int32) for x in (polls, sel))
    rc = h.L.potus_loo_mm_ratios_device(h.h, C.c_void_p(blk.data_ptr()), Cn, n, a.ctypes.data_as(DP), b.ctypes.data_as(DP), pl.ctypes.data_as(IP),
                                        sl.ctypes.data_as(IP), B, int(integrate), C.c_void_p(lp.data_ptr()), C.c_void_p(ll.data_ptr()),
                                        C.c_void_p(l0.data_ptr()) if lp0 else None)
    assert rc == 0, rc
    return lp.cpu().numpy(), ll.cpu().numpy(), l0.cpu().numpy()


def test_the_planted_outlier_has_a_high_k_on_the_oracle_s_own_chain():
    """Before the device is relied on: the CPU oracle's chain on the edited data gives the outlier k-hat > 0.7 in both forms."""
    data, i = outlier_data("full")
    m = OracleModel(data, "full")
    d, _, _ = m.sample_chain(1, m.default_opts(num_warmup=NW, num_samples=NS, seed=SEED, fast_grad=0, save_warmup=0))
    h = type("H", (), dict(data=data, variant="full", layout=__import__("us_potus_model_amd")._abi.column_layout(data, "full")[0]))
    orc = Oracle(h)
    for integrate in (True, False):
        l = orc.log_lik(i, integrate)(d[:, 7:])
        _, k = psis_ref.psis(l, psis_ref.relative_eff(l[None, :]))
        assert k > 0.7, (integrate, k)


@pytest.mark.parametrize("integrate", [False, True])
def test_identity_map_gives_zero_and_the_bytes_of_log_lik(fits, integrate):
    import torch
    h = fits["three"]
    blk = _block(h)
    polls = list(range(h.n_polls))
    lp, ll, lp0 = _ratios(h, blk, np.zeros((len(polls), h.D)), np.ones((len(polls), h.D)), polls, [0] * len(polls), integrate)
    assert np.isfinite(lp0).all() and np.all(lp - lp0[None] == 0.0)
    lp1, ll1, _ = _ratios(h, blk, np.zeros((len(polls), h.D)), np.ones((len(polls), h.D)), polls, [1] * len(polls), integrate)   # T with a = 0, b = 1
    assert np.all(lp1 - lp0[None] == 0.0) and ll1.tobytes() == ll.tobytes()
    t = torch.empty((h.n_polls, h.opts.chains, h.post_warmup_saved()), dtype=torch.float64, device=blk.device)
    h.log_lik_device(0, h.n_polls, t, integrate=integrate)
    assert ll.tobytes() == t.cpu().numpy().tobytes()
    # lp0 is the model pass's log density: the draws' own lp__ to the rounding of a separate evaluation
    assert np.allclose(lp0, h.draws()[:, -h.post_warmup_saved():, 0], rtol=1e-11, atol=0)


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_pass_under_a_map_agrees_with_the_oracle(fits, variant):
    """lp to 1e-11 |lp| (test_gpu_parity.py), the poll terms to 1e-9 (test_gpu_loo.py), at T theta, T^-1 theta and the split's mixture of
    the two; everything stays finite (all coordinates are unconstrained)."""
    h = fits[variant]
    blk = _block(h)[:, :40].contiguous()
    orc = Oracle(h)
    rng = np.random.default_rng(5)
    polls = [outlier_data(variant)[1], 0, h.n_polls - 1, int(h.data["N_state_polls"])]
    B = len(polls)
    a, b = rng.normal(0, 0.3, (B, h.D)), rng.uniform(0.5, 2.0, (B, h.D))
    th = blk.cpu().numpy()[:, :, 7:]
    it_odd = (np.arange(th.shape[1]) % 2 == 1)[None, :, None]
    for integrate in (False, True):
        for sel in (1, 2, 3):
            lp, ll, _ = _ratios(h, blk, a, b, polls, [sel] * B, integrate, lp0=False)
            assert np.isfinite(lp).all() and np.isfinite(ll).all()
            for k in range(B):
                fwd, inv = a[k] + b[k] * th, (th - a[k]) / b[k]
                x = fwd if sel == 1 else inv if sel == 2 else np.where(it_odd, inv, fwd)
                x = x.reshape(-1, h.D)
                lpo = orc.log_prob(x)
                assert np.all(np.abs(lp[k].reshape(-1) - lpo) <= 1e-11 * np.abs(lpo)), (sel, k)
                llo = orc.log_lik(polls[k], integrate)(x)
                assert np.abs(ll[k].reshape(-1) - llo).max() < 1e-9, (sel, k, integrate)


def test_a_nan_in_the_map_is_that_poll_s_alone(fits):
    import torch
    h = fits["three"]
    blk = _block(h)
    polls = [0, 1, 2]
    a, b = np.zeros((3, h.D)), np.ones((3, h.D))
    a[1, 5] = np.nan
    lp, ll, lp0 = _ratios(h, blk, a, b, polls, [1, 1, 1], True)
    assert np.isfinite(lp[[0, 2]]).all() and np.isfinite(ll[[0, 2]]).all() and not np.isfinite(lp[1]).any()
    r = ref.ratios(ll.reshape(3, -1), lp.reshape(3, -1), lp0.reshape(-1))
    assert np.all(r[1] == -np.inf) and np.isfinite(r[[0, 2]]).all()
    lw, k = _psis(torch.tensor(r.reshape(lp.shape), device=blk.device), np.ones(3))
    assert np.isnan(k[1]) and np.isfinite(k[[0, 2]]).all() and np.isnan(lw[1]).all()      # the candidate is rejected


# ---------------------------------------------------------------------------------------------- moments
def _moments(L, blk, w, m0, is_log=False):
    import torch
    Cn, n, row = blk.shape
    D, B = row - 7, w.shape[0]
    wd = torch.tensor(np.ascontiguousarray(w), device=blk.device)
    mu, q = np.zeros((B, D)), np.zeros((B, D))
    m0 = None if m0 is None else np.ascontiguousarray(m0, dtype=np.float64)
    rc = L.potus_loo_mm_moments_device(int(blk.device.index or 0), C.c_void_p(blk.data_ptr()), Cn, n, D, C.c_void_p(wd.data_ptr()), B, int(is_log),
                                       None if m0 is None else m0.ctypes.data_as(DP), mu.ctypes.data_as(DP), q.ctypes.data_as(DP))
    assert rc == 0, rc
    return mu, q


@pytest.mark.parametrize("which", ["three", "full"])     # S = 501 (one chunk, no multiple of 16 or 64) and 2000 (four chunks)
def test_weighted_moments_against_fsum(fits, which):
    h = fits[which]
    blk = _block(h)
    th = blk.cpu().numpy()[:, :, 7:].reshape(-1, h.D)
    S = th.shape[0]
    assert S == (501 if which == "three" else 2000) and h.D % 16 != 0
    rng = np.random.default_rng(9)
    m0 = th.mean(axis=0)
    u = np.full((1, S), 1.0 / S)
    mu_u, _ = _moments(h.L, blk, u, None)
    _, q_u = _moments(h.L, blk, u, mu_u[0])
    assert np.allclose(mu_u[0], m0, rtol=1e-13, atol=1e-15) and np.allclose(q_u[0] * S / (S - 1), th.var(axis=0, ddof=1), rtol=1e-12)
    wall = rng.exponential(1.0, (17, S)) * (rng.random((17, S)) < 0.7)
    wall[0] = rng.exponential(1.0, S)                      # poll 0 has no zero weight: its logarithms go through the is_log path
    wall /= wall.sum(axis=1, keepdims=True)
    got = {}
    for B in (1, 16, 17):
        w = wall[:B]
        mu, q = _moments(h.L, blk, w, m0)
        mu2, q2 = _moments(h.L, blk, w, m0)
        assert mu2.tobytes() == mu.tobytes() and q2.tobytes() == q.tobytes()              # the same bytes on a second call
        got[B] = (mu, q)
        for b in range(B):
            for j in range(h.D):                           # every entry
                t1 = w[b] * th[:, j]
                t2 = w[b] * (th[:, j] - m0[j]) ** 2
                assert abs(mu[b, j] - math.fsum(t1)) <= S * 2.0**-52 * math.fsum(np.abs(t1)), (B, b, j)
                assert abs(q[b, j] - math.fsum(t2)) <= S * 2.0**-52 * math.fsum(t2), (B, b, j)
    # log weights in: w = exp(log w) differs from w by an ulp, so the bound is the same sum's with one more rounding per term (S + 1 for S)
    lw = np.log(wall[:1])
    mul, ql = _moments(h.L, blk, lw, m0, is_log=True)
    wl = np.exp(lw[0])
    for j in range(h.D):
        t1, t2 = wl * th[:, j], wl * (th[:, j] - m0[j]) ** 2
        assert abs(mul[0, j] - math.fsum(t1)) <= (S + 2) * 2.0**-52 * math.fsum(np.abs(t1)), j
        assert abs(ql[0, j] - math.fsum(t2)) <= (S + 2) * 2.0**-52 * math.fsum(t2), j
    # a poll's moments do not depend on the polls beside it
    assert got[17][0][:16].tobytes() == got[16][0].tobytes() and got[17][1][:16].tobytes() == got[16][1].tobytes()
    assert got[16][0][:1].tobytes() == got[1][0].tobytes() and got[16][1][:1].tobytes() == got[1][1].tobytes()


# ---------------------------------------------------------------------------------------------- PSIS of general ratios
def _psis(r, r_eff):
    import torch
    from us_potus_model_amd.sampler import load_library
    L = load_library()
    B, Cn, n = r.shape
    lw = torch.full_like(r, float("nan"))
    k = np.zeros(B)
    re = np.ascontiguousarray(r_eff, dtype=np.float64)
    rc = L.potus_psis_device(int(r.device.index or 0), C.c_void_p(r.data_ptr()), B, Cn, n, re.ctypes.data_as(DP), C.c_void_p(lw.data_ptr()), k.ctypes.data_as(DP))
    assert rc == 0, rc
    return lw.cpu().numpy().reshape(B, -1), k


def _close(a, b, tol=1e-8):
    a, b = np.asarray(a), np.asarray(b)
    assert np.array_equal(np.isinf(a), np.isinf(b)) and np.array_equal(np.isnan(a), np.isnan(b))
    fin = np.isfinite(b)
    if fin.any():
        err = np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))
        assert err.max() <= tol, float(err.max())


@pytest.mark.parametrize("integrate", [False, True])
def test_psis_of_minus_ll_is_potus_loo_s(fits, loos, integrate):
    import torch
    from scipy.special import logsumexp
    h = fits["full"]
    lo = loos[("full", integrate)]
    t = torch.empty((h.n_polls, h.opts.chains, h.post_warmup_saved()), dtype=torch.float64, device=f"cuda:{h.opts.device}")
    h.log_lik_device(0, h.n_polls, t, integrate=integrate)
    lw, k = _psis((-t).contiguous(), lo.r_eff)
    assert np.abs(k - lo.pareto_k).max() <= 1e-12
    ll = t.cpu().numpy().reshape(h.n_polls, -1)
    assert np.abs(logsumexp(ll + lw, axis=1) - lo.pointwise[:, 0]).max() <= 1e-12 * np.abs(lo.pointwise[:, 0]).max()


def test_psis_of_general_ratios_matches_the_restatement():
    import torch
    rng = np.random.default_rng(21)
    r = rng.normal(0, 1.5, (7, 3, 167)) + 0.5 * rng.standard_t(3, (7, 3, 167))
    r[1].reshape(-1)[rng.choice(501, 60, replace=False)] = -np.inf            # weight 0
    x = r[2].reshape(-1)
    x[x > np.quantile(x, 0.9)] = np.quantile(x, 0.9)                           # ties: the largest ratios are one value
    x = r[3].reshape(-1)
    x[:] = np.round(x, 1)                                                      # ties everywhere
    r[4] = -np.inf                                                             # nothing finite
    r[5, 1, 7] = np.nan
    r[6] = rng.normal(0, 1.5, (3, 167))
    r[6].reshape(-1)[:450] = -np.inf                                           # fewer finite ratios than the tail holds
    r_eff = np.array([1.0, 0.6, 1.0, 0.3, 1.0, 1.0, 1.0])
    lw, k = _psis(torch.tensor(r, device="cuda:0"), r_eff)
    for p in range(7):
        lwr, kr = ref.psis_general(r[p], r_eff[p])
        if p in (4, 5):
            assert np.isnan(kr) and np.isnan(k[p]) and np.isnan(lw[p]).all()
            continue
        _close(k[p], kr)
        _close(lw[p], lwr)
    big = rng.normal(0, 1.5, (2, 16, 1000))                                    # more than one sorted run
    lw, k = _psis(torch.tensor(big, device="cuda:0"), np.ones(2))
    for p in range(2):
        lwr, kr = ref.psis_general(big[p], 1.0)
        _close(k[p], kr)
        _close(lw[p], lwr)


# ---------------------------------------------------------------------------------------------- the whole call
def _reference(h, lo, poll, integrate, max_iters, k_threshold=None):
    orc = Oracle(h)
    n = h.post_warmup_saved()
    th = h.draws()[:, -n:, 7:].reshape(-1, h.D)
    return ref.moment_match(th, n, orc.log_prob, orc.log_lik(poll, integrate), lo.r_eff[poll], k_threshold=k_threshold, max_iters=max_iters, split=True)


_REF_CACHE = {}


def _whole_call_case(fits, loos, which, poll, integrate, split, max_iters, k_threshold=None):
    """k_threshold None: the default threshold, and the poll must have k-hat > 0.7; a number: that threshold for the reference and the device."""
    h, lo = fits[which], loos[(which, integrate)]
    key = (which, poll, integrate, max_iters, k_threshold)
    if key not in _REF_CACHE:
        _REF_CACHE[key] = _reference(h, lo, poll, integrate, max_iters, k_threshold)
    want = _REF_CACHE[key]
    thr = ref.default_threshold(lo.n_draws) if k_threshold is None else k_threshold
    assert k_threshold is not None or lo.pareto_k[poll] > 0.7
    kw = {} if k_threshold is None else dict(k_threshold=k_threshold)
    # every decision of the reference compares two k's: they must not be close
    kcur = want["k0"]
    for c, k1, ok in want["steps"]:
        assert abs(k1 - kcur) > 1e-6 and (not ok or abs(k1 - thr) > 1e-6), (poll, c, k1, kcur)
        if ok:
            kcur = k1
    got = loo_mod.moment_match([h], lo, polls=[poll], max_iters=max_iters, split=split, **kw)
    info = got.mm_info[poll]
    print(f"{which} poll {poll} integrate={integrate} split={split}: steps {[(c, round(k, 4), ok) for c, k, ok in want['steps']]} k0 {want['k0']:.4f} "
          f"k {got.pareto_k[poll]:.4f} elpd {lo.pointwise[poll, 0]:.4f} -> {got.pointwise[poll, 0]:.4f} ms {got.mm_ms}")
    assert tuple(info[:3]) == want["info"][:3] and info[4] == want["info"][3]
    assert info[3] == int(split and want["split_done"])
    acc = [want["k0"]] + [k1 for _, k1, ok in want["steps"] if ok]
    k_end, elpd_end = (want["k"], want["elpd"]) if (split and want["split_done"]) else (want["k_loop"], want["elpd_loop"])
    if split and want["split_done"]:
        acc.append(want["k"])
    path = got.mm_k_path[poll]
    assert np.isnan(path[len(acc):]).all() and np.abs(path[:len(acc)] - np.array(acc)).max() <= 1e-8
    a, b = got.mm_map[0]
    assert np.all(np.abs(a - want["a"]) <= 1e-9 * np.maximum(1, np.abs(want["a"]))) and np.all(np.abs(b - want["b"]) <= 1e-9 * np.maximum(1, np.abs(want["b"])))
    if want["info"][0] + want["info"][1] > 0:
        assert abs(got.pareto_k[poll] - k_end) <= 1e-8 and abs(got.pointwise[poll, 0] - elpd_end) <= 1e-8
        lpd = lo.pointwise[poll, 0] + lo.pointwise[poll, 1]
        assert got.pointwise[poll, 1] == lpd - got.pointwise[poll, 0] and got.pointwise[poll, 2] == -2.0 * got.pointwise[poll, 0]
    else:
        assert got.pointwise[poll].tobytes() == lo.pointwise[poll].tobytes()
    others = np.arange(h.n_polls) != poll
    assert got.pointwise[others].tobytes() == lo.pointwise[others].tobytes() and got.pointwise[poll, 4] == lo.pointwise[poll, 4]
    assert np.allclose(got.estimates, psis_ref.estimates(got.pointwise), rtol=1e-12)
    return want


@pytest.mark.parametrize("split", [True, False])
def test_whole_call_with_accepted_mean_steps(fits, loos, split):
    """The polls above the threshold accept only variance steps on this posterior, so the mean step a' = a + (mu_w - m) and its composition
    with later steps is held against the reference with k_threshold = -1, where every poll enters the loop.  A batch call over all polls
    names the polls that accept a T1 step; the reference must accept it too (asserted, like everything else, against the reference)."""
    h = fits["three"]
    for integrate in (False, True):
        lo = loos[("three", integrate)]
        allp = loo_mod.moment_match([h], lo, k_threshold=-1.0, max_iters=3)
        cand = np.flatnonzero(allp.mm_info[:, 0] > 0)
        if cand.size:
            break
    assert cand.size, "no poll of either form accepts a mean step"
    order = cand[np.argsort(-(allp.mm_info[cand, 0] + allp.mm_info[cand, 1]))]     # the longest composition first
    poll = int(order[0])
    want = _whole_call_case(fits, loos, "three", poll, integrate, split, 3, k_threshold=-1.0)
    assert want["info"][0] >= 1, want["steps"]
    one = loo_mod.moment_match([h], lo, polls=[poll], k_threshold=-1.0, max_iters=3, split=True)
    assert one.pointwise[poll].tobytes() == allp.pointwise[poll].tobytes()


@pytest.mark.parametrize("split", [True, False])
def test_whole_call_on_the_planted_outlier_integrated(fits, loos, split):
    _whole_call_case(fits, loos, "full", outlier_data("full")[1], True, split, 4)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("poll", PLAIN_POLLS)
def test_whole_call_on_plain_polls(fits, loos, poll, split):
    _whole_call_case(fits, loos, "three", poll, False, split, 6)


# ---------------------------------------------------------------------------------------------- behaviour
def test_nothing_to_do_returns_the_rows_byte_for_byte(fits, loos):
    h, lo = fits["full"], loos[("full", True)]
    for kw in (dict(k_threshold=1e9), dict(max_iters=0), dict(max_iters=0, k_threshold=-1.0)):
        got = loo_mod.moment_match([h], lo, **kw)
        assert got.pointwise.tobytes() == lo.pointwise.tobytes() and got.estimates.tobytes() == lo.estimates.tobytes()
        assert not got.mm_info[:, :4].any()


def test_a_poll_s_row_does_not_depend_on_the_batch(fits, loos):
    h, lo = fits["three"], loos[("three", False)]
    allp = loo_mod.moment_match([h], lo, k_threshold=-1.0, max_iters=3)
    again = loo_mod.moment_match([h], lo, k_threshold=-1.0, max_iters=3)
    assert allp.pointwise.tobytes() == again.pointwise.tobytes() and allp.mm_k_path.tobytes() == again.mm_k_path.tobytes()
    assert (allp.mm_info[:, 0] + allp.mm_info[:, 1] > 0).sum() >= 3
    some = [int(i) for i in np.argsort(-lo.pareto_k)[:5]]
    rev = loo_mod.moment_match([h], lo, polls=some[::-1], k_threshold=-1.0, max_iters=3)
    fwd = loo_mod.moment_match([h], lo, polls=some, k_threshold=-1.0, max_iters=3)
    assert rev.pointwise.tobytes() == fwd.pointwise.tobytes() and rev.mm_map[::-1].tobytes() == fwd.mm_map.tobytes()
    for i in some:
        one = loo_mod.moment_match([h], lo, polls=[i], k_threshold=-1.0, max_iters=3)
        assert one.pointwise[i].tobytes() == allp.pointwise[i].tobytes() == rev.pointwise[i].tobytes()
        assert one.mm_info[i].tobytes() == allp.mm_info[i].tobytes() and one.mm_k_path[i].tobytes() == allp.mm_k_path[i].tobytes()
    assert np.isfinite(allp.pointwise).all()
    rows = loo_mod.loo_compare(allp, lo)
    assert len(rows) == 2


def test_cluster_fit_with_a_separate_model_handle_and_pooled_handles(fits):
    data = outlier_data("full")[0]
    c4 = _fit(data, "full", chains=4, cus_per_chain=4)
    lo = loo_mod.loo([c4], integrate=True)
    got = loo_mod.moment_match([c4], lo, max_iters=2)            # creates and closes a one-chain handle for the model
    assert np.isfinite(got.pointwise).all() and (got.mm_info[:, 0] + got.mm_info[:, 1]).sum() >= 1
    with pytest.raises(PotusError, match="one workgroup per chain"):
        loo_mod.moment_match([c4], lo, model_handle=c4)
    c4.close()
    one = fits["full"]
    a = _fit(data, "full", chains=2)
    b = _fit(data, "full", chains=2, chain_id_offset=2)
    assert np.concatenate([a.draws(), b.draws()]).tobytes() == one.draws().tobytes()
    lo1, lo2 = loo_mod.loo([one], integrate=True), loo_mod.loo([a, b], integrate=True)
    m1, m2 = loo_mod.moment_match([one], lo1, max_iters=2), loo_mod.moment_match([a, b], lo2, max_iters=2, model_handle=one)
    assert m1.pointwise.tobytes() == m2.pointwise.tobytes() and m1.mm_info.tobytes() == m2.mm_info.tobytes()
    a.close()
    b.close()


def test_refusals_come_before_any_kernel(fits, loos):
    h, lo = fits["full"], loos[("full", True)]
    data = outlier_data("full")[0]
    with pytest.raises(PotusError, match="singular"):
        loo_mod.moment_match([h], lo, cov=True)
    d = Handle(data, "full", chains=1, num_warmup=1, num_samples=1, metric=1)
    with pytest.raises(PotusError, match="dense metric"):
        loo_mod.moment_match([h], lo, model_handle=d)
    d.close()
    m = Handle(data, "full", chains=2, num_warmup=5, num_samples=5, cus_per_chain=1, twin=0)
    ys, yn = np.asarray(data["n_democrat_state"])[None], np.asarray(data["n_democrat_national"])[None]
    m.set_datasets(np.repeat(ys, 2, 0), np.repeat(yn, 2, 0))
    with pytest.raises(PotusError, match="data sets"):
        loo_mod.moment_match([h], lo, model_handle=m)
    with pytest.raises(PotusError, match="data sets"):
        loo_mod.moment_match([m], lo, model_handle=h)
    m.close()
    o = Handle(dict(data, n_democrat_state=np.asarray(data["n_democrat_state"]) // 2), "full", chains=1, num_warmup=1, num_samples=1, cus_per_chain=1, twin=0)
    with pytest.raises(PotusError, match="another model"):
        loo_mod.moment_match([h], lo, model_handle=o)
    o.close()
    with pytest.raises(PotusError, match="not potus_loo's"):
        loo_mod.moment_match([h], loos[("full", False)], integrate=True, max_iters=1)     # rows of the other form
    ms = np.ones(4)
    assert h.L.potus_loo_mm_timing(ms.ctypes.data_as(DP)) == 0


def test_r_entry_point_gives_the_bytes_of_the_c_call(fits, loos):
    h, lo = fits["three"], loos[("three", True)]
    want = loo_mod.moment_match([h], lo, max_iters=2)
    pw, est, info, st = np.array(lo.pointwise), np.zeros(6), np.zeros((h.n_polls, 6), np.int32), C.c_int(-1)
    h.L.potus_R_loo_moment_match(C.byref(C.c_int(h.h)), (C.c_int * 1)(h.h), C.byref(C.c_int(1)), (C.c_int * 5)(1, 2, 1, 0, 0), C.byref(C.c_double(0.0)),
                                 (C.c_int * 1)(0), pw.ctypes.data_as(DP), est.ctypes.data_as(DP), info.ctypes.data_as(C.POINTER(C.c_int)), C.byref(st))
    assert st.value == 0
    assert pw.tobytes() == want.pointwise.tobytes() and est.tobytes() == want.estimates.tobytes() and info.tobytes() == want.mm_info.tobytes()
