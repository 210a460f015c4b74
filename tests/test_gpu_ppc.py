"""Posterior predictive checks on the MI355X (potus_ppc.hpp): the replicate sampler in distribution against scipy, the
stage kernels against the numpy restatement (tests/ppc_ref.py) with their edge groups and edge weights, the bytes the call promises, that the
check finds a planted misfit and is silent on clean fits, and the refusals.  The fits are test_gpu_loo.py's (synthetic.small, both variants,
4 chains, 300 + 500) and three more: polls of 3 .. 19 respondents with n = 0, y = 0 and y = n among them; 290 polls; the planted misfit."""
import ctypes as C

import numpy as np
import pytest
from scipy import integrate as sci_int, special, stats

import ppc_ref as ref
from conftest import second_device
from test_gpu_loo import NS, NW, SEED, VARIANTS, _fit, _polls
from us_potus_model_amd import loo as loo_mod, ppc, synthetic
from us_potus_model_amd.sampler import Handle, PotusError, run_many

pytestmark = pytest.mark.gpu
DP, IP, LLP = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
MISFIT_SEED = 7
FITS = ("full", "no_mode_adjustment", "low", "big")


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def _low_data():
    """synthetic.small("full") with ten polls of 3 .. 19 respondents (the inversion branch of the sampler), their outcomes scaled to match, one
    of them with y = 0 and one with y = n, and an eleventh poll with n = 0."""
    d = dict(synthetic.small("full"))
    sizes = np.rint(np.linspace(3, 19, 10)).astype(int)
    for key, idx, ns in (("state", np.arange(8), sizes[:8]), ("national", np.arange(2), sizes[8:])):
        n2, y = np.array(d[f"n_two_share_{key}"]).copy(), np.array(d[f"n_democrat_{key}"]).copy()
        y[idx] = np.rint(y[idx] * ns / n2[idx]).astype(int)
        n2[idx] = ns
        d[f"n_two_share_{key}"], d[f"n_democrat_{key}"] = n2.astype(np.int32), y.astype(np.int32)
    d["n_democrat_state"][0] = 0
    d["n_democrat_state"][1] = d["n_two_share_state"][1]
    d["n_two_share_national"][2] = 0
    d["n_democrat_national"][2] = 0
    return d


def _misfit_data():
    """synthetic.small("full") with the outcomes of the most frequent pollster's polls drawn again with ten times the measurement noise the data
    list states: the model still believes sigma.  Returns (data, the pollster's label, its polls)."""
    d = dict(synthetic.small("full", seed=MISFIT_SEED))
    rng = np.random.default_rng(99)
    pol = np.concatenate([d["poll_state"], d["poll_national"]]) - 1
    worst = int(np.bincount(pol).argmax())
    for key in ("state", "national"):
        y, n = np.array(d[f"n_democrat_{key}"]).astype(float), np.array(d[f"n_two_share_{key}"]).astype(float)
        sel = np.flatnonzero(np.asarray(d[f"poll_{key}"]) - 1 == worst)
        eta = special.logit(np.clip(y[sel] / n[sel], 0.01, 0.99)) + 10.0 * float(d[f"sigma_measure_noise_{key}"]) * rng.normal(size=sel.size)
        y[sel] = rng.binomial(n[sel].astype(int), special.expit(eta))
        d[f"n_democrat_{key}"] = y.astype(np.int32)
    return d, worst, np.flatnonzero(pol == worst)


@pytest.fixture(scope="module")
def fits():
    out = {v: _fit(synthetic.small(v), v) for v in VARIANTS}
    out["low"] = _fit(_low_data(), "full")
    big = synthetic.make(S=6, T=24, N_state=230, N_national=60, P=9)
    h = Handle(big, "full", chains=2, num_warmup=100, num_samples=60, seed=SEED, cus_per_chain=1, twin=0)
    h.init()
    h.run(160)
    out["big"] = h
    yield out
    for h in out.values():
        h.close()


@pytest.fixture(scope="module")
def checks(fits):
    """ppc.check of every fit, integrate = 1, rep = 0: computed once, compared by many tests, never changed"""
    return {k: ppc.check(h) for k, h in fits.items()}


def _cols(h, *names):
    n = h.draws_saved()
    return np.concatenate([h.write_array(h.layout[k][0], h.layout[k][1], n).transpose(2, 1, 0) for k in names])


def _eta_z(h):
    """(eta without the noise term, sigma, z) per poll and pooled draw [N, S], from the logit_pi_* and raw_measure_noise_* columns"""
    _, _, sig = _polls(h.data)
    N, w = h.n_polls, h.draws_saved() - h.post_warmup_saved()
    z = _cols(h, "raw_measure_noise_state", "raw_measure_noise_national")[:, :, w:].reshape(N, -1)
    lp = _cols(h, "logit_pi_democrat_state", "logit_pi_democrat_national")[:, :, w:].reshape(N, -1)
    return lp - sig[:, None] * z, sig, z


def _flat(t):
    return t.cpu().numpy().reshape(t.shape[0], -1)


def _blocks(h, integrate, rep=0):
    """the device's own blocks of a fit over every poll: y_rep, a1, a2 (torch, on the GPU)"""
    a1, a2 = h.poll_share_device(0, h.n_polls, integrate=integrate)
    return h.poll_rep_device(0, h.n_polls, integrate=integrate, rep=rep), a1, a2


def _weights(h, integrate):
    """(normalised PSIS log weights [N, chains, draws] on the GPU, potus_loo's pointwise rows) as potus_ppc forms them"""
    import torch
    ll = torch.empty((h.n_polls, h.opts.chains, h.post_warmup_saved()), dtype=torch.float64, device=f"cuda:{h.opts.device}")
    h.log_lik_device(0, h.n_polls, ll, integrate=integrate)
    pw = loo_mod.loo_of_block(ll).pointwise
    re = np.where(np.isfinite(pw[:, 4]) & (pw[:, 4] > 0), pw[:, 4], 1.0)
    lw, _ = loo_mod.psis_weights((-ll).contiguous(), re)
    return lw, pw


def _standardised(got, exact, sd, what):
    """|got - exact| <= 5 sd + 1e-12 per poll and sum of squares below N + 5 sqrt(2 N) over the polls with sd > 0; returns the largest deviation"""
    assert (np.abs(got - exact) <= 5.0 * sd + 1e-12).all(), (what, float(np.max(np.abs(got - exact) / np.maximum(sd, 1e-300))))
    ok = sd > 0
    zz = (got[ok] - exact[ok]) / sd[ok]
    N = int(ok.sum())
    print(f"{what}: largest standardised deviation {np.abs(zz).max():.3f}, sum of squares {np.sum(zz * zz):.1f} over {N} polls (bound {N + 5 * np.sqrt(2 * N):.1f})")
    assert np.sum(zz * zz) < N + 5.0 * np.sqrt(2.0 * N), what
    return float(np.abs(zz).max())


# ------------------------------------------------------------------------------------------------ 1. the sampler, in distribution
@pytest.mark.parametrize("name", FITS)
def test_plain_replicates_follow_the_binomial_of_the_logit_pi_columns(fits, name):
    h = fits[name]
    y, n, _ = _polls(h.data)
    w = h.draws_saved() - h.post_warmup_saved()
    p = special.expit(_cols(h, "logit_pi_democrat_state", "logit_pi_democrat_national")[:, :, w:].reshape(h.n_polls, -1))
    yr = h.poll_rep_device(0, h.n_polls, integrate=False)
    lo, eq = ppc.pit_of_block(yr, y)
    yrep = _flat(yr)
    assert ((yrep >= 0) & (yrep <= n[:, None]) & (yrep == np.rint(yrep))).all()
    rlo, req = ref.pit_sums(yrep, y)
    assert lo.tobytes() == rlo.tobytes() and eq.tobytes() == req.tobytes()      # (equal weights: exact counts over S)
    S = p.shape[1]
    for k, got in ((y - 1, lo), (y, lo + eq)):
        F = np.where(n[:, None] > 0, stats.binom.cdf(k[:, None], np.maximum(n, 1)[:, None], p), (k >= 0)[:, None] * 1.0)
        _standardised(got, F.mean(axis=1), np.sqrt((F * (1 - F)).mean(axis=1) / S), f"{name} plain F(y{'' if k is y else ' - 1'})")
    if name == "low":
        assert (yrep[95 - 25 + 2] == 0).all() and lo[72] == 0 and eq[72] == 1                       # the n = 0 poll (national poll 2)
        assert lo[0] == 0 and abs(lo[1] + eq[1] - 1) < 1e-15                                      # y = 0, y = n


def _quad_cdf(k, n, eta, sig):
    """int F(k | n, inv_logit(eta + sig z)) phi(z) dz by scipy.integrate.quad, the point where F crosses from 1 to 0 (p = (k + 1/2) / n) a break point"""
    if k < 0:
        return 0.0
    if k >= n:
        return 1.0
    k, n = int(k), int(n)
    f = lambda z: special.bdtr(k, n, special.expit(eta + sig * z)) * np.exp(-0.5 * z * z) * 0.3989422804014327
    if sig == 0.0:
        return float(special.bdtr(k, n, special.expit(eta)))
    zb = float(np.clip((special.logit((k + 0.5) / n) - eta) / sig, -7.9, 7.9))
    return sci_int.quad(f, -8.0, 8.0, points=[zb], epsabs=1e-11, epsrel=1e-10, limit=200)[0]


def _quad_cdf_of_draws(k, n, eta, sig, rng, nodes=65):
    """_quad_cdf at every draw's eta [S].  A quad per draw is half a millisecond, 2 000 draws x 20 polls x 2 bounds a minute; the integral is an
    entire function of eta that crosses from 1 to 0 over at least sig (0.04) while the draws of one poll span a few tenths: quad at `nodes`
    Chebyshev points of [min eta, max eta], the interpolating polynomial at the draws, and that against quad itself at 12 random draws to 1e-9."""
    if k < 0 or k >= n:
        return np.full(len(eta), 0.0 if k < 0 else 1.0)
    a, b = float(eta.min()), float(eta.max())
    x = np.cos(np.pi * (np.arange(nodes) + 0.5) / nodes)
    c = np.polynomial.chebyshev.chebfit(x, [_quad_cdf(k, n, 0.5 * (a + b) + 0.5 * (b - a) * t, sig) for t in x], nodes - 1)
    F = np.polynomial.chebyshev.chebval((2.0 * eta - (a + b)) / (b - a), c)
    for s in rng.integers(0, len(eta), 12):
        assert abs(F[s] - _quad_cdf(k, n, eta[s], sig)) < 1e-9
    return np.clip(F, 0.0, 1.0)


@pytest.mark.parametrize("name", ["full", "low"])
def test_integrated_replicates_follow_the_quadrature_of_the_binomial(fits, name):
    h = fits[name]
    y, n, sig = _polls(h.data)
    eta, _, _ = _eta_z(h)
    Ns = int(h.data["N_state_polls"])
    polls = (list(range(8)) + [20, 40, Ns, Ns + 1, Ns + 2, Ns + 10]) if name == "low" else (list(range(0, 70, 7)) + [Ns, Ns + 3, Ns + 7, Ns + 11, Ns + 20])   # (at most twenty)
    yr = h.poll_rep_device(0, h.n_polls, integrate=True)
    lo, eq = ppc.pit_of_block(yr, y)
    S = eta.shape[1]
    rng = np.random.default_rng(8)
    for k, got, what in ((y - 1, lo, "F(y - 1)"), (y, lo + eq, "F(y)")):
        F = np.array([_quad_cdf_of_draws(k[i], n[i], eta[i], sig[i], rng) for i in polls])
        _standardised(got[polls], F.mean(axis=1), np.sqrt((F * (1 - F)).mean(axis=1) / S), f"{name} integrated {what}")


@pytest.mark.parametrize("name", FITS)
def test_integrated_replicates_have_the_mean_and_variance_of_the_shares(fits, name):
    """Given the draws, E[y_rep_s] = m_s and var[y_rep_s] = v_s: the mean of y_rep over the draws against mean m (sd sqrt(mean v / S)), its variance
    against mean v + var m (sd from the spread of the squared deviations)."""
    h = fits[name]
    _, n, _ = _polls(h.data)
    yr, a1, a2 = (_flat(t) for t in _blocks(h, True))
    m, sd = ref.moments(n, a1, a2)
    v, S = sd * sd, yr.shape[1]
    mean, var = yr.mean(axis=1), yr.var(axis=1)
    zero = n == 0
    assert (mean[zero] == 0).all() and (var[zero] == 0).all()
    _standardised(mean, m.mean(axis=1), np.sqrt(v.mean(axis=1) / S), f"{name} mean of y_rep")
    d2 = (yr - mean[:, None]) ** 2
    _standardised(var, v.mean(axis=1) + m.var(axis=1), d2.std(axis=1) / np.sqrt(S), f"{name} variance of y_rep")


# ------------------------------------------------------------------------------------------------ 2. the stage kernels against ppc_ref.py
def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


def _edge_labels(N, n, G):
    """labels with a group of one poll (0), an unused label (G - 1), polls in no group (-1), and the rest spread over 1 .. G - 2"""
    lab = 1 + (np.arange(N) * 7) % (G - 2)
    lab[3] = 0
    lab[(np.arange(N) % 11) == 5] = -1
    return lab.astype(np.int32)


def _check_groups(yr, a1, a2, y, n, lab, G, cut):
    """potus_ppc_groups_device in one block, and in two blocks cut at `cut` with the accumulators kept on the device, against the restatement"""
    import torch
    N, C_, D_ = yr.shape
    f = lambda t: _flat(t)
    T, cnt = ref.group_sums(f(yr), f(a1), f(a2), y, n, lab, G)
    tab = ref.group_table(T, cnt)
    acc = torch.full((G, 3, 2, C_, D_), 7.0, dtype=torch.float64, device=yr.device)               # (BEGIN zeroes it)
    one, c1 = ppc.groups_of_block(yr, a1, a2, y, n, lab, G, acc=acc)
    A = acc.cpu().numpy().reshape(G, 3, 2, -1)
    assert cnt.tolist() == c1.tolist()
    assert A[:, 2].tobytes() == T[:, 2].tobytes()                                                   # the counts N: exact
    assert (np.abs(A - T) <= 1e-12 * (1.0 + np.abs(T))).all(), float(np.max(np.abs(A - T) / (1.0 + np.abs(T))))
    used = cnt > 0
    assert np.allclose(one[used, :, :2], tab[used, :, :2], rtol=1e-12, atol=1e-12) and np.isnan(one[~used][:, :, [0, 1, 5]]).all() and (one[~used][:, :, 2:5] == 0).all()
    assert (one[used, :, 2:5].sum(axis=2) == C_ * D_).all()
    assert one[:, 2, 2:].tobytes() == tab[:, 2, 2:].tobytes()                                       # the counts of N: exact
    near = ref.near_ties(T)
    assert near.max() <= 1e-3 * C_ * D_, near.max()
    moved = np.abs(one[used, :2, 2:5] - tab[used, :2, 2:5]).sum(axis=2) / 2
    assert (moved <= near[used, :2]).all()
    assert (np.abs(one[used, :, 5] - tab[used, :, 5]) <= near[used] / (C_ * D_)).all()
    # two blocks, the cut inside several groups: the bytes of one block
    acc2, c2 = torch.empty_like(acc), np.zeros(G, np.int64)
    ppc.groups_of_block(yr[:cut].contiguous(), a1[:cut].contiguous(), a2[:cut].contiguous(), y[:cut], n[:cut], lab[:cut], G, acc=acc2, flags=ppc.BEGIN, n_in_group=c2)
    two, c2 = ppc.groups_of_block(yr[cut:].contiguous(), a1[cut:].contiguous(), a2[cut:].contiguous(), y[cut:], n[cut:], lab[cut:], G, acc=acc2, flags=ppc.FINISH,
                                  n_in_group=c2)
    assert torch.equal(acc, acc2) and two.tobytes() == one.tobytes() and c2.tolist() == c1.tolist()
    # without a buffer of the caller's
    three, c3 = ppc.groups_of_block(yr, a1, a2, y, n, lab, G)
    assert three.tobytes() == one.tobytes() and c3.tolist() == c1.tolist()
    return one, T


@pytest.mark.parametrize("name", ["full", "low"])
def test_stage_kernels_on_the_device_blocks(fits, name):
    h = fits[name]
    y, n, _ = _polls(h.data)
    yr, a1, a2 = _blocks(h, True)
    lw, _ = _weights(h, True)
    for w in (None, lw):
        lo, eq = ppc.pit_of_block(yr, y, w)
        rlo, req = ref.pit_sums(_flat(yr), y, None if w is None else _flat(w))
        assert np.allclose(lo, rlo, rtol=1e-12, atol=0) and np.allclose(eq, req, rtol=1e-12, atol=0)
    G = 9
    lab = _edge_labels(h.n_polls, n, G)
    if name == "low":
        lab[72] = 2                                                                                  # the n = 0 poll carries a label and joins no sum
    one, T = _check_groups(yr, a1, a2, y, n, lab, G, cut=41)
    # the group of one poll: the exact ties y_rep = y are the draws counted as equal, in all three statistics
    ties = int((_flat(yr)[3] == y[3]).sum())
    assert ties > 0 and (one[0, :, 3] == ties).all()


@pytest.mark.parametrize("chains,draws", [(3, 37), (4, 250)])
def test_stage_kernels_on_synthetic_blocks(chains, draws):
    rng = np.random.default_rng(100 * chains + draws)
    N, G = 40, 8
    n = rng.integers(5, 900, N).astype(float)
    n[6] = 0.0
    a1 = rng.uniform(0.2, 0.8, (N, chains, draws))
    a2 = a1 * a1 + rng.uniform(0, 1e-3, a1.shape) * (rng.random(a1.shape) < 0.7)                   # (some cells without overdispersion)
    a1[8], a2[8] = 1.0, 1.0                                                                        # v = 0: residual 0
    yrep = rng.binomial(n.astype(int)[:, None, None], a1).astype(float)
    y = rng.binomial(n.astype(int), 0.5).astype(float)
    y[3] = np.sort(yrep[3].reshape(-1))[yrep[3].size // 2]                                         # exact ties in the group of one poll
    lab = _edge_labels(N, n, G)
    lab[6] = 1
    one, T = _check_groups(_dev(yrep), _dev(a1), _dev(a2), y, n, lab, G, cut=17)
    assert one[0, 0, 3] == (yrep[3] == y[3]).sum() > 0
    # the PIT sums: equal weights, PSIS-like weights, a weight of -inf, a poll whose weights are NaN
    lw = rng.normal(0, 2, yrep.shape)
    lw[2, 0, :5] = -np.inf
    lw -= np.log(np.exp(lw).sum(axis=(1, 2), keepdims=True))
    lw[5] = np.nan
    f = lambda a: a.reshape(N, -1)
    for w in (None, lw):
        lo, eq = ppc.pit_of_block(_dev(yrep), y, None if w is None else _dev(w))
        rlo, req = ref.pit_sums(f(yrep), y, None if w is None else f(w))
        assert np.allclose(lo, rlo, rtol=1e-12, atol=0, equal_nan=True) and np.allclose(eq, req, rtol=1e-12, atol=0, equal_nan=True)
        assert np.isnan(lo).sum() == (0 if w is None else 1) and (w is None or (np.isnan(lo[5]) and np.isnan(eq[5])))


# ------------------------------------------------------------------------------------------------ 3. equal bytes
def _same(a, b):
    assert a.pit_lo.tobytes() == b.pit_lo.tobytes() and a.pit_eq.tobytes() == b.pit_eq.tobytes()
    assert a.loo_pit_lo.tobytes() == b.loo_pit_lo.tobytes() and a.loo_pit_eq.tobytes() == b.loo_pit_eq.tobytes() and a.pareto_k.tobytes() == b.pareto_k.tobytes()
    assert list(a.groups) == list(b.groups)
    for k in a.groups:
        for f in ("n_polls", "T_obs", "T_rep", "gt", "eq", "lt", "p_bias", "p_dispersion", "p_count"):
            assert np.asarray(a.groups[k][f]).tobytes() == np.asarray(b.groups[k][f]).tobytes(), (k, f)


@pytest.mark.parametrize("name", ["full", "low"])
def test_twice_and_in_three_blocks_give_the_same_bytes(fits, checks, name, monkeypatch):
    h = fits[name]
    _same(checks[name], ppc.check(h))
    S = h.opts.chains * h.post_warmup_saved()
    monkeypatch.setenv("POTUS_PPC_BLOCK_BUDGET", str(S * 8 * 7 * 40))                               # 95 polls: blocks of 40, 40 and 15
    _same(checks[name], ppc.check(h))
    monkeypatch.setenv("POTUS_PPC_BLOCK_BUDGET", "1")                                               # one poll per block
    few = ppc.check(h, by=("state", "all"))
    for k in ("state", "all"):
        assert few.groups[k]["p_dispersion"].tobytes() == checks[name].groups[k]["p_dispersion"].tobytes()
    assert few.loo_pit_lo.tobytes() == checks[name].loo_pit_lo.tobytes()


def test_two_handles_of_two_chains_give_the_bytes_of_one_handle_of_four(fits, checks):
    d = synthetic.small("full")
    a = Handle(d, "full", chains=2, num_warmup=NW, num_samples=NS, seed=SEED, cus_per_chain=1, twin=0)
    b = Handle(d, "full", chains=2, chain_id_offset=2, device=second_device(), num_warmup=NW, num_samples=NS, seed=SEED, cus_per_chain=1, twin=0)
    a.init()
    b.init()
    run_many([a, b], NW + NS)
    _same(checks["full"], ppc.check([a, b]))
    # a cell's y_rep depends on seed, chain id, iteration, poll and rep alone: the second handle's block is chains 2 and 3 of the one handle's
    whole = fits["full"].poll_rep_device(0, 95, integrate=True)
    part = b.poll_rep_device(20, 61, integrate=True)
    assert np.array_equal(whole[20:61, 2:].cpu().numpy(), part.cpu().numpy())
    a.close()
    b.close()


@pytest.mark.parametrize("integrate", [True, False])
def test_the_call_equals_its_stages_chained_by_hand(fits, checks, integrate):
    h = fits["low"]
    y, n, _ = _polls(h.data)
    got = checks["low"] if integrate else ppc.check(h, integrate=False)
    yr, a1, a2 = _blocks(h, integrate)
    lw, pw = _weights(h, integrate)
    lo, eq = ppc.pit_of_block(yr, y)
    llo, leq = ppc.pit_of_block(yr, y, lw)
    for v in (lo, eq, llo, leq):
        v[n == 0] = np.nan
    assert got.pareto_k.tobytes() == pw[:, 3].tobytes() == loo_mod.loo(h, integrate=integrate).pareto_k.tobytes()
    assert got.pit_lo.tobytes() == lo.tobytes() and got.pit_eq.tobytes() == eq.tobytes() and got.loo_pit_lo.tobytes() == llo.tobytes() and got.loo_pit_eq.tobytes() == leq.tobytes()
    assert np.isnan(got.pit_lo[72]) and np.isnan(got.loo_pit_eq[72]) and np.isfinite(np.delete(got.loo_pit_lo, 72)).all()
    for name, (lab, names) in ppc.groupings(h.data, "full").items():
        out, cnt = ppc.groups_of_block(yr, a1, a2, y, n, lab, len(names))
        g = got.groups[name]
        assert cnt.tolist() == g["n_polls"].tolist() and out[:, :, 0].tobytes() == np.ascontiguousarray(g["T_obs"]).tobytes()
        assert out[:, :, 1].tobytes() == np.ascontiguousarray(g["T_rep"]).tobytes() and out[:, 1, 5].tobytes() == np.ascontiguousarray(g["p_dispersion"]).tobytes()
        assert (out[:, :, 2] == g["gt"]).all() and (out[:, :, 3] == g["eq"]).all() and (out[:, :, 4] == g["lt"]).all()
    assert got.groups["all"]["n_polls"].tolist() == [94] and got.groups["state"]["n_polls"].sum() == 94     # the n = 0 poll is in no group


def test_dot_c_entry_a_second_replicate_and_an_undisturbed_run(fits, checks):
    h, ck = fits["full"], checks["full"]
    N = h.n_polls
    gs = ppc.groupings(h.data, "full", ("pollster", "state"))
    lab = np.ascontiguousarray(np.stack([v[0] for v in gs.values()]), dtype=np.int32)
    ng = np.array([len(v[1]) for v in gs.values()], dtype=np.int32)
    tot = int(ng.sum())
    pit, k, out, cnt, st = np.zeros((N, 4)), np.zeros(N), np.zeros((tot, 3, 6)), np.zeros(tot), C.c_int(-1)
    p = lambda a: a.ctypes.data_as(DP)
    h.L.potus_R_ppc((C.c_int * 1)(h.h), C.byref(C.c_int(1)), (C.c_int * 3)(1, 0, 2), lab.ctypes.data_as(C.POINTER(C.c_int)), ng.ctypes.data_as(C.POINTER(C.c_int)),
                    p(pit), p(k), p(out), p(cnt), C.byref(st))
    assert st.value == 0 and pit[:, 2].tobytes() == ck.loo_pit_lo.tobytes() and pit[:, 1].tobytes() == ck.pit_eq.tobytes() and k.tobytes() == ck.pareto_k.tobytes()
    P_ = len(gs["pollster"][1])
    assert out[:P_, 1, 5].tobytes() == ck.groups["pollster"]["p_dispersion"].tobytes() and out[P_:, 0, 5].tobytes() == ck.groups["state"]["p_bias"].tobytes()
    assert cnt[:P_].tolist() == ck.groups["pollster"]["n_polls"].tolist()
    h.L.potus_R_ppc((C.c_int * 1)(h.h), C.byref(C.c_int(1)), (C.c_int * 3)(2, 0, 0), None, None, p(pit), p(k), None, None, C.byref(st))
    assert st.value == 1
    # rep = 1: another replicate, the same realised side
    r0, r1 = h.poll_rep_device(0, N, rep=0), h.poll_rep_device(0, N, rep=1)
    assert 0.5 < float((r0 != r1).double().mean()) and ck.ms.shape == (4,) and (ck.ms > 0).all()
    two = ppc.check(h, by=("all",), rep=1)
    assert two.loo_pit_lo.tobytes() != ck.loo_pit_lo.tobytes() and two.pareto_k.tobytes() == ck.pareto_k.tobytes()
    assert two.groups["all"]["T_obs"].tobytes() == ck.groups["all"]["T_obs"].tobytes() and two.groups["all"]["T_rep"].tobytes() != ck.groups["all"]["T_rep"].tobytes()
    # a sampling run with a check in its middle gives the bytes of an uninterrupted one
    run = dict(chains=2, num_warmup=20, num_samples=20, seed=SEED, cus_per_chain=1, twin=0)
    a, b = Handle(h.data, "full", **run), Handle(h.data, "full", **run)
    for x in (a, b):
        x.init()
    a.run(40)
    b.run(30)
    b.ppc(by=("pollster",))
    b.run(10)
    assert a.draws().tobytes() == b.draws().tobytes() and a.chain_status() == b.chain_status()
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 4. the check works, and is silent where nothing is wrong
def _p_values(g, min_polls=5):
    ok = g["n_polls"] >= min_polls
    return np.stack([g["p_bias"][ok], g["p_dispersion"][ok], g["p_count"][ok]])


def test_the_planted_misfit_is_found_and_nothing_else(fits):
    data, worst, polls = _misfit_data()
    assert polls.size >= 8
    h = _fit(data, "full")
    ck = ppc.check(h)
    h.close()
    g = ck.groups["pollster"]
    G = len(g["labels"])
    u = ck.pit(loo=True, seed=1)[polls]
    outside = float(((u < 0.1) | (u > 0.9)).mean())
    others = [(g["labels"][j], float(g["p_dispersion"][j])) for j in range(G) if j != worst and g["n_polls"][j] >= 5]
    print(f"misfit: pollster {worst + 1} ({polls.size} polls) p_dispersion {g['p_dispersion'][worst]:.5f}, LOO-PIT mass outside [0.1, 0.9] {outside:.3f}; "
          f"the others' p_dispersion {others}")
    assert g["p_dispersion"][worst] < 0.01
    assert outside > 0.5
    assert all(p >= 0.01 / G for _, p in others)
    assert ("pollster", g["labels"][worst], "dispersion") in [f[:3] for f in ck.flag(0.01, 5)]


@pytest.mark.parametrize("name", VARIANTS)
def test_clean_fits_raise_no_flag(checks, name):
    ck = checks[name]
    for gname, g in ck.groups.items():
        G, p = len(g["labels"]), _p_values(g)
        print(f"{name} {gname}: {p.shape[1]} groups of five or more polls, p in [{p.min():.4f}, {p.max():.4f}]" if p.size else f"{name} {gname}: no group of five or more polls")
        assert ((p > 0.001 / G) & (p < 1.0 - 0.001 / G)).all(), (gname, p)
    ks = stats.kstest(ck.pit(loo=True, seed=1), "uniform").pvalue
    print(f"{name}: KS p-value of the randomised LOO-PIT {ks:.4f}; histogram {np.round(ck.pit_hist(10), 3).tolist()}; coverage 50 % {ck.coverage(0.5):.3f}, 95 % {ck.coverage(0.95):.3f}")
    assert ks > 0.001
    assert abs(ck.pit_hist(10).sum() - 1.0) < 1e-12


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_before_any_kernel(fits):
    import torch
    data = synthetic.small("full")
    m = Handle(data, "full", chains=2, num_warmup=5, num_samples=5, cus_per_chain=1, twin=0)
    ys, yn = np.asarray(data["n_democrat_state"])[None], np.asarray(data["n_democrat_national"])[None]
    m.set_datasets(np.repeat(ys, 2, 0), np.repeat(yn, 2, 0))
    m.init()
    m.run(10)
    for call in (lambda: m.ppc(), lambda: m.poll_rep_device(0, 1)):
        with pytest.raises(PotusError, match="error 4.*slice the chains per data set"):
            call()
    m.close()
    e = Handle(data, "full", chains=2, num_warmup=5, num_samples=3, cus_per_chain=1, twin=0)
    e.init()
    e.run(8)
    with pytest.raises(PotusError, match="error 4.*at least four"):
        e.ppc()
    e.close()
    h = fits["full"]
    N = h.n_polls
    with pytest.raises(PotusError, match="error 1.*rep = 1024"):
        h.ppc(rep=1024)
    with pytest.raises(PotusError, match="error 1.*listed twice"):
        ppc.check([h, h])
    with pytest.raises(PotusError, match="error 1.*another posterior"):
        ppc.check([h, fits["no_mode_adjustment"]])
    with pytest.raises(PotusError, match="error 1.*label 3"):
        ppc.check(h, by=(), groups={"mine": (np.full(N, 3), ["a", "b", "c"])})
    with pytest.raises(PotusError, match="error 1.*label -2"):
        ppc.check(h, by=(), groups={"mine": (np.full(N, -2), ["a", "b", "c"])})
    ids = (C.c_int * 1)(h.h)
    pit, k = np.zeros((N, 4)), np.zeros(N)
    assert h.L.potus_ppc(ids, 1, 1, 0, None, 0, None, None, k.ctypes.data_as(DP), None, None) == 1
    assert h.L.potus_ppc(ids, 1, 1, 0, None, 0, None, pit.ctypes.data_as(DP), None, None, None) == 1
    assert h.L.potus_ppc(ids, 1, 2, 0, None, 0, None, pit.ctypes.data_as(DP), k.ctypes.data_as(DP), None, None) == 1
    assert not pit.any() and not k.any()
    t = torch.zeros((2, 2, 8), dtype=torch.float64, device="cuda:0")
    p, host = C.c_void_p(t.data_ptr()), np.zeros(32)
    hp = C.c_void_p(host.ctypes.data)
    for b0, b1, ig, rep in ((-1, 1, 1, 0), (0, N + 1, 1, 0), (2, 2, 1, 0), (0, 1, 2, 0), (0, 1, 1, -1), (0, 1, 1, 1024)):
        assert h.L.potus_poll_rep_device(h.h, b0, b1, ig, rep, p) == 1
    assert h.L.potus_poll_rep_device(h.h, 0, 1, 1, 0, hp) == 1 and h.L.potus_poll_rep_device(h.h, 0, 1, 1, 0, None) == 4
    d = host.ctypes.data_as(DP)
    out = np.zeros(4)
    assert h.L.potus_ppc_pit_device(0, hp, d, None, 2, 2, 8, out.ctypes.data_as(DP)) == 1            # blocks that are not memory of the device
    assert h.L.potus_ppc_pit_device(0, p, d, hp, 2, 2, 8, out.ctypes.data_as(DP)) == 1
    assert h.L.potus_ppc_pit_device(0, p, d, None, 2, 2, 3, out.ctypes.data_as(DP)) == 1             # fewer than four draws per chain
    lab, cnt, go = np.zeros(2, np.int32), np.zeros(1, np.int64), np.zeros(18)
    for args in ((hp, p, p, None), (p, hp, p, None), (p, p, hp, None), (p, p, p, hp)):
        assert h.L.potus_ppc_groups_device(0, args[0], args[1], args[2], d, d, lab.ctypes.data_as(IP), 1, 2, 2, 8, args[3], 3, go.ctypes.data_as(DP), cnt.ctypes.data_as(LLP)) == 1
    assert not out.any() and not go.any()
