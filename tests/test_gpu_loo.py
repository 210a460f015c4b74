"""PSIS-LOO on the MI355X (potus_loo.hpp): per-poll log-likelihoods against scipy, their tie to the model's log density, PSIS against
the numpy restatement (tests/psis_ref.py) on every branch, pooling over handles, refusals, the .C() path, exact LOO by refitting, and a
comparison that must prefer the model that generated the data."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats
from scipy.special import logsumexp

import psis_ref
from conftest import second_device
from us_potus_model_amd import loo as loo_mod, synthetic
from us_potus_model_amd.sampler import Handle, PotusError, run_many

pytestmark = pytest.mark.gpu
SEED = 4242
NW, NS = 300, 500
VARIANTS = ("full", "no_mode_adjustment")
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def _fit(data, variant, chains=4, **kw):
    h = Handle(data, variant, chains=chains, num_warmup=NW, num_samples=NS, seed=SEED, cus_per_chain=1, twin=0, **kw)
    h.init()
    h.run(NW + NS)
    return h


@pytest.fixture(scope="module")
def fits():
    out = {v: _fit(synthetic.small(v), v) for v in VARIANTS}
    yield out
    for h in out.values():
        h.close()


def _polls(data):
    """(y, n, sigma) per poll: state polls, then national polls."""
    y, n = (a.astype(float) for a in loo_mod.poll_vectors(data))
    Ns, Nn = int(data["N_state_polls"]), int(data["N_national_polls"])
    sig = np.concatenate([np.full(Ns, float(data["sigma_measure_noise_state"])), np.full(Nn, float(data["sigma_measure_noise_national"]))])
    return y, n, sig


def _log_lik(h, integrate):
    import torch
    t = torch.empty((h.n_polls, h.opts.chains, h.post_warmup_saved()), dtype=torch.float64, device=f"cuda:{h.opts.device}")
    h.log_lik_device(0, h.n_polls, t, integrate=integrate)
    return t.cpu().numpy()


def _columns(h, *names):
    """[column][chain][draw] of the named output blocks, one after the other."""
    n = h.draws_saved()
    return np.concatenate([h.write_array(h.layout[k][0], h.layout[k][1], n).transpose(2, 1, 0) for k in names])


def _close(a, b, tol=1e-8):
    a, b = np.asarray(a), np.asarray(b)
    assert np.array_equal(np.isinf(a), np.isinf(b)) and not np.isnan(a).any()
    fin = np.isfinite(b)
    err = np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))
    assert err.max() <= tol, float(err.max())


@pytest.mark.parametrize("via", ["log_lik", "cv_log_lik"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_plain_log_lik_equals_scipy_on_the_logit_pi_columns(fits, variant, via):
    """The three users of the row's poll predictor agree on the row's column blocks: the logit_pi columns are wa_build_row's, the
    log-likelihoods k_loo_loglik's (via = log_lik) or k_cv_loglik's (cv_log_lik: the plain handle as one data set that holds every poll out).
    On the host the noise term comes out of logit_pi and goes back in: eta = logit_pi - raw_measure_noise sigma, x = eta + sigma z."""
    h = fits[variant]
    y, n, sig = _polls(h.data)
    Ns, Nn = int(h.data["N_state_polls"]), int(h.data["N_national_polls"])
    assert Ns > 0 and Nn > 0 and len(y) == Ns + Nn                       # state polls and national polls are both compared
    z = _columns(h, "raw_measure_noise_state", "raw_measure_noise_national")
    eta = _columns(h, "logit_pi_democrat_state", "logit_pi_democrat_national") - sig[:, None, None] * z
    ref = stats.binom.logpmf(y[:, None, None], n[:, None, None], 1.0 / (1.0 + np.exp(-(eta + sig[:, None, None] * z))))
    if via == "log_lik":
        ll = _log_lik(h, False)
    else:
        ll = h.cv_log_lik_device(np.ones((1, Ns)), np.ones((1, Nn)), integrate=False).cpu().numpy().reshape(ref.shape)
    err = np.abs(ll - ref)
    print(f"{variant} {via}: largest |device - scipy| state polls {err[:Ns].max():.2e}, national polls {err[Ns:].max():.2e}")
    assert err[:Ns].max() < 1e-9 and err[Ns:].max() < 1e-9


@pytest.mark.parametrize("variant", VARIANTS)
def test_integrated_log_lik_equals_quadrature(fits, variant):
    h = fits[variant]
    y, n, sig = _polls(h.data)
    eta = _columns(h, "logit_pi_democrat_state", "logit_pi_democrat_national") - \
        sig[:, None, None] * _columns(h, "raw_measure_noise_state", "raw_measure_noise_national")
    ll = _log_lik(h, True)
    rng = np.random.default_rng(1)
    Ns = int(h.data["N_state_polls"])
    polls = np.concatenate([rng.integers(0, len(y), 150), np.arange(Ns, len(y)), np.full(10, int(np.argmax(n)))])   # national polls, the largest n
    worst = 0.0
    for i in polls:
        c, d = rng.integers(0, ll.shape[1]), rng.integers(0, ll.shape[2])
        worst = max(worst, abs(ll[i, c, d] - psis_ref.log_lik_quad(y[i], n[i], eta[i, c, d], sig[i])))
    print(f"{variant}: largest |device - quad| over {len(polls)} (draw, poll) pairs: {worst:.2e}")
    assert worst < 1e-9


@pytest.mark.parametrize("variant", VARIANTS)
def test_plain_log_lik_sums_to_the_model_pass(fits, variant):
    h = fits[variant]
    d0 = dict(h.data)
    for k in ("n_democrat_state", "n_two_share_state", "n_democrat_national", "n_two_share_national"):
        d0[k] = np.zeros_like(np.asarray(h.data[k]))
    h0 = Handle(d0, variant, chains=1, num_warmup=1, num_samples=1)
    y, n, _ = _polls(h.data)
    lc = psis_ref.lchoose(n, y).sum()
    ll = _log_lik(h, False)
    dr = h.draws()
    for c, i in ((0, 0), (1, 37), (3, NS - 1)):
        q = dr[c, i, 7:]
        a = h.log_prob_grad(q)[0][0] - h0.log_prob_grad(q)[0][0]
        b = ll[:, c, i].sum() - lc
        assert abs(a - b) <= 1e-9 * abs(a), (a, b)
    h0.close()


@pytest.mark.parametrize("integrate", [False, True])
def test_psis_matches_the_restatement_and_repeats_bytes(fits, integrate):
    h = fits["full"]
    ref = psis_ref.loo_pointwise(_log_lik(h, integrate))
    r = loo_mod.loo([h], integrate=integrate)
    _close(r.pointwise, ref)
    _close(r.estimates, psis_ref.estimates(ref))
    r2 = loo_mod.loo([h], integrate=integrate)
    assert r2.pointwise.tobytes() == r.pointwise.tobytes() and r2.estimates.tobytes() == r.estimates.tobytes()
    print(f"integrate={integrate}: {r.pareto_k_table()}")


def test_psis_branches_on_built_blocks():
    import torch
    rng = np.random.default_rng(3)
    base = rng.normal(-3, 0.7, (6, 4, 250)) + 0.3 * rng.standard_t(3, (6, 4, 250))
    x = base[4].reshape(-1)
    x[x < np.quantile(x, 0.3)] = np.quantile(x, 0.3)      # poll 4: the largest ratios are one value
    base[5] = -1.25                                        # poll 5: identical log-likelihoods
    S = 1000
    blk = torch.tensor(base, device="cuda:0")
    for r_eff in (None, np.full(6, 1e-6), np.full(6, float(S))):   # computed; tail = 0.2 S; tail shorter than 5
        got = loo_mod.loo_of_block(blk, r_eff=r_eff)
        ref = psis_ref.loo_pointwise(base, r_eff)
        _close(got.pointwise, ref)
        _close(got.estimates, psis_ref.estimates(ref))
        if r_eff is not None and r_eff[0] < 1:
            assert psis_ref.tail_length(r_eff[0], S) == 200 and np.isfinite(got.pareto_k[:4]).all()
        if r_eff is not None and r_eff[0] == S:
            assert np.isinf(got.pareto_k).all()
    assert np.isinf(got.pareto_k[4]) and np.isinf(got.pareto_k[5]) and abs(got.pointwise[5, 0] + 1.25) < 1e-12
    # more than one sorted run: 16 chains x 1000 draws > 8192
    big = rng.normal(-3, 0.7, (3, 16, 1000)) + 0.3 * rng.standard_t(3, (3, 16, 1000))
    _close(loo_mod.loo_of_block(torch.tensor(big, device="cuda:0")).pointwise, psis_ref.loo_pointwise(big))


def test_pooled_handles_give_the_bytes_of_one_handle(fits):
    h = fits["full"]
    d = synthetic.small("full")
    a = Handle(d, "full", chains=2, num_warmup=NW, num_samples=NS, seed=SEED, cus_per_chain=1, twin=0)
    b = Handle(d, "full", chains=2, chain_id_offset=2, device=second_device(), num_warmup=NW, num_samples=NS, seed=SEED, cus_per_chain=1, twin=0)
    a.init()
    b.init()
    run_many([a, b], NW + NS)
    assert np.concatenate([a.draws(), b.draws()]).tobytes() == h.draws().tobytes()
    for integrate in (False, True):
        one, two = loo_mod.loo([h], integrate), loo_mod.loo([a, b], integrate)
        assert one.pointwise.tobytes() == two.pointwise.tobytes() and one.estimates.tobytes() == two.estimates.tobytes()
    a.close()
    b.close()


def test_refusals(fits):
    import torch
    h, g = fits["full"], fits["no_mode_adjustment"]
    data = synthetic.small("full")
    with pytest.raises(PotusError, match="another posterior"):
        loo_mod.loo([h, g])
    o = Handle(dict(data, n_democrat_state=np.asarray(data["n_democrat_state"]) // 2), "full", chains=2, num_warmup=5, num_samples=5,
               cus_per_chain=1, twin=0)
    o.init()
    o.run(10)
    with pytest.raises(PotusError, match="another posterior"):
        loo_mod.loo([h, o])
    with pytest.raises(PotusError, match="listed twice"):
        loo_mod.loo([h, h])
    e = Handle(data, "full", chains=2, num_warmup=5, num_samples=5, cus_per_chain=1, twin=0)
    e.init()
    with pytest.raises(PotusError, match="at least four"):
        loo_mod.loo([e])
    t = torch.zeros(8, dtype=torch.float64, device="cuda:0")
    ptr = C.c_void_p(t.data_ptr())
    assert h.L.potus_log_lik_device(e.h, 0, 1, 1, ptr) == 4                      # no post-warm-up draws
    Np = h.n_polls
    for b0, b1 in ((-1, 3), (0, Np + 1), (3, 3)):
        assert h.L.potus_log_lik_device(h.h, b0, b1, 1, ptr) == 1
    assert h.L.potus_log_lik_device(h.h, 0, 1, 2, ptr) == 1
    pw, est = np.zeros((Np, 5)), np.zeros(6)
    ids = (C.c_int * 1)(h.h)
    assert h.L.potus_loo(ids, 1, 2, None, pw.ctypes.data_as(DP), est.ctypes.data_as(DP)) == 1
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(PotusError, match="r_eff"):
            loo_mod.loo([h], r_eff=np.where(np.arange(Np) == 3, bad, 1.0))
    m = Handle(data, "full", chains=2, num_warmup=5, num_samples=5, cus_per_chain=1, twin=0)
    ys, yn = np.asarray(data["n_democrat_state"])[None], np.asarray(data["n_democrat_national"])[None]
    m.set_datasets(np.repeat(ys, 2, 0), np.repeat(yn, 2, 0))
    m.init()
    m.run(10)
    with pytest.raises(PotusError, match="slice the chains per data set"):
        loo_mod.loo([m])
    assert h.L.potus_log_lik_device(m.h, 0, 1, 1, ptr) == 4
    for x in (o, e, m):
        x.close()


def test_r_entry_point_gives_the_bytes_of_potus_loo(fits):
    h = fits["full"]
    ref = loo_mod.loo([h], integrate=True)
    f = h.L.potus_R_loo
    for given in (0, 1):
        pw, est, st = np.zeros(h.n_polls * 5), np.zeros(6), C.c_int(-1)
        re = np.ascontiguousarray(ref.r_eff) if given else np.zeros(1)
        f((C.c_int * 1)(h.h), C.byref(C.c_int(1)), (C.c_int * 2)(1, given), re.ctypes.data_as(DP), pw.ctypes.data_as(DP), est.ctypes.data_as(DP),
          C.byref(st))
        assert st.value == 0
        assert pw.tobytes() == ref.pointwise.tobytes() and est.tobytes() == ref.estimates.tobytes()


def _drop_state_poll(data, i):
    d = dict(data, N_state_polls=int(data["N_state_polls"]) - 1)
    for k in ("state", "day_state", "poll_state", "poll_mode_state", "poll_pop_state", "n_democrat_state", "n_two_share_state", "unadjusted_state"):
        if k in d:
            d[k] = np.delete(np.asarray(data[k]), i)
    return d


def _state_poll_eta(g, data, i):
    """eta of state poll i (without its noise term) at every draw of fit g, from g's output columns: [chains, draws]."""
    S = int(data["S"])
    s, t = int(data["state"][i]) - 1, int(data["day_state"][i]) - 1
    n = g.draws_saved()

    def col(name, off):
        c = g.layout[name][0] + off
        return g.write_array(c, c + 1, n)[:, :, 0].T
    eta = col("mu_b", s + S * t) + col("mu_c", int(data["poll_state"][i]) - 1) + col("polling_bias", s)
    return eta + col("mu_m", int(data["poll_mode_state"][i]) - 1) + col("mu_pop", int(data["poll_pop_state"][i]) - 1) + \
        float(data["unadjusted_state"][i]) * col("e_bias", t)


def test_exact_loo_by_refitting_agrees(fits):
    h = fits["full"]
    data = h.data
    r = loo_mod.loo([h], integrate=True)
    ll = _log_lik(h, True)
    y, n, sig = _polls(data)
    cand = [i for i in range(int(data["N_state_polls"])) if r.pareto_k[i] < 0.5]
    for i in np.random.default_rng(8).choice(cand, 3, replace=False):
        g = _fit(_drop_state_poll(data, i), "full")
        l = psis_ref.log_lik_integrated(y[i], n[i], _state_poll_eta(g, data, i), sig[i])
        g.close()
        exact = logsumexp(l) - np.log(l.size)
        w = np.exp(l - l.max())
        var_exact = w.var() / (w.mean() ** 2 * l.size * psis_ref.relative_eff(l))          # delta method
        lw, _ = psis_ref.psis(ll[i], r.r_eff[i])
        p = np.exp(ll[i].reshape(-1) - ll[i].max())
        W = np.exp(lw)
        E = (W * p).sum()
        var_psis = (W * W * (p / E - 1) ** 2).sum() / r.r_eff[i]
        tol = 4 * np.sqrt(var_exact + var_psis)
        print(f"poll {i}: exact {exact:.4f}, PSIS {r.pointwise[i, 0]:.4f}, k {r.pareto_k[i]:.2f}, tolerance {tol:.4f}")
        assert tol < 0.1
        assert abs(exact - r.pointwise[i, 0]) < tol


def test_loo_compare_prefers_the_model_with_mode_effects():
    data = synthetic.small("full")
    g = Handle(data, "full", chains=1, num_warmup=1, num_samples=1)
    lay = g.layout
    rng = np.random.default_rng(17)
    q = np.zeros(g.D)
    o = lay["raw_mu_m"][0] - 7
    q[o:o + 3] = np.array([0.1, -0.1, 0.0]) / float(data["sigma_m"])        # mode effects of +-0.1 on the logit scale
    for k in ("raw_measure_noise_state", "raw_measure_noise_national"):
        a, b, _ = lay[k]
        q[a - 7:b - 7] = rng.normal(size=b - a)
    lp = g.constrain(q[None], lay["logit_pi_democrat_state"][0], lay["logit_pi_democrat_national"][1])[0]
    g.close()
    _, n, _ = _polls(data)
    ys = rng.binomial(n.astype(np.int64), 1.0 / (1.0 + np.exp(-lp))).astype(np.int32)
    Ns = int(data["N_state_polls"])
    sim = dict(data, n_democrat_state=ys[:Ns], n_democrat_national=ys[Ns:])
    loos = []
    for v in VARIANTS:
        f = _fit(sim, v)
        loos.append(loo_mod.loo([f], name=v))
        f.close()
    rows = loo_mod.loo_compare(*loos)
    print(loo_mod.format_compare(rows))
    assert rows[0]["name"] == "full" and -rows[1]["elpd_diff"] > 4 * rows[1]["se_diff"]
