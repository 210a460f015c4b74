"""Simulation-based calibration on the MI355X: the prior simulator (k_simulate_prior), potus_constrain, many data sets in one handle
(k_init_ds / k_run_ds), the device ranks (k_sbc_ranks) and SBC itself, with a negative control that shows the check has power."""
import ctypes as C
import time

import numpy as np
import pytest
from scipy import stats

from oracle_lib import OracleModel, lib as oracle_lib
from us_potus_model_amd import _abi, sbc
from us_potus_model_amd.sampler import Handle, PotusError

pytestmark = pytest.mark.gpu
SEED = 20250611


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """sbc.run takes R-hat through torch tensors: torch's GPU runtime comes up before this module's first library call (as bench.py does)."""
    import torch
    torch.cuda.init()


def _normal_pairs(seed, chain, aux, n):
    L = oracle_lib()
    a, b = C.c_double(), C.c_double()
    out = np.zeros(2 * n)
    for j in range(n):
        L.oracle_rng_normal_pair(seed, chain, 0, 6, aux, j, C.byref(a), C.byref(b))
        out[2 * j], out[2 * j + 1] = a.value, b.value
    return out


def _expected_prior_point(seed, sim, D, o_rho):
    """potus_hmc.h's counter mapping restated with the oracle's Philox: standard normals, then rho_e_bias by rejection."""
    q = _normal_pairs(seed, sim + 1, 0, (D + 1) // 2)[:D]
    if o_rho is not None:
        L = oracle_lib()
        a, b = C.c_double(), C.c_double()
        for att in range(256):
            L.oracle_rng_normal_pair(seed, sim + 1, 0, 6, 1, att, C.byref(a), C.byref(b))
            r = 0.7 + 0.1 * a.value
            if 0 < r < 1:
                break
        q[o_rho] = np.log(r / (1 - r))
    return q


def _small_n_design(data):
    """synthetic.small with n_two_share in 3..19: every outcome goes through the inversion branch (n min(p, 1 - p) <= 9.5 < 10)."""
    rng = np.random.default_rng(5)
    d = dict(data)
    for k in ("state", "national"):
        n = rng.integers(3, 20, len(data[f"n_two_share_{k}"]))
        d[f"n_two_share_{k}"], d[f"n_democrat_{k}"] = n, n // 2
    return d


def _pit_pvalue(data, variant, q, ys, yn, seed=0):
    """Randomised PIT of every (sim, poll) outcome under p = inv_logit(logit_pi) from the oracle's write_array(q): uniform if exact."""
    m = OracleModel(data, variant)
    lay, _ = _abi.column_layout(data, variant)
    a_s, b_s, _ = lay["logit_pi_democrat_state"]
    a_n, b_n, _ = lay["logit_pi_democrat_national"]
    ns, nn = np.asarray(data["n_two_share_state"]), np.asarray(data["n_two_share_national"])
    rng = np.random.default_rng(seed)
    us = []
    for i in range(q.shape[0]):
        row = np.concatenate([np.full(7, np.nan), m.write_array(q[i])])
        for y, n, eta in ((ys[i], ns, row[a_s:b_s]), (yn[i], nn, row[a_n:b_n])):
            p = 1 / (1 + np.exp(-eta))
            lo, hi = stats.binom.cdf(y - 1, n, p), stats.binom.cdf(y, n, p)
            us.append(lo + rng.random(len(y)) * (hi - lo))
    u = np.concatenate(us)
    return stats.chisquare(np.histogram(u, bins=20, range=(0, 1))[0]).pvalue


@pytest.mark.parametrize("name", ["small_full", "small_nomode", "2016"])
def test_prior_simulator(cases, name):
    data, variant = cases[name]
    h = Handle(data, variant, chains=1, num_warmup=0, num_samples=0)
    q8, ys8, yn8 = h.simulate_prior(SEED, 8)
    q2, ys2, yn2 = h.simulate_prior(SEED, 2, 0)
    q6, ys6, yn6 = h.simulate_prior(SEED, 6, 2)
    assert np.concatenate([q2, q6]).tobytes() == q8.tobytes()
    assert np.concatenate([ys2, ys6]).tobytes() == ys8.tobytes() and np.concatenate([yn2, yn6]).tobytes() == yn8.tobytes()
    lay, _ = _abi.column_layout(data, variant)
    o_rho = lay["rho_e_bias"][0] - 7 if "rho_e_bias" in lay else None
    for i in range(8):
        e = _expected_prior_point(SEED, i, h.D, o_rho)
        keep = np.ones(h.D, bool)
        if o_rho is not None:
            keep[o_rho] = False
            assert abs(q8[i, o_rho] - e[o_rho]) <= 1e-12 * max(1.0, abs(e[o_rho]))
        np.testing.assert_allclose(q8[i, keep], e[keep], rtol=1e-14, atol=1e-300)
    ns, nn = np.asarray(data["n_two_share_state"]), np.asarray(data["n_two_share_national"])
    assert (ys8 >= 0).all() and (ys8 <= ns).all() and (yn8 >= 0).all() and (yn8 <= nn).all()
    h.close()


@pytest.mark.parametrize("which", ["inversion", "btrs"])
def test_simulated_outcomes_follow_the_binomial(cases, which):
    """Randomised PIT of the outcomes under the oracle's logit_pi: n_two_share 3..19 exercises inversion, 2016 (n in the hundreds) BTRS."""
    if which == "inversion":
        data, variant = _small_n_design(cases["small_full"][0]), "full"
        n_sims = 200
    else:
        data, variant = cases["2016"]
        n_sims = 6
    h = Handle(data, variant, chains=1, num_warmup=0, num_samples=0)
    q, ys, yn = h.simulate_prior(SEED + 1, n_sims)
    h.close()
    p = _pit_pvalue(data, variant, q, ys, yn)
    assert p > 1e-3, p


@pytest.mark.parametrize("name", ["small_full", "small_nomode"])
def test_constrain_matches_the_oracle_write_array(cases, name):
    data, variant = cases[name]
    h = Handle(data, variant, chains=1, num_warmup=0, num_samples=0)
    q, _, _ = h.simulate_prior(SEED, 4)
    rows = h.constrain(q, 0, h.n_cols)
    assert np.isnan(rows[:, :7]).all()
    m = OracleModel(data, variant)
    for i in range(4):
        ref = m.write_array(q[i])
        assert (np.abs(rows[i, 7:] - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref))).all()
    mid = h.constrain(q, 20, 30)
    assert mid.tobytes() == np.ascontiguousarray(rows[:, 20:30]).tobytes()
    h.close()


NW, NS = 150, 50


@pytest.fixture(scope="module", params=["small_full", "small_nomode"])
def many(request, cases):
    """4 data sets x 2 chains of synthetic.small in one handle, 150 + 50 transitions (across the window ends)."""
    data, variant = cases[request.param]
    sim = Handle(data, variant, chains=1, num_warmup=0, num_samples=0)
    q, ys, yn = sim.simulate_prior(SEED + 2, 4)
    sim.close()
    h = Handle(data, variant, chains=8, num_warmup=NW, num_samples=NS, seed=1843, cus_per_chain=1, twin=0)
    h.set_datasets(ys, yn)
    h.init()
    h.run(NW + NS)
    yield dict(h=h, data=data, variant=variant, q=q, ys=ys, yn=yn)
    h.close()


def test_many_datasets_equal_single_handles_byte_for_byte(many):
    h, data, variant = many["h"], many["data"], many["variant"]
    d_many = h.draws()
    eps_many, minv_many = h.adaptation()
    assert h.chain_status()[0] == [0] * 8
    for c in range(8):
        d1 = dict(data, n_democrat_state=many["ys"][c // 2], n_democrat_national=many["yn"][c // 2])
        g = Handle(d1, variant, chains=1, num_warmup=NW, num_samples=NS, seed=1843, cus_per_chain=1, twin=0, chain_id_offset=c)
        g.init()
        g.run(NW + NS)
        eps, minv = g.adaptation()
        assert g.draws()[0].tobytes() == d_many[c].tobytes(), c
        assert eps.tobytes() == eps_many[c:c + 1].tobytes() and minv.tobytes() == minv_many[c:c + 1].tobytes(), c
        g.close()
    # the data sets differ, and so do their chains
    assert d_many[0].tobytes() != d_many[2].tobytes()


def test_set_datasets_and_set_datasets_ex_give_the_same_draws(cases):
    """The plain call is the _ex call with only the outcomes given: the same models byte for byte, hence the same chains."""
    data, variant = cases["small_full"]
    ys, yn = np.asarray(data["n_democrat_state"], np.int32), np.asarray(data["n_democrat_national"], np.int32)
    ys, yn = np.stack([ys, ys // 2]), np.stack([yn, yn // 2])
    draws = []
    for ex in (False, True):
        g = Handle(data, variant, chains=4, num_warmup=20, num_samples=10, seed=1843, cus_per_chain=1, twin=0)
        if ex:
            g.set_datasets_ex(n_democrat_state=ys, n_democrat_national=yn)
        else:
            g.set_datasets(ys, yn)
        g.init()
        g.run(30)
        draws.append(g.draws())
        g.close()
    assert draws[0].shape[1] == 10 and np.isfinite(draws[0]).all()
    assert np.array_equal(draws[0], draws[1])
    assert not np.array_equal(draws[0][0], draws[0][2])     # the two data sets differ, and so do their chains


def test_many_datasets_refusals(many, cases, tmp_path):
    data, variant = cases["small_full"]
    ys, yn = np.asarray(data["n_democrat_state"])[None], np.asarray(data["n_democrat_national"])[None]

    def refused(match, **opts):
        g = Handle(data, variant, num_warmup=10, num_samples=10, **opts)
        try:
            with pytest.raises(PotusError, match=match):
                g.set_datasets(np.repeat(ys, 2, 0), np.repeat(yn, 2, 0))
        finally:
            g.close()
    refused("not a multiple", chains=3, cus_per_chain=1, twin=0)
    refused("one workgroup per chain", chains=2, cus_per_chain=2, twin=0)
    refused("one workgroup per chain", chains=2, cus_per_chain=1, twin=1)
    refused("dense metric", chains=2, metric=_abi.METRIC_DENSE)
    g = Handle(data, variant, chains=2, num_warmup=10, num_samples=10, cus_per_chain=1, twin=0)
    g.init()
    with pytest.raises(PotusError, match="already initialised"):
        g.set_datasets(np.repeat(ys, 2, 0), np.repeat(yn, 2, 0))
    g.close()
    g = Handle(data, variant, chains=2, num_warmup=10, num_samples=10, cus_per_chain=1, twin=0)
    bad = np.repeat(ys, 2, 0).copy()
    bad[1, 3] = int(data["n_two_share_state"][3]) + 1
    with pytest.raises(PotusError, match=r"potus_set_datasets: data set 2: n_democrat_state\[4\]"):   # names the function that was called
        g.set_datasets(bad, np.repeat(yn, 2, 0))
    g.set_datasets(np.repeat(ys, 2, 0), np.repeat(yn, 2, 0))                    # ... and the refusal left nothing behind
    assert g.n_datasets == 2
    g.close()
    # calls that pool all chains of the handle refuse and point to per-data-set slicing
    from us_potus_model_amd import sampler
    h = many["h"]
    for call in (lambda: h.posterior_summary(np.ones(int(many["data"]["S"]))), lambda: sampler.device_diagnostics([h], 0, 8),
                 lambda: sampler.check_convergence([h]), lambda: h.write_stan_csv(tmp_path)):
        with pytest.raises(PotusError, match="slice the chains per data set"):
            call()
    out, rows = np.zeros(8 * NS), C.c_longlong()
    ids = (C.c_int * 1)(h.h)
    assert h.L.potus_extract_matrix(ids, 1, 7, 8, out.ctypes.data_as(C.POINTER(C.c_double)), C.c_longlong(8 * NS), C.byref(rows)) == 4   # POTUS_ERR_STATE


@pytest.mark.parametrize("thin", [1, 3, 7])
def test_device_ranks_equal_a_numpy_count(many, thin):
    h, data, variant = many["h"], many["data"], many["variant"]
    a, e = 7 + h.D, h.n_cols
    truth = h.constrain(many["q"], a, e)
    rows = h.write_array(a, e, NS)                                   # [draw, chain, col]: what k_write_array builds, bit for bit
    truth[0] = rows[0, 0]                                            # ties: data set 0's truth is one of its own compared draws
    less, equal, L = h.sbc_ranks(truth, a, e, thin)
    assert L == 2 * len(range(0, NS, thin))
    for ds in range(4):
        x = rows[::thin, 2 * ds:2 * ds + 2].reshape(-1, e - a)
        assert np.array_equal(less[ds], (x < truth[ds]).sum(0)), ds
        assert np.array_equal(equal[ds], (x == truth[ds]).sum(0)), ds
    assert (equal[0] >= 1).all()
    # the rows themselves are the oracle's constrained rows
    m = OracleModel(data, variant)
    d = h.draws()
    ref = m.write_array(d[3, NS - 1, 7:])[h.D:]
    assert (np.abs(rows[NS - 1, 3] - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref))).all()


# SBC proper.  synthetic.small, 256 replicates x 2 chains in ONE handle; warm-up 300, 500 draws kept, every 10th compared: L = 100.
# Measured on the MI355X (32 replicates x 2 chains of each variant, every default column): the bulk ESS of a replicate's 100 thinned
# draws has a median of 88-111 per column, so the compared draws are close to independent.
SBC_SIMS, SBC_NW, SBC_NS, SBC_THIN = 256, 300, 500, 10


@pytest.mark.parametrize("name", ["small_full", "small_nomode"])
def test_sbc_ranks_are_uniform(cases, name):
    data, variant = cases[name]
    t0 = time.perf_counter()
    r = sbc.run(data, variant, n_sims=SBC_SIMS, chains_per_sim=2, num_warmup=SBC_NW, num_samples=SBC_NS, thin=SBC_THIN, seed=SEED)
    assert r["batched"] and r["L"] == 100
    ok = ~r["failed"]
    assert ok.sum() >= SBC_SIMS - 2, r["failed"].sum()
    p = sbc.uniformity(r["ranks"][ok], r["L"], bins=20)
    print(f"{name}: {time.perf_counter() - t0:.1f} s, {r['leapfrogs']} leapfrogs, failed {int(r['failed'].sum())}, "
          f"max R-hat {np.nanmax(r['rhat']):.3f}, divergent {int(r['divergent'].sum())}")
    for c, pv in zip(r["columns"], p):
        print(f"  {c:32s} p = {pv:.4f}")
    assert (p > 0.001 / len(p)).all(), dict(zip(r["columns"], p))


def test_sbc_has_power_against_a_wrong_prior(cases):
    """Negative control: simulate with sigma_c three times the model's, fit with the model's: the house effects' ranks are far from uniform."""
    data, variant = cases["small_full"]
    wide = dict(data, sigma_c=3 * float(data["sigma_c"]))
    cols = ["mu_c.1", "mu_c.2", "mu_c.9", "mu_b.1.24"]
    r = sbc.run(data, variant, n_sims=SBC_SIMS, chains_per_sim=2, num_warmup=SBC_NW, num_samples=SBC_NS, thin=SBC_THIN, seed=SEED,
                columns=cols, sim_data=wide)
    p = sbc.uniformity(r["ranks"][~r["failed"]], r["L"], bins=20)
    print(dict(zip(cols, p)))
    assert (p[:3] < 1e-6).all(), dict(zip(cols, p))
