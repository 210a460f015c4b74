"""Prior sensitivity by refit on the MI355X: prior settings as the data sets of one handle (potus_set_datasets_grid) against stand-alone
handles on each setting's data, the calls that take such a handle (scores, log-likelihoods, modes) against the same, and the distance
kernel (k_sg_distance, potus_sens.hpp) against the numpy restatement in tests/sens_ref.py at the edges of its sizes."""
import numpy as np
import pytest

import sens_ref
from us_potus_model_amd import _abi, loo, sensitivity, synthetic, timeline
from us_potus_model_amd.sampler import N_SCALES, SCALE_NAMES, Handle, PotusError, ecdf_distance_device

pytestmark = pytest.mark.gpu
NW, NS, CPS = 30, 20, 2
EV = np.array([100, 90, 80, 70, 60, 138])
OPTS = dict(seed=1843, cus_per_chain=1, twin=0)
VARIANTS = ("full", "no_mode_adjustment")
ALL = 1 + N_SCALES                              # the setting with all nine scales changed, a poll mask and a prior of its own


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """Blocks go in and come back as torch tensors: torch's GPU runtime comes up before this module's first library call."""
    import torch
    torch.cuda.init()


def bytes_design(variant):
    """synthetic.small: the baseline, each of the nine scales x 1.5 alone, and one setting with all nine changed together, every third state
    poll and every second national poll unseen, and a mu_b_prior of its own."""
    data = synthetic.small(variant)
    d = sensitivity.grid(data, {name: [1.5] for name in SCALE_NAMES}, null=False)
    n, S = ALL + 1, int(data["S"])
    f = np.linspace(0.6, 1.7, N_SCALES)
    d["factors"] = np.vstack([d["factors"], f])
    d["scales"] = np.vstack([d["scales"], f * sensitivity.scales_of(data)])
    d["labels"] = d["labels"] + ["all nine"]
    d["run_dates"] = list(d["labels"])
    d["varied"] = np.append(d["varied"], -1)
    ks, kn = np.ones(int(data["N_state_polls"]), bool), np.ones(int(data["N_national_polls"]), bool)
    ks[::3] = False
    kn[::2] = False
    d["keep_state"], d["keep_national"] = np.vstack([d["keep_state"], ks]), np.vstack([d["keep_national"], kn])
    prior = np.tile(np.asarray(data["mu_b_prior"], dtype=np.float64), (n, 1))
    prior[ALL] += np.linspace(-0.3, 0.4, S)
    d["mu_b_prior"] = prior
    return d


def run(design, variant, chains_per_setting, nw, ns, q0=None):
    n = design["scales"].shape[0]
    h = Handle(design["data"], variant, chains=n * chains_per_setting, num_warmup=nw, num_samples=ns, **OPTS)
    timeline.set_design(h, design)
    h.init(q0)
    h.run(nw + ns)
    return h


@pytest.fixture(scope="module")
def fits():
    out = {}
    for v in VARIANTS:
        design = bytes_design(v)
        out[v] = dict(design=design, h=run(design, v, CPS, NW, NS))
    yield out
    for v in VARIANTS:
        out[v]["h"].close()


def single(design, variant, d, chains=CPS, first=None, nw=NW, ns=NS, go=True):
    """A stand-alone handle on setting d's data with the chain ids of the setting's chains (or of chain `first` alone)."""
    g = Handle(timeline.data_of(design, d), variant, chains=chains, num_warmup=nw, num_samples=ns, chain_id_offset=CPS * d if first is None else first, **OPTS)
    if go:
        g.init()
        g.run(nw + ns)
    return g


# ---------------------------------------------------------------------------------------------------------------- 1. bytes
@pytest.mark.parametrize("variant", VARIANTS)
def test_chains_equal_stand_alone_handles_byte_for_byte(fits, variant):
    h, design = fits[variant]["h"], fits[variant]["design"]
    n = ALL + 1
    _, ncols = _abi.column_layout(design["data"], variant)
    assert h.chain_status()[0] == [0] * (n * CPS)
    d_many, rows_many = h.draws(), h.write_array(0, ncols, NS)
    eps_many, minv_many = h.adaptation()
    for c in range(n * CPS):
        g = single(design, variant, c // CPS, chains=1, first=c)
        eps, minv = g.adaptation()
        assert g.draws()[0].tobytes() == d_many[c].tobytes(), (c, design["labels"][c // CPS])
        assert eps.tobytes() == eps_many[c:c + 1].tobytes() and minv.tobytes() == minv_many[c:c + 1].tobytes(), c
        rows = g.write_array(0, ncols, NS)
        assert np.ascontiguousarray(rows[:, 0]).tobytes() == np.ascontiguousarray(rows_many[:, c]).tobytes(), (c, design["labels"][c // CPS])
        g.close()
    # every scale the variant reads reaches the chains: same chain id, other bytes than on the baseline's data
    ignored = {1 + SCALE_NAMES.index(nm) for nm in ("sigma_m", "sigma_pop", "sigma_e_bias")} if variant != "full" else set()
    for d in range(1, n):
        c = d * CPS
        g = Handle(design["data"], variant, chains=1, num_warmup=NW, num_samples=NS, chain_id_offset=c, **OPTS)
        g.init()
        g.run(NW + NS)
        same = g.draws()[0].tobytes() == d_many[c].tobytes()
        g.close()
        assert same == (d in ignored), (d, design["labels"][d])          # no-mode: the three ignored scales give the baseline's bytes


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_grid_of_the_handles_own_scales_gives_the_rows_of_a_plain_handle(variant):
    data = synthetic.small(variant)
    design = sensitivity.grid(data, {}, null=True)
    assert design["scales"].shape == (2, N_SCALES)
    _, ncols = _abi.column_layout(data, variant)
    rows = []
    for many in (True, False):
        h = Handle(data, variant, chains=4, num_warmup=20, num_samples=20, **OPTS)
        if many:
            timeline.set_design(h, design)
        h.init()
        h.run(40)
        assert h.chain_status()[0] == [0] * 4
        rows.append((h.draws(), h.write_array(0, ncols, 20)))
        h.close()
    assert rows[0][0].tobytes() == rows[1][0].tobytes()
    assert rows[0][1].tobytes() == rows[1][1].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 2. timeline scores
def test_scores_equal_write_array(fits):
    h, design = fits["full"]["h"], fits["full"]["design"]
    lay, _ = _abi.column_layout(design["data"], "full")
    a, b, _ = lay["predicted_score"]
    S, T, n = int(design["data"]["S"]), int(design["data"]["T"]), ALL + 1
    wa = h.write_array(a, b, NS)                                               # [iteration, chain, t + T s]
    want = wa.reshape(NS, n, CPS, S, T).transpose(1, 2, 0, 4, 3).reshape(n, CPS * NS, T, S)
    x = h.timeline_scores_device((0, T)).cpu().numpy()
    for nm in ("random_walk_scale", "mu_b_T_scale", "polling_bias_scale"):
        d = 1 + SCALE_NAMES.index(nm)
        assert x[d].tobytes() == np.ascontiguousarray(want[d]).tobytes(), nm
        assert x[d].tobytes() != x[0].tobytes()
    assert x.tobytes() == np.ascontiguousarray(want).tobytes()


# ---------------------------------------------------------------------------------------------------------------- 3. log-likelihood
@pytest.fixture(scope="module")
def noise_singles(fits):
    design = fits["full"]["design"]
    hs = {nm: single(design, "full", 1 + SCALE_NAMES.index(nm)) for nm in ("sigma_measure_noise_national", "sigma_measure_noise_state")}
    yield hs
    for g in hs.values():
        g.close()


@pytest.mark.parametrize("integrate", [0, 1])
def test_log_lik_with_every_poll_held_equals_the_stand_alone_handles(fits, noise_singles, integrate):
    import torch
    h, design = fits["full"]["h"], fits["full"]["design"]
    g = sensitivity.Grid(h, design, CPS)
    ll = g.log_lik_device(bool(integrate))
    N = h.n_polls
    assert tuple(ll.shape) == (ALL + 1, N, CPS, NS)
    for nm, s in noise_singles.items():
        d = 1 + SCALE_NAMES.index(nm)
        out = torch.empty((N, CPS, NS), dtype=torch.float64, device=ll.device)
        s.log_lik_device(0, N, out, bool(integrate))
        assert ll[d].cpu().numpy().tobytes() == out.cpu().numpy().tobytes(), nm
        assert ll[d].cpu().numpy().tobytes() != ll[0].cpu().numpy().tobytes()


def test_grid_loo_equals_loo_of_the_stand_alone_handle(fits, noise_singles):
    h, design = fits["full"]["h"], fits["full"]["design"]
    got = sensitivity.Grid(h, design, CPS).loo()
    assert len(got) == ALL + 1
    for nm, s in noise_singles.items():
        d = 1 + SCALE_NAMES.index(nm)
        want = loo.loo(s)
        assert got[d].pointwise.tobytes() == want.pointwise.tobytes() and got[d].estimates.tobytes() == want.estimates.tobytes(), nm
        assert got[d].n_draws == want.n_draws == CPS * NS
    cmp_ = loo.loo_compare(*got)
    assert cmp_ is not None


# ---------------------------------------------------------------------------------------------------------------- 4. modes
def test_modes_equal_the_stand_alone_handles_optimize(fits):
    h, design = fits["full"]["h"], fits["full"]["design"]
    n = ALL + 1
    q0 = np.random.default_rng(5).uniform(-1, 1, (n, h.D))
    got = sensitivity.Grid(h, design, CPS).modes(q0=q0, iter=150)
    assert got["q"].shape == (n, 1, h.D)
    for d in (1 + SCALE_NAMES.index("sigma_c"), ALL):
        g = single(design, "full", d, chains=1, nw=0, ns=0, go=False)
        want = g.optimize(q0[d:d + 1], iter=150)
        g.close()
        assert got["q"][d].tobytes() == want["q"].tobytes() and got["lp"][d].tobytes() == want["lp"].tobytes(), d
        assert got["iterations"][d, 0] == want["iterations"][0] > 5
        assert got["q"][d].tobytes() != got["q"][0].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 5. k_sg_distance
def _dist(a, b):
    import torch
    return ecdf_distance_device(torch.as_tensor(np.ascontiguousarray(a), device="cuda:0"), torch.as_tensor(np.ascontiguousarray(b), device="cuda:0"))


def _check(got, a, b, who):
    """ks to 1e-15 (a difference of two integer ratios), w1 to 1e-10 x the column's range, cjs^2 to 1e-10: a sum here has at most 16 384
    terms of order one in fp64."""
    want = sens_ref.distance_columns(a, b)
    assert got.shape == want.shape
    for j in range(a.shape[1]):
        if np.isnan(want[j]).any():
            assert np.isnan(got[j]).all(), (who, j)
            continue
        rng = max(np.ptp(np.concatenate([a[:, j], b[:, j]])), 1e-300)
        e = (abs(got[j, 0] - want[j, 0]) / rng, abs(got[j, 1] - want[j, 1]), abs(got[j, 2] ** 2 - want[j, 2]))
        assert e[0] <= 1e-10 and e[1] <= 1e-15 and e[2] <= 1e-10, (who, j, e, got[j], want[j])
        assert 0 <= got[j, 1] <= 1 and 0 <= got[j, 2] <= 1
    return want


def _swap_check(got, a, b, who):
    back = _dist(b, a)
    for j in range(a.shape[1]):
        rng = max(np.ptp(np.concatenate([a[:, j], b[:, j]])), 1e-300)
        assert abs(back[j, 0] - got[j, 0]) <= 1e-10 * rng and abs(back[j, 1] - got[j, 1]) <= 1e-15 and abs(back[j, 2] ** 2 - got[j, 2] ** 2) <= 1e-10, (who, j)


@pytest.mark.parametrize("na,nb", [(1, 1), (1, 2), (2, 1), (63, 64), (64, 64), (65, 64), (8192, 8192), (8191, 8193)])
def test_distance_against_the_restatement_at_the_edges_of_its_sizes(na, nb):
    rng = np.random.default_rng(1000 * na + nb)
    S2 = 8                                                                      # S + 2 columns
    a, b = rng.standard_normal((na, S2)), 0.3 + 1.2 * rng.standard_normal((nb, S2))
    a[:, 1], b[:, 1] = rng.integers(0, 5, na), rng.integers(1, 6, nb)            # heavy ties
    a[:, 2], b[:, 2] = 1.0, 3.0                                                  # one constant against another
    b[:, 3] = np.resize(a[:, 3], nb)                                             # b repeats a's values
    a[:, 4] *= 1e6
    b[:, 4] *= 1e6                                                               # another scale: w1 is in the column's units
    got = _dist(a, b)
    _check(got, a, b, (na, nb))
    assert got[2].tolist() == [2.0, 1.0, 1.0]
    _swap_check(got, a, b, (na, nb))
    one = _dist(a[:, :1], b[:, :1])                                              # 1 column
    assert one.tobytes() == got[:1].tobytes()


def test_identical_samples_nonfinite_columns_and_a_thousand_columns():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((64, 1000))
    b = rng.standard_normal((65, 1000)) + np.linspace(-1, 1, 1000)
    b[:64, 10] = a[:, 10]
    b[64, 10] = a[0, 10]
    a[5, 20], b[7, 30], a[9, 40] = np.nan, np.inf, -np.inf
    got = _dist(a, b)                                                            # 1 000 columns: more than the workgroups of a launch
    _check(got, a, b, "1000")
    for j in (20, 30, 40):
        assert np.isnan(got[j]).all() and np.isfinite(got[[j - 1, j + 1]]).all()
    for j in (0, 511, 512, 777, 999):                                            # the bytes of a column alone are its bytes among the thousand
        assert _dist(a[:, j:j + 1], b[:, j:j + 1]).tobytes() == got[j:j + 1].tobytes(), j
    same = _dist(a[:, 100:108], a[:, 100:108].copy())                            # identical samples: exactly 0, 0, 0
    assert same.tobytes() == np.zeros((8, 3)).tobytes()
    perm = _dist(a[:, 100:108], a[::-1, 100:108])                                # ... in any order
    assert perm.tobytes() == np.zeros((8, 3)).tobytes()
    z = _dist(np.array([[0.0], [-0.0], [1.0]]), np.array([[-0.0], [0.0], [1.0]]))
    assert z.tobytes() == np.zeros((1, 3)).tobytes()


def test_more_than_16384_draws_is_refused_before_the_device_is_touched():
    import torch
    a, b = torch.zeros((8192, 1), dtype=torch.float64, device="cuda:0"), torch.zeros((8193, 1), dtype=torch.float64, device="cuda:0")
    with pytest.raises(PotusError, match=r"potus_ecdf_distance_device: n_a \+ n_b = 8192 \+ 8193 = 16385: both samples of a column are sorted in LDS, at most 16384"):
        ecdf_distance_device(a, b)
    with pytest.raises(PotusError, match="not device memory"):
        ecdf_distance_device(a[:4], torch.zeros((4, 1), dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------- 6. potus_grid_compare
@pytest.mark.parametrize("base", [0, 3])
def test_grid_compare_equals_the_distance_on_the_slices(fits, base):
    import torch
    h, design = fits["full"]["h"], fits["full"]["design"]
    S, T, n = int(design["data"]["S"]), int(design["data"]["T"]), ALL + 1
    days = (T - 3, T)
    out = h.grid_compare(EV, base, days)
    t = h.grid_timing()                                                         # of this thread's last call: read before the next one
    assert t["distance_ms"] > 0 and t["scores_ms"] > 0
    dist = out["distance"]
    assert dist.shape == (n, 3, S + 2, 3) and out["n_draws"].tolist() == [CPS * NS] * n
    assert dist[base].tobytes() == np.zeros((3, S + 2, 3)).tobytes()
    x = h.timeline_scores_device(days)                                          # [n, draws, 3, S]
    xh = x.cpu().numpy()
    w = np.asarray(design["data"]["state_weights"], dtype=np.float64)
    w = w / w.sum()
    nat = np.zeros(xh.shape[:3])
    for s in range(S):
        nat = nat + w[s] * xh[..., s]
    ev = ((xh > 0.5) * EV.astype(np.float64)).sum(-1)
    for d in range(n):
        want = ecdf_distance_device(x[d].reshape(CPS * NS, 3 * S), x[base].reshape(CPS * NS, 3 * S)).reshape(3, S, 3)
        assert dist[d][:, :S].tobytes() == want.tobytes(), d
        assert dist[d][:, S + 1].tobytes() == _dist(ev[d], ev[base]).tobytes(), d          # sums of integers: exact in any order
        got_nat = dist[d][:, S]
        want_nat = _dist(nat[d], nat[base])                                      # the host's sum is not fused: equal up to the last bit of a value
        assert np.abs(got_nat[:, 0] - want_nat[:, 0]).max() <= 1e-10 and np.abs(got_nat[:, 1] - want_nat[:, 1]).max() <= 1e-15
        assert np.abs(got_nat[:, 2] ** 2 - want_nat[:, 2] ** 2).max() <= 1e-10
    assert (dist[1 + SCALE_NAMES.index("mu_b_T_scale")][2, :S, 1] > 0).all()
    t = h.grid_timing()                                                         # potus_ecdf_distance_device: no scores kernel
    assert t["distance_ms"] > 0 and t["scores_ms"] == 0


def test_a_failed_chain_fails_its_setting_alone():
    data = synthetic.small("full")
    design = sensitivity.grid(data, {"mu_b_T_scale": [2.0], "sigma_c": [0.5]})      # baseline, null copy, two settings
    D = _abi.num_params(data, "full")
    q0 = 0.1 * np.random.default_rng(11).standard_normal((4 * CPS, D))
    good = run(design, "full", CPS, 30, 20, q0)
    want = good.grid_compare(EV)
    good.close()
    bad_q0 = q0.copy()
    bad_q0[5] = 1e308                                                           # a non-finite log density: an error status of chain 5, setting 2
    bad = run(design, "full", CPS, 30, 20, bad_q0)
    status = bad.chain_status()[0]
    assert status[5] != 0 and [s for c, s in enumerate(status) if c != 5] == [0] * 7
    got = bad.grid_compare(EV)
    assert got["n_draws"].tolist() == [40, 40, 0, 40]
    assert np.isnan(got["distance"][2]).all()
    assert got["distance"][[0, 1, 3]].tobytes() == want["distance"][[0, 1, 3]].tobytes()
    every = bad.grid_compare(EV, base=2)                                        # the base failed: every row is NaN
    assert np.isnan(every["distance"]).all() and every["n_draws"].tolist() == [0] * 4
    bad.close()


# ---------------------------------------------------------------------------------------------------------------- 7. it sees what it should
def test_a_wider_prior_is_seen_and_the_null_copy_is_not():
    """Every poll masked, so the posterior is the prior: election-day scores are inv_logit(prior + L_T z_T), and mu_b_T_scale x 3 triples
    their logit-scale spread.  No free threshold: in numpy, with independent draws of a logistic-normal at n = 200 over 200 repetitions,
    the null maximum of cjs was 0.10 and the effect minimum 0.18."""
    data = synthetic.small("full")
    design = sensitivity.grid(data, {"mu_b_T_scale": [3.0]})
    design["keep_state"][:] = False
    design["keep_national"][:] = False
    g = sensitivity.fit(design, "full", chains_per_setting=2, num_warmup=100, num_samples=100, seed=1843)
    try:
        assert g.handle.chain_status()[0] == [0] * 6
        c = g.compare(EV)
        S = int(data["S"])
        null_max, effect_median = float(c.cjs[1, 0, :S].max()), float(np.median(c.cjs[2, 0, :S]))
        print(f"election day, six states: max cjs of the null copy = {null_max:.4f}, median cjs of mu_b_T_scale x 3 = {effect_median:.4f}")
        print(c.table())
        assert effect_median > null_max
        fl = c.flag()
        assert fl[2].any() and not fl[0].any() and not fl[1].any()
        assert np.allclose(c.sensitivity[2], c.cjs[2] / np.log2(3.0)) and np.isnan(c.sensitivity[:2]).all()
        assert c.floor.shape == (3, 1, S + 2) and c.floor[2].tobytes() == c.cjs[1].tobytes()
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(fits):
    data = synthetic.small("full")
    own = np.tile(sensitivity.scales_of(data), (2, 1))

    def refused(match, scales=own, init=False, call=None, **opts):
        g = Handle(data, "full", num_warmup=10, num_samples=10, **dict(dict(chains=2, cus_per_chain=1, twin=0), **opts))
        try:
            if init:
                g.init()
            with pytest.raises(PotusError, match=match):
                (call or (lambda g: g.set_datasets_grid(scales)))(g)
        finally:
            g.close()
    refused(r"potus_set_datasets_grid: both mu_b_T_scale\[\] and scales are given", call=lambda g: g.set_datasets_grid(own, mu_b_T_scale=[0.1, 0.2]))
    for bad in (np.nan, np.inf, 0.0, -0.5):
        for j in (0, 3, 6, 7, 8):
            sc = own.copy()
            sc[1, j] = bad
            refused(rf"potus_set_datasets_grid: data set 2: {SCALE_NAMES[j]} = .*must be positive and finite", scales=sc)
    refused("dense metric is not supported", metric=_abi.METRIC_DENSE)
    refused("one workgroup per chain", cus_per_chain=2)
    refused("not a multiple", chains=3)
    refused("already initialised", init=True)
    # none of the refusals leaves anything behind; a second call is refused
    g = Handle(data, "full", chains=2, num_warmup=10, num_samples=10, cus_per_chain=1, twin=0)
    with pytest.raises(PotusError, match="data set 1: sigma_c"):
        g.set_datasets_grid(own * np.array([[-1.0] + [1.0] * 8, [1.0] * 9]))
    g.set_datasets_grid(own)
    with pytest.raises(PotusError, match="already holds"):
        g.set_datasets_grid(own)
    g.close()
    h = fits["full"]["h"]
    for base in (-1, ALL + 1):
        with pytest.raises(PotusError, match=rf"potus_grid_compare: base = {base} outside the handle's {ALL + 1} data sets"):
            h.grid_compare(EV, base)
    with pytest.raises(PotusError, match="bad day range"):
        h.grid_compare(EV, 0, (3, 3))
    q = np.zeros((1, h.D))
    for call in (lambda: h.constrain(q), lambda: h.simulate_prior(1, 1), lambda: h.sbc_ranks(np.zeros((ALL + 1, 1)), 7, 8)):
        with pytest.raises(PotusError, match="models of their own"):
            call()
    from us_potus_model_amd import sampler
    for call in (lambda: h.posterior_summary(EV.astype(float)), lambda: sampler.device_diagnostics([h], 0, 8), lambda: h.outcomes(EV), lambda: h.monitor(cols=(0, 8)),
                 lambda: loo.loo(h)):
        with pytest.raises(PotusError, match="slice the chains per data set"):
            call()
