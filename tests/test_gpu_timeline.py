"""The forecast timeline on the MI355X: run dates as the data sets of one handle (potus_set_datasets_ex, k_write_array_ds), their scores
(k_tl_scores) and their summaries (k_tl_summary), against stand-alone handles on timeline.mask(...) of each data set, against
potus_posterior_summary and against the numpy restatement in tests/timeline_ref.py."""
import numpy as np
import pytest

import timeline_ref
from test_timeline_host import drop_set
from us_potus_model_amd import _abi, synthetic, timeline
from us_potus_model_amd.sampler import Handle, PotusError

pytestmark = pytest.mark.gpu
NW, NS, CPD, N_DS = 150, 50, 2, 4
EV = np.array([100, 90, 80, 70, 60, 138])      # 538 in all; 270 to win, as potus_posterior_summary has it
OPTS = dict(seed=1843, cus_per_chain=1, twin=0)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """The scores come back as torch tensors: torch's GPU runtime comes up before this module's first library call (as bench.py does)."""
    import torch
    torch.cuda.init()


def small_design():
    """synthetic.small with four data sets that differ in the ways the feature allows: all polls; a mask that empties a day and a pollster;
    no poll at all with another prior and scale; only the scale changed."""
    data = synthetic.small("full")
    ks, kn, _, _ = drop_set(data)
    Ns, Nn, S = int(data["N_state_polls"]), int(data["N_national_polls"]), int(data["S"])
    keep_s = np.stack([np.ones(Ns, bool), ks, np.zeros(Ns, bool), np.ones(Ns, bool)])
    keep_n = np.stack([np.ones(Nn, bool), kn, np.zeros(Nn, bool), np.ones(Nn, bool)])
    prior = np.tile(np.asarray(data["mu_b_prior"], dtype=np.float64), (N_DS, 1))
    prior[2] += np.linspace(-0.3, 0.4, S)
    scale = np.array([data["mu_b_T_scale"], data["mu_b_T_scale"], 0.2, 0.15])
    return timeline.design_of(data, keep_s, keep_n, prior, scale)


def fit(design, chains_per_ds, nw, ns, q0=None):
    h = Handle(design["data"], "full", chains=N_DS * chains_per_ds, num_warmup=nw, num_samples=ns, **OPTS)
    timeline.set_design(h, design)
    h.init(q0)
    h.run(nw + ns)
    return h


@pytest.fixture(scope="module")
def tl():
    design = small_design()
    h = fit(design, CPD, NW, NS)
    lay, ncols = _abi.column_layout(design["data"], "full")
    a, b, _ = lay["predicted_score"]
    S, T = int(design["data"]["S"]), int(design["data"]["T"])
    wa = h.write_array(a, b, NS)                                               # [iteration, chain, t + T s]
    # reference scores [data set, draw (chain after chain), day, state], computed once
    ref = wa.reshape(NS, N_DS, CPD, S, T).transpose(1, 2, 0, 4, 3).reshape(N_DS, CPD * NS, T, S).copy()
    ref.setflags(write=False)
    yield dict(h=h, design=design, lay=lay, ncols=ncols, ref=ref, S=S, T=T)
    h.close()


@pytest.fixture(scope="module")
def singles(tl):
    """Per data set a stand-alone handle on timeline.mask(...) of it, with the chain ids of the data set's chains."""
    hs = []
    for d in range(N_DS):
        g = Handle(timeline.data_of(tl["design"], d), "full", chains=CPD, num_warmup=NW, num_samples=NS, chain_id_offset=CPD * d, **OPTS)
        g.init()
        g.run(NW + NS)
        hs.append(g)
    yield hs
    for g in hs:
        g.close()


def test_chains_equal_stand_alone_handles_byte_for_byte(tl):
    h, design, ncols = tl["h"], tl["design"], tl["ncols"]
    assert h.chain_status()[0] == [0] * (N_DS * CPD)
    d_many = h.draws()
    eps_many, minv_many = h.adaptation()
    rows_many = h.write_array(0, ncols, NS)
    for c in range(N_DS * CPD):
        g = Handle(timeline.data_of(design, c // CPD), "full", chains=1, num_warmup=NW, num_samples=NS, chain_id_offset=c, **OPTS)
        g.init()
        g.run(NW + NS)
        eps, minv = g.adaptation()
        assert g.draws()[0].tobytes() == d_many[c].tobytes(), c
        assert eps.tobytes() == eps_many[c:c + 1].tobytes() and minv.tobytes() == minv_many[c:c + 1].tobytes(), c
        rows = g.write_array(0, ncols, NS)
        for name, (a, b, _) in tl["lay"].items():                             # mu_b, predicted_score and logit_pi depend on the data set's prior
            assert np.ascontiguousarray(rows[:, 0, a:b]).tobytes() == np.ascontiguousarray(rows_many[:, c, a:b]).tobytes(), (c, name)
        assert np.ascontiguousarray(rows[:, 0]).tobytes() == np.ascontiguousarray(rows_many[:, c]).tobytes(), c
        g.close()
    # the data sets differ, and so do their chains: also the two that differ in the scale alone
    assert d_many[0].tobytes() != d_many[2].tobytes() and d_many[0].tobytes() != d_many[6].tobytes()


@pytest.mark.parametrize("variant", ["full", "no_mode_adjustment"])
def test_data_sets_that_are_the_handles_own_give_the_rows_of_a_plain_handle(variant):
    """One row loop serves both kinds of handle: with chains_per_ds = 2 (k_write_array_ds; two data sets that are the handle's own data, prior
    and scale) and with chains_per_ds = 0 (k_write_array, the plain handle) it must pick the same model for every chain.  4 x 130 = 520 rows:
    the 512 workgroups wrap."""
    data = synthetic.small(variant)
    Ns, Nn, nw, ns = int(data["N_state_polls"]), int(data["N_national_polls"]), 20, 130
    design = timeline.design_of(data, np.ones((2, Ns), bool), np.ones((2, Nn), bool), np.tile(np.asarray(data["mu_b_prior"], dtype=np.float64), (2, 1)),
                                np.full(2, float(data["mu_b_T_scale"])))
    _, ncols = _abi.column_layout(data, variant)
    rows = []
    for many in (True, False):
        h = Handle(data, variant, chains=4, num_warmup=nw, num_samples=ns, **OPTS)
        if many:
            timeline.set_design(h, design)
        h.init()
        h.run(nw + ns)
        assert h.chain_status()[0] == [0] * 4
        rows.append((h.draws(), h.write_array(0, ncols, ns)))
        h.close()
    assert rows[0][1].shape == (ns, 4, ncols) and ns * 4 > 512
    assert rows[0][0].tobytes() == rows[1][0].tobytes()
    assert rows[0][1].tobytes() == rows[1][1].tobytes()


@pytest.mark.parametrize("days", ["first", "last", "all", "middle"])
def test_scores_equal_write_array(tl, days):
    T = tl["T"]
    t0, t1 = dict(first=(0, 1), last=(T - 1, T), all=(0, T), middle=(10, 13))[days]
    x = tl["h"].timeline_scores_device((t0, t1)).cpu().numpy()
    want = tl["ref"][:, :, t0:t1]
    assert x.shape == want.shape == (N_DS, CPD * NS, t1 - t0, tl["S"])
    print("max |scores - write_array| =", np.abs(x - want).max())
    assert x.tobytes() == np.ascontiguousarray(want).tobytes()                  # exact: no re-association is declared (potus_timeline.hpp)
    if days == "last":
        y = tl["h"].timeline_scores_device().cpu().numpy()                     # the default range is election day
        assert y.tobytes() == x.tobytes()


def _compare(got, want, who):
    """Quantiles, probabilities and EV figures to 1e-15, means to 1e-12 (another order of a sum of <= 111 terms in [0, 1]: <= 111 x 2^-53)."""
    for key, mean_col in (("state", 2), ("national", 2), ("electoral_votes", None)):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape, (who, key)
        err = np.abs(g - w)
        print(who, key, "max abs difference per column", err.reshape(-1, g.shape[-1]).max(0))
        for j in range(g.shape[-1]):
            assert err[..., j].max() <= (1e-12 if j == mean_col else 1e-15), (who, key, j, err[..., j].max())


def test_summary_equals_posterior_summary_and_the_restatement(tl, singles):
    h, T, w = tl["h"], tl["T"], tl["design"]["data"]["state_weights"]
    out = h.timeline(EV, (0, T))
    assert out["n_draws"].tolist() == [CPD * NS] * N_DS
    for d in range(N_DS):
        got = dict(state=out["state"][d], national=out["national"][d], electoral_votes=out["electoral_votes"][d])
        _compare(got, singles[d].posterior_summary(EV), f"data set {d} against potus_posterior_summary")
        _compare(got, timeline_ref.summary(tl["ref"][d], w, EV), f"data set {d} against timeline_ref")
    last = h.timeline(EV)                                                       # election day alone: the same numbers
    assert last["state"].tobytes() == np.ascontiguousarray(out["state"][:, T - 1:]).tobytes()
    assert last["electoral_votes"].tobytes() == np.ascontiguousarray(out["electoral_votes"][:, T - 1:]).tobytes()
    # the data sets are different posteriors: no poll at all and a wider scale give the widest election-day intervals
    width = out["state"][:, T - 1, :, 1] - out["state"][:, T - 1, :, 0]
    assert (width[2] > width[0]).all()
    ms = h.timeline_timing()
    assert ms["scores_ms"] > 0 and ms["summary_ms"] > 0


def test_summary_with_fractional_quantile_positions():
    """3 chains x 37 draws per data set: 111 draws, (n - 1) p = 2.75, 107.25 and 55; not a multiple of a wave."""
    design = small_design()
    h = fit(design, 3, 60, 37)
    T, S = int(design["data"]["T"]), int(design["data"]["S"])
    lay, _ = _abi.column_layout(design["data"], "full")
    a, b, _ = lay["predicted_score"]
    ref = h.write_array(a, b, 37).reshape(37, N_DS, 3, S, T).transpose(1, 2, 0, 4, 3).reshape(N_DS, 111, T, S)
    out = h.timeline(EV, (T - 3, T), ev_to_win=200)
    assert out["n_draws"].tolist() == [111] * N_DS
    for d in range(N_DS):
        got = dict(state=out["state"][d], national=out["national"][d], electoral_votes=out["electoral_votes"][d])
        _compare(got, timeline_ref.summary(ref[d][:, T - 3:], design["data"]["state_weights"], EV, ev_to_win=200), f"data set {d}")
    h.close()


def test_outcomes_of_a_date_equal_the_stand_alone_handle(tl, singles):
    t = timeline.Timeline(tl["h"], tl["design"], CPD)
    for d in range(N_DS):
        a = t.outcomes(d, EV, days=(0, tl["T"]))
        b = singles[d].outcomes(EV)
        assert a.n_draws == b.n_draws == CPD * NS
        for k in ("ev_hist", "tipping", "joint"):
            assert getattr(a, k).dtype == np.int64 and np.array_equal(getattr(a, k), getattr(b, k)), (d, k)
    s = t.summary(EV)
    assert s["rhat_max"].shape == (N_DS,) and np.isfinite(s["rhat_max"]).all() and (s["ess_bulk_min"] > 0).all()
    sc = t.scenario(1, ev=EV, given={0: "win"})
    assert 0 <= sc.n_kept <= CPD * NS


def test_a_failed_chain_fails_its_data_set_alone():
    design = small_design()
    D = _abi.num_params(design["data"], "full")
    q0 = 0.1 * np.random.default_rng(11).standard_normal((N_DS * CPD, D))
    good = fit(design, CPD, 40, 20, q0)
    want = good.timeline(EV)
    good.close()
    bad_q0 = q0.copy()
    bad_q0[5] = 1e308                                                           # a non-finite log density: an error status of chain 5, data set 2
    bad = fit(design, CPD, 40, 20, bad_q0)
    status = bad.chain_status()[0]
    assert status[5] != 0 and [s for c, s in enumerate(status) if c != 5] == [0] * 7
    got = bad.timeline(EV)
    assert got["n_draws"].tolist() == [40, 40, 0, 40]
    for k in ("state", "national", "electoral_votes"):
        assert np.isnan(got[k][2]).all(), k
        keep = [0, 1, 3]
        assert got[k][keep].tobytes() == want[k][keep].tobytes(), k
    x = bad.timeline_scores_device().cpu().numpy()
    assert np.isnan(x[2]).all() and np.isfinite(x[[0, 1, 3]]).all()
    bad.close()


def test_refusals(tl):
    design = tl["design"]
    data = design["data"]

    def refused(match, design=design, init=False, **opts):
        g = Handle(data, "full", num_warmup=10, num_samples=10, **dict(dict(chains=N_DS, cus_per_chain=1, twin=0), **opts))
        try:
            if init:
                g.init()
            with pytest.raises(PotusError, match=match):
                timeline.set_design(g, design)
        finally:
            g.close()
    refused("already initialised", init=True)
    refused("one workgroup per chain", cus_per_chain=2)
    refused("not a multiple", chains=N_DS + 1)
    g = Handle(data, "full", chains=N_DS, num_warmup=10, num_samples=10, cus_per_chain=1, twin=0)
    y = np.tile(np.asarray(data["n_democrat_state"], np.int32), (N_DS, 1))
    y[1, 3] = int(data["n_two_share_state"][3]) + 1
    with pytest.raises(PotusError, match=r"potus_set_datasets_ex: data set 2: n_democrat_state\[4\]"):   # names the function that was called
        g.set_datasets_ex(n_democrat_state=y)
    n0 = np.zeros((N_DS, int(data["N_state_polls"])), np.int32)                 # a poll the data set has not seen cannot have Democrats in it
    with pytest.raises(PotusError, match="data set 1: n_democrat_state"):
        g.set_datasets_ex(n_two_share_state=n0)
    for s in (0.0, -0.1, np.nan):
        with pytest.raises(PotusError, match="mu_b_T_scale"):
            g.set_datasets_ex(mu_b_T_scale=[0.1, s, 0.1, 0.1])
    g.set_datasets_ex(mu_b_T_scale=[0.1, 0.2, 0.1, 0.1])                        # ... and none of the refusals left anything behind
    with pytest.raises(PotusError, match="already holds"):
        g.set_datasets_ex(mu_b_T_scale=[0.1, 0.2, 0.1, 0.1])
    g.close()
    # more than 16 384 draws per data set: refused on the arguments, before the device is touched
    g = Handle(synthetic.small("no_mode_adjustment"), "no_mode_adjustment", chains=1, num_warmup=0, num_samples=16385, cus_per_chain=1, twin=0)
    with pytest.raises(PotusError, match="at most 16384"):
        g.timeline(EV)
    g.close()
    h = tl["h"]
    with pytest.raises(PotusError, match="bad day range"):
        h.timeline(EV, (3, 3))
    # calls that build rows with the handle's one model
    q = np.zeros((1, h.D))
    for call in (lambda: h.constrain(q), lambda: h.simulate_prior(1, 1), lambda: h.sbc_ranks(np.zeros((N_DS, 1)), 7, 8)):
        with pytest.raises(PotusError, match="models of their own"):
            call()
    # the pooled calls still refuse
    from us_potus_model_amd import sampler
    for call in (lambda: h.posterior_summary(EV.astype(float)), lambda: sampler.device_diagnostics([h], 0, 8), lambda: h.outcomes(EV), lambda: h.monitor(cols=(0, 8))):
        with pytest.raises(PotusError, match="slice the chains per data set"):
            call()
