"""CPU tests of the forecast timeline (us_potus_model_amd.timeline, dataprep.build_timeline): a masked poll is a truncated poll (against the
oracle), the run dates of the reference's CSVs on one design, the committed fixture, the numpy restatement of the summary, and the names of
the new entry points in the header, the R shim and sampler.EXPORTS."""
import os
import re
from pathlib import Path

import numpy as np
import pytest

import timeline_ref
from oracle_lib import OracleModel
from us_potus_model_amd import _abi, dataprep, sampler, synthetic, timeline

ROOT = Path(__file__).resolve().parent.parent
REF_DATA = Path(os.environ.get("POTUS_REFERENCE_DATA", "/root/reference/data"))
needs_csvs = pytest.mark.skipif(not (REF_DATA / "all_polls.csv").exists(), reason="the reference's CSVs are not on this machine")
POLL_KEYS = ("state", "day_state", "poll_state", "poll_mode_state", "poll_pop_state", "unadjusted_state", "n_democrat_state", "n_two_share_state",
             "day_national", "poll_national", "poll_mode_national", "poll_pop_national", "unadjusted_national", "n_democrat_national", "n_two_share_national")


def drop_set(data):
    """Polls to drop from synthetic.small: every poll of the pollster with the fewest polls (at least one), and every poll of one polled day."""
    ps, pn = np.asarray(data["poll_state"]), np.asarray(data["poll_national"])
    cnt = np.bincount(np.concatenate([ps, pn]), minlength=int(data["P"]) + 1)
    p = min((c, i) for i, c in enumerate(cnt) if i >= 1 and c > 0)[1]
    day = int(np.asarray(data["day_state"])[np.asarray(data["poll_state"]) != p][0])
    keep_s = (ps != p) & (np.asarray(data["day_state"]) != day)
    keep_n = (pn != p) & (np.asarray(data["day_national"]) != day)
    assert 0 < keep_s.sum() < keep_s.size and keep_n.sum() < keep_n.size
    return keep_s, keep_n, p, day


def truncated(data, keep_s, keep_n, p):
    """The data list without the dropped polls and without pollster p (the pollsters after it move down by one)."""
    d = dict(data)
    for k in POLL_KEYS:
        if k in data:
            d[k] = np.asarray(data[k])[keep_s if k.endswith("state") else keep_n]
    for k in ("poll_state", "poll_national"):
        assert (d[k] != p).all()
        d[k] = np.where(d[k] > p, d[k] - 1, d[k]).astype(np.int32)
    d["N_state_polls"], d["N_national_polls"], d["P"] = int(keep_s.sum()), int(keep_n.sum()), int(data["P"]) - 1
    return d


@pytest.mark.parametrize("variant", ["full", "no_mode_adjustment"])
def test_a_masked_poll_is_a_truncated_poll(variant):
    data = synthetic.small(variant)
    keep_s, keep_n, p, day = drop_set(data)
    assert not ((np.asarray(data["day_state"]) == day) & keep_s).any()
    masked = timeline.mask(data, keep_s, keep_n)
    assert (masked["n_two_share_state"][~keep_s] == 0).all() and (masked["n_democrat_national"][~keep_n] == 0).all()
    assert (masked["n_two_share_state"][keep_s] == np.asarray(data["n_two_share_state"])[keep_s]).all()
    trunc = truncated(data, keep_s, keep_n, p)
    lay, _ = _abi.column_layout(data, variant)
    D = _abi.num_params(data, variant)
    shared = np.ones(D, bool)
    a, _, _ = lay["raw_mu_c"]
    shared[a - 7 + p - 1] = False
    a, _, _ = lay["raw_measure_noise_national"]
    shared[a - 7 + np.flatnonzero(~keep_n)] = False
    a, _, _ = lay["raw_measure_noise_state"]
    shared[a - 7 + np.flatnonzero(~keep_s)] = False
    assert shared.sum() == _abi.num_params(trunc, variant)
    mm, mt = OracleModel(masked, variant), OracleModel(trunc, variant)
    rng = np.random.default_rng(3)
    for q in (rng.uniform(-2, 2, D), 0.3 * rng.standard_normal(D)):
        lp_m, g_m = mm.log_prob_grad(q)
        lp_t, g_t = mt.log_prob_grad(q[shared])
        want = -0.5 * np.sum(q[~shared] ** 2)
        assert abs((lp_m - lp_t) - want) <= 1e-12 * max(1.0, abs(lp_m)), (lp_m, lp_t, want)
        assert np.abs(g_m[shared] - g_t).max() <= 1e-12 * max(1.0, np.abs(g_t).max())
        assert np.abs(g_m[~shared] + q[~shared]).max() <= 1e-12


def test_mask_replaces_prior_and_scale_and_checks_shapes():
    data = synthetic.small("full")
    ks, kn = np.ones(70, bool), np.ones(25, bool)
    d = timeline.mask(data, ks, kn, np.arange(6.0), 0.2)
    assert d["mu_b_prior"].tolist() == list(range(6)) and d["mu_b_T_scale"] == 0.2 and data["mu_b_T_scale"] == 0.12
    assert timeline.mask(data, ks, kn)["n_two_share_state"].tobytes() == np.asarray(data["n_two_share_state"], np.int32).tobytes()
    with pytest.raises(ValueError):
        timeline.mask(data, ks[:-1], kn)
    with pytest.raises(ValueError):
        timeline.mask(data, ks, kn, np.zeros(5))



@needs_csvs
def test_build_timeline_2016_against_build_2016():
    dates = ["2016-07-07", "2016-09-01", "2016-10-19", "2016-11-08"]
    design = dataprep.build_timeline(REF_DATA, 2016, dates)
    last = dataprep.build_2016(REF_DATA, dates[-1], _levels=True)
    for k, v in dataprep.build_2016(REF_DATA, dates[-1])["data"].items():
        assert np.asarray(design["data"][k]).tobytes() == np.asarray(v).tobytes(), k
    assert design["keep_state"][-1].all() and design["keep_national"][-1].all()
    for j, r in enumerate(dates[:3]):
        b = dataprep.build_2016(REF_DATA, r, _levels=True)
        d = b["data"]
        assert design["keep_state"][j].sum() == d["N_state_polls"] and design["keep_national"][j].sum() == d["N_national_polls"]
        assert d["T"] == design["data"]["T"]
        assert np.asarray(d["state_weights"]).tobytes() == np.asarray(design["data"]["state_weights"]).tobytes()
        assert np.asarray(d["state_covariance_0"]).tobytes() == np.asarray(design["data"]["state_covariance_0"]).tobytes()
        assert design["mu_b_prior"][j].tobytes() == np.asarray(d["mu_b_prior"], np.float64).tobytes()
        assert design["mu_b_T_scale"][j] == d["mu_b_T_scale"]
        for kind, keep in (("state", design["keep_state"][j]), ("national", design["keep_national"][j])):
            kept = [k for k, m in zip(dataprep._poll_keys(last, kind), keep) if m]
            assert sorted(kept) == sorted(dataprep._poll_keys(b, kind)), (r, kind)
        # the masked data list of the date holds the date's counts and nothing else
        m = timeline.data_of(design, j)
        assert int((m["n_two_share_state"] > 0).sum()) == d["N_state_polls"] and m["n_two_share_state"].sum() == np.asarray(d["n_two_share_state"]).sum()
    # the dates differ in all three things
    assert design["mu_b_T_scale"][0] > design["mu_b_T_scale"][1] > design["mu_b_T_scale"][3]
    assert design["mu_b_prior"][0].tobytes() != design["mu_b_prior"][3].tobytes()


@needs_csvs
def test_build_timeline_2012_and_a_date_that_must_raise():
    design = dataprep.build_timeline(REF_DATA, 2012, ["2012-10-01", "2012-11-06"])
    b = dataprep.build_backtest(REF_DATA, 2012, "2012-10-01")
    last = dataprep.build_backtest(REF_DATA, 2012, "2012-11-06")
    assert design["keep_state"][0].sum() == b["data"]["N_state_polls"] < last["data"]["N_state_polls"]
    assert design["mu_b_prior"][0].tobytes() == np.asarray(b["data"]["mu_b_prior"], np.float64).tobytes() and design["mu_b_T_scale"][0] == b["data"]["mu_b_T_scale"]
    for kind, keep in (("state", design["keep_state"][0]), ("national", design["keep_national"][0])):
        assert sorted(k for k, m in zip(dataprep._poll_keys(last, kind), keep) if m) == sorted(dataprep._poll_keys(b, kind))
    # 2016-03-02: the polls known by then begin on 2016-03-01, the campaign's first poll in the field began on 2016-02-28 -- T would be 252, not 254
    with pytest.raises(ValueError, match="run date 2016-03-02: the first day moves"):
        dataprep.build_timeline(REF_DATA, 2016, ["2016-03-02", "2016-11-08"])
    # 2012-03-01: no poll yet; the date is named, not a NaN conversion deep in the build
    with pytest.raises(ValueError, match="run date 2012-03-01"):
        dataprep.build_timeline(REF_DATA, 2012, ["2012-03-01", "2012-11-06"])
    with pytest.raises(ValueError, match="ascending"):
        dataprep.build_timeline(REF_DATA, 2016, ["2016-11-08", "2016-10-01"])


def test_fixture_loads_on_the_committed_design():
    data = dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")["data"]
    design = timeline.load_fixture(ROOT / "tests" / "golden" / "timeline_2016.npz", data)
    n = design["keep_state"].shape[0]
    assert n == 32 and design["keep_state"].shape == (n, data["N_state_polls"]) and design["keep_national"].shape == (n, data["N_national_polls"])
    assert design["keep_state"][-1].all() and design["keep_national"][-1].all() and design["run_dates"][-1] == "2016-11-08"
    assert (np.diff(design["keep_state"].sum(1)) >= 0).all() and (np.diff(design["mu_b_T_scale"]) < 0).all()
    assert design["mu_b_prior"][-1].tobytes() == np.asarray(data["mu_b_prior"], np.float64).tobytes() and design["mu_b_T_scale"][-1] == data["mu_b_T_scale"]
    m = timeline.data_of(design, 0)
    assert (m["n_democrat_state"] <= m["n_two_share_state"]).all() and int((m["n_two_share_state"] > 0).sum()) == design["keep_state"][0].sum()


@needs_csvs
def test_fixture_regenerates_bit_for_bit(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_timeline_fixture", ROOT / "scripts" / "make_timeline_fixture.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(REF_DATA, tmp_path / "t.npz")
    a, b = np.load(tmp_path / "t.npz"), np.load(ROOT / "tests" / "golden" / "timeline_2016.npz")
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def test_reference_summary_restatement():
    rng = np.random.default_rng(0)
    x = rng.random((37, 2, 5))
    w, ev = rng.random(5), np.array([3.0, 10.0, 7.0, 4.0, 6.0])
    s = timeline_ref.summary(x, w, ev, ev_to_win=15)
    np.testing.assert_allclose(s["state"][..., 0], np.quantile(x, 0.025, axis=0), rtol=0, atol=1e-15)    # numpy's default is type 7 too
    np.testing.assert_allclose(s["state"][..., 1], np.quantile(x, 0.975, axis=0), rtol=0, atol=1e-15)
    nat = x @ (w / w.sum())
    np.testing.assert_allclose(s["national"][:, 2], nat.mean(0), atol=1e-15)
    np.testing.assert_allclose(s["national"][:, 3], (nat > 0.5).mean(0))
    e = ((x > 0.5) * ev).sum(-1)
    np.testing.assert_allclose(s["electoral_votes"], np.stack([e.mean(0), np.median(e, 0), np.quantile(e, 0.975, axis=0), np.quantile(e, 0.025, axis=0),
                                                              (e >= 15).mean(0)], -1), atol=1e-12)
    assert timeline_ref.quantile7(np.array([1.0, 2.0, 4.0]), 0.5) == 2.0 and timeline_ref.quantile7(np.array([3.0]), 0.975) == 3.0


def test_entry_points_are_declared_everywhere():
    hdr = (ROOT / "include" / "potus_hmc.h").read_text()
    new = {"potus_set_datasets_ex", "potus_timeline", "potus_timeline_scores_device", "potus_timeline_timing", "potus_R_set_datasets_ex", "potus_R_timeline"}
    assert new <= set(re.findall(r"\b(potus_[A-Za-z_0-9]+)\s*\(", hdr))
    assert new <= set(sampler.EXPORTS)
    r = (ROOT / "R" / "potus_sampling.R").read_text()
    assert "potus_R_set_datasets_ex" in r and "potus_R_timeline" in r and "potus_timeline <- function" in r
    L = sampler.load_library()
    assert L.potus_timeline_timing(None) != 0            # an argument refusal: no device needed
