"""The boundary as the reference side would drive it, and the reference's published numbers.

* the `.C()` surface: every `potus_R_*` export called with int* / double* / char** arguments exactly as
  R/potus_sampling.R marshals them (R is not installed here, so ctypes replays the shim call for call) and compared
  byte for byte with the struct ABI;
* every posterior number the reference publishes (README.md tables of the 2008 / 2012 / 2016 backtests: 3 x 52 rows
  of election-day predicted_score, plus the Brier scores), tests/golden/readme_*.csv;
* summaries over more draws than one LDS sort holds and over several handles; the cluster watchdog.
"""
import csv
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD
from us_potus_model_amd import Handle, PotusModel, _abi, backtest_scores, dataprep, posterior_summary, run_many, sampler

pytestmark = pytest.mark.gpu

IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)


def _ints(x):
    a = np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int32)
    return a, a.ctypes.data_as(IP)


def _dbls(x):
    a = np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.float64)
    return a, a.ctypes.data_as(DP)


class RShim:
    """R/potus_sampling.R replayed with ctypes: only the potus_R_* exports, every argument a pointer, status by pointer."""

    def __init__(self):
        self.L = sampler.load_library()
        self.keep = []

    def call(self, name, *args):
        f = getattr(self.L, name)
        f.restype = None
        f(*args)

    def check(self, status):
        if status.value != 0:
            buf = C.create_string_buffer(b" " * 512)
            p = (C.c_char_p * 1)(C.addressof(buf))                     # char **: what .C() passes for a character vector
            ln = C.c_int(512)
            self.call("potus_R_last_error", p, C.byref(ln))
            raise RuntimeError(f"libpotus_hmc error {status.value}: {buf.value.decode().strip()}")

    def sample(self, data, variant, seed, chains, iter_warmup, iter_sampling, refresh, gpus=(0,), cus_per_chain=0, metric="diag_e", twin=-1,
               metric_storage="f64", chain_id_offset=0, save_warmup=False, adapt_delta=0.8, max_treedepth=10, init=2.0, pooled_metric=False):
        full = variant == "full"
        Ns, Nn = int(data["N_state_polls"]), int(data["N_national_polls"])
        iv = lambda k, n: _ints(data[k] if data.get(k) is not None else np.zeros(max(n, 1)))
        dv = lambda k, n: _dbls(data[k] if data.get(k) is not None else np.zeros(max(n, 1)))
        dims = _ints([Nn, Ns, data["T"], data["S"], data["P"], data["M"] if full else 0, data["Pop"] if full else 0, 0 if full else 1])
        scalars = _dbls([data["sigma_c"], data["sigma_m"] if full else 0, data["sigma_pop"] if full else 0,
                         data["sigma_measure_noise_national"], data["sigma_measure_noise_state"],
                         data["sigma_e_bias"] if full else 0, data["random_walk_scale"], data["mu_b_T_scale"], data["polling_bias_scale"]])
        cov = _dbls(np.asarray(data["state_covariance_0"], dtype=np.float64).T)          # column-major, as R stores it
        per = [chains // len(gpus) + (1 if g < chains % len(gpus) else 0) for g in range(len(gpus))]
        first = np.concatenate([[0], np.cumsum(per)])[:len(per)]
        handles, counts = [], []
        for g, dev in enumerate(gpus):
            if per[g] == 0:
                continue
            args = [dims, iv("state", Ns), iv("day_state", Ns), iv("day_national", Nn), iv("poll_state", Ns), iv("poll_national", Nn),
                    iv("poll_mode_state", Ns), iv("poll_mode_national", Nn), iv("poll_pop_state", Ns), iv("poll_pop_national", Nn),
                    iv("n_democrat_national", Nn), iv("n_two_share_national", Nn), iv("n_democrat_state", Ns), iv("n_two_share_state", Ns),
                    dv("unadjusted_national", Nn), dv("unadjusted_state", Ns), _dbls(data["mu_b_prior"]), _dbls(data["state_weights"]),
                    scalars, cov,
                    _ints([per[g], chain_id_offset + first[g], iter_warmup, iter_sampling, max_treedepth, dev, int(save_warmup), cus_per_chain,
                           1 if metric == "dense_e" else 0, twin, 1 if metric_storage == "f32" else 0, 1 if pooled_metric else 0]),
                    _dbls([adapt_delta, 0.05, 0.75, 10, 1, init, seed])]
            h, st = C.c_int(-1), C.c_int(-1)
            self.call("potus_R_create", *[a[1] for a in args], C.byref(h), C.byref(st))
            self.check(st)
            self.call("potus_R_init", C.byref(h), C.byref(st))
            self.check(st)
            handles.append(h.value); counts.append(per[g])
        total, done = iter_warmup + iter_sampling, 0
        chunk = total if not refresh else int(refresh)
        hv = _ints(handles)
        while done < total:
            n = min(chunk, total - done)
            st = C.c_int(-1)
            self.call("potus_R_run_many", hv[1], C.byref(C.c_int(len(handles))), C.byref(C.c_int(n)), C.byref(st))
            self.check(st)
            done += n
        D, nc, st = C.c_int(), C.c_int(), C.c_int(-1)
        self.call("potus_R_num_columns", C.byref(C.c_int(handles[0])), C.byref(D), C.byref(nc), C.byref(st))
        self.check(st)
        ns = C.c_int()
        self.call("potus_R_saved_count", C.byref(C.c_int(handles[0])), C.byref(ns), C.byref(st))
        self.check(st)
        return dict(handles=handles, chains_per_handle=counts, D=D.value, n_cols=nc.value, n_saved=ns.value, data=data, variant=variant, chains=chains)

    def write_array(self, fit, begin, end):
        """potus_extract's loop: [iter, chain, col] per handle, chains concatenated in id order."""
        parts = []
        for h, ch in zip(fit["handles"], fit["chains_per_handle"]):
            out = np.zeros(fit["n_saved"] * ch * (end - begin))
            st = C.c_int(-1)
            self.call("potus_R_write_array", C.byref(C.c_int(h)), C.byref(C.c_int(begin)), C.byref(C.c_int(end)), out.ctypes.data_as(DP), C.byref(st))
            self.check(st)
            parts.append(out.reshape(fit["n_saved"], ch, end - begin))
        return np.concatenate(parts, axis=1)

    def summary(self, fit, ev):
        S, T = int(fit["data"]["S"]), int(fit["data"]["T"])
        st_, na, eo, st = np.zeros(T * S * 4), np.zeros(T * 4), np.zeros(T * 5), C.c_int(-1)
        hv = _ints(fit["handles"])
        self.call("potus_R_posterior_summary", hv[1], C.byref(C.c_int(len(fit["handles"]))), _dbls(ev)[1], st_.ctypes.data_as(DP),
                  na.ctypes.data_as(DP), eo.ctypes.data_as(DP), C.byref(st))
        self.check(st)
        return dict(state_raw=st_, state=st_.reshape(S, T, 4).transpose(1, 0, 2), national=na.reshape(T, 4), electoral_votes=eo.reshape(T, 5))

    def diagnostics(self, fit, begin, end):
        rh, es, st = np.zeros(end - begin), np.zeros(end - begin), C.c_int(-1)
        self.call("potus_R_diagnostics", _ints(fit["handles"])[1], C.byref(C.c_int(len(fit["handles"]))), _ints([begin, end])[1], rh.ctypes.data_as(DP),
                  es.ctypes.data_as(DP), C.byref(st))
        self.check(st)
        return rh, es

    def check_convergence(self, fit, rhat_below, ess_at_least):
        conv, out, st = C.c_int(-1), np.zeros(2), C.c_int(-1)
        self.call("potus_R_check_convergence", _ints(fit["handles"])[1], C.byref(C.c_int(len(fit["handles"]))), _dbls([rhat_below, ess_at_least])[1], C.byref(conv),
                  out.ctypes.data_as(DP), C.byref(st))
        self.check(st)
        return conv.value, out[0], out[1]

    def scores(self, fit, summ, ev, won, day=0):
        out, st = np.zeros(3), C.c_int(-1)
        self.call("potus_R_backtest_scores", summ["state_raw"].ctypes.data_as(DP), _ints([fit["data"]["T"], fit["data"]["S"], day])[1],
                  _dbls(ev)[1], _ints(won)[1], out.ctypes.data_as(DP), C.byref(st))
        self.check(st)
        return out

    def csv(self, fit, directory, basename):
        for h in fit["handles"]:
            st = C.c_int(-1)
            d = (C.c_char_p * 1)(str(directory).encode()); b = (C.c_char_p * 1)(basename.encode())
            self.call("potus_R_write_stan_csv", C.byref(C.c_int(h)), d, b, C.byref(st))
            self.check(st)

    def free(self, fit):
        for h in fit["handles"]:
            st = C.c_int(-1)
            self.call("potus_R_destroy", C.byref(C.c_int(h)), C.byref(st))
            self.check(st)


@pytest.mark.parametrize("name", ["small_full", "small_nomode"])
def test_r_entry_points_replay_the_shim(cases, name, tmp_path):
    """potus_R_create -> _init -> _run_many (chunks of `refresh`) -> _num_columns / _saved_count -> _write_array ->
    _posterior_summary -> _diagnostics -> _backtest_scores -> _write_stan_csv -> _destroy, with `gpus = c(0, 0)` (two handles),
    a seed beyond 32 bits and cus_per_chain = 8: the same bytes as the struct ABI, and potus_R_run on its own."""
    data, variant = cases[name]
    seed = 2 ** 40 + 1843
    kw = dict(seed=seed, chains=3, iter_warmup=24, iter_sampling=10, refresh=7)
    r = RShim()
    fit = r.sample(data, variant, gpus=(0, 0), cus_per_chain=8, **kw)
    assert fit["chains_per_handle"] == [2, 1] and fit["n_saved"] == 10
    ref = PotusModel(variant).sample(data, devices=[0, 0], cus_per_chain=8, **kw)
    assert ref._hs[0].cus_per_chain == 8 and fit["D"] == ref._hs[0].D and fit["n_cols"] == ref._hs[0].n_cols
    full = r.write_array(fit, 0, fit["n_cols"])
    assert np.array_equal(full, ref._write_array(0, fit["n_cols"]))
    a, b, _ = ref._hs[0].layout["predicted_score"]
    assert np.array_equal(r.write_array(fit, a, b), full[:, :, a:b])
    S = int(data["S"])
    ev = np.arange(3, 3 + S, dtype=np.float64)
    sm, sm_ref = r.summary(fit, ev), ref.summary(ev)
    for k in ("state", "national", "electoral_votes"):
        assert np.array_equal(sm[k], sm_ref[k]), k
    from us_potus_model_amd import device_diagnostics
    rh, es = r.diagnostics(fit, a, a + 30)
    rh_ref, es_ref = device_diagnostics(ref._hs, a, a + 30)
    assert np.array_equal(rh, rh_ref) and np.array_equal(es, es_ref) and np.isfinite(es).all()
    from us_potus_model_amd import check_convergence
    assert r.check_convergence(fit, 1.5, 1.0) == tuple(int(x) if i == 0 else x for i, x in enumerate(check_convergence(ref._hs, 1.5, 1.0)))
    won = (np.arange(S) % 2).astype(int)
    sc = r.scores(fit, sm, ev, won)
    p = sm["state"][-1, :, 3]
    assert np.isclose(sc[0], np.sum(ev / ev.sum() * (won - p) ** 2)) and np.isclose(sc[1], np.mean((won - p) ** 2))
    assert sc[2] == np.sum(np.round(p) == won)                       # numpy rounds half to even, as R does
    assert backtest_scores(sm_ref, ev, won)["states_correct"] == int(sc[2])
    r.csv(fit, tmp_path, "rshim")
    ref.output_files(tmp_path / "ref", "rshim")
    for c in (1, 2, 3):
        la = [ln for ln in open(tmp_path / f"rshim-{c}.csv") if not ln.startswith("#")]
        lb = [ln for ln in open(tmp_path / "ref" / f"rshim-{c}.csv") if not ln.startswith("#")]
        assert la == lb and len(la) == 11
    # potus_R_run (one handle, no run_many) gives the chain it gives inside run_many; errors come back through *status
    one = r.sample(data, variant, gpus=(0,), cus_per_chain=8, **{**kw, "chains": 1, "iter_warmup": 0, "iter_sampling": 0, "refresh": 0})
    st = C.c_int(-1)
    r.call("potus_R_run", C.byref(C.c_int(one["handles"][0])), C.byref(C.c_int(1)), C.byref(st))
    assert st.value == 0
    r.call("potus_R_run", C.byref(C.c_int(12345)), C.byref(C.c_int(1)), C.byref(st))
    assert st.value == 4                                              # POTUS_ERR_STATE: bad handle
    with pytest.raises(RuntimeError, match="bad handle"):
        r.check(st)
    r.free(one); r.free(fit)
    with pytest.raises(RuntimeError, match="seed"):
        r.sample(data, variant, gpus=(0,), **{**kw, "seed": -1})


def test_rhat_stop_ends_sampling_early_without_changing_a_draw(cases):
    """SURVEY 8(f4), "online R-hat-based early stop" (VERDICT r04 item 8): with rhat_stop the host loop asks potus_check_convergence after every
    `refresh` transitions of the sampling phase -- rank-normalised split R-hat / bulk ESS of lp__ and mu_b[:, T] over the pooled chains of both
    handles, on the device -- and stops once they pass.  The flag trips on the small model; the draws saved up to that point are, bit for bit, the
    first draws of the uninterrupted run; the check's numbers are the numpy restatement's; and a threshold nothing meets never trips.  Declared
    in INTEGRATION.md as a deviation from Stan (off by default)."""
    from us_potus_model_amd import check_convergence, diagnostics as dg
    data, variant = cases["small_full"]
    kw = dict(seed=7, chains=4, iter_warmup=150, iter_sampling=400, refresh=50, devices=[0, 0])
    m_full, m_stop, m_never = PotusModel(variant), PotusModel(variant), PotusModel(variant)
    full = m_full.sample(data, **kw)
    stop = m_stop.sample(data, rhat_stop=1.05, ess_stop=100.0, **kw)
    assert m_full.last_convergence == [] and full.n_saved == 400
    log = m_stop.last_convergence
    assert log and log[-1]["converged"] and all(not c["converged"] for c in log[:-1])
    n = log[-1]["sampling_draws"]
    assert stop.n_saved == n and 50 <= n < 400 and n % 50 == 0
    a, b, _ = full._h.layout["mu_b"]
    assert np.array_equal(stop.as_array("mu_b"), full.as_array("mu_b")[:n])                     # same draws up to the stop
    assert np.array_equal(stop.sampler_params()["lp__"], full.sampler_params()["lp__"][:, :n])
    S, T = int(data["S"]), int(data["T"])
    cols = np.concatenate([stop._write_array(0, 1), stop._write_array(a + S * (T - 1), a + S * T)], axis=2)   # [draw, chain, 1 + S]
    x = np.transpose(cols, (1, 0, 2))
    r_ref = max(dg.rhat(x[:, :, j]) for j in range(1 + S)); e_ref = min(dg.ess_bulk(x[:, :, j]) for j in range(1 + S))
    conv, r, e = check_convergence(stop._hs, 1.05, 100.0)
    assert conv and np.isclose(r, r_ref, rtol=1e-9) and np.isclose(e, e_ref, rtol=1e-9) and r == log[-1]["rhat_max"] and e == log[-1]["ess_bulk_min"]
    never = m_never.sample(data, rhat_stop=1.0, **kw)                                            # R-hat < 1 exactly: never
    assert never.n_saved == 400 and not any(c["converged"] for c in m_never.last_convergence) and len(m_never.last_convergence) == 7
    assert np.array_equal(never.as_array("mu_b"), full.as_array("mu_b"))


def _readme(year):
    from conftest import readme_golden
    return readme_golden(year)


# Tolerances of the README comparison: about twice what the device runs have shown (mean 0.0021, interval ends 0.0046,
# P(win) 0.032 with 4 chains; the oracle's 8 chains: 0.0019 / 0.0043 / 0.031, test_oracle.py).  The published tables are rounded
# to 3 decimals and were knitted from saved fits whose script revision cannot be matched to the committed final_*.R
# (BASELINE.md section 3).  RMSE (README.md:79,175,275, seven digits): the oracle sits 0.7-1.3e-4 below the published values.
TOL_MEAN, TOL_END, TOL_PROB, TOL_BRIER, TOL_RMSE = 0.005, 0.010, 0.045, 0.003, 4e-4


def test_readme_tables_of_the_three_backtests(cases):
    """Everything the reference publishes about these posteriors: README.md:83-136 (2008), :179-232 (2012),
    :279-332 (2016) -- election-day mean / 2.5 % / 97.5 % / P(win) of 51 states + the national vote -- and
    README.md:75,169,260 (Brier scores, states called correctly), against three backtests run concurrently
    (BASELINE configs[3] on one GPU: 4 chains x 16 CUs each, 1000 + 1000, seed 1843) and summarised on the device.
    Round 6: the same three fits against the CPU oracle's own runs of final_2008.R:562-573, final_2012.R:558-569 and final_2016.R:533-541's posteriors
    (tests/golden/posterior_<year>.npz: 8 chains x (1000 + 1000)) -- means of mu_b[:, T] and predicted_score[T, :] within 5 combined MCSE, the
    2.5 % / 97.5 % quantiles within 6 MCSE + 0.004 -- so that both no-mode posteriors and the tag-17 kernels are held to the oracle at full length
    and not only to three published decimals."""
    from conftest import assert_posterior_within_mcse, election_day_draws
    hs, metas, zmax = {}, {}, {}
    for year in ("2008", "2012", "2016"):
        data, variant = cases[year]
        h = Handle(data, variant, chains=4, num_warmup=1000, num_samples=1000, seed=1843)
        h.init()
        hs[year] = h
        metas[year] = dataprep.load_npz(GOLD / f"data_{year}.npz")["meta"]
    for _ in range(20):
        run_many(list(hs.values()), 100)
    report = {}
    for year, h in hs.items():
        meta, rows = _readme(year)
        states, ev = list(metas[year]["states"]), np.asarray(metas[year]["ev_state"], dtype=np.float64)
        sm = h.posterior_summary(ev)
        T = int(h.data["T"])
        worst = dict(mean=0.0, low=0.0, high=0.0, prob=0.0)
        for r in rows:
            got = sm["national"][T - 1] if r["state"] == "--" else sm["state"][T - 1, states.index(r["state"])]
            for k, j in (("low", 0), ("high", 1), ("mean", 2), ("prob", 3)):
                worst[k] = max(worst[k], abs(got[j] - float(r[k])))
        won = np.array([int(next(r for r in rows if r["state"] == s)["won_readme"]) for s in states])
        sc = backtest_scores(sm, ev, won)
        from conftest import rmse_ex_dc
        sc["rmse_ex_dc"] = rmse_ex_dc(states, sm["state"][T - 1, :, 2], rows)
        report[year] = (worst, sc, meta)
        mu_b_T, ps_T = election_day_draws(h, 1000)
        assert mu_b_T.shape == (4, 1000, int(h.data["S"])) and np.allclose(ps_T, 1.0 / (1.0 + np.exp(-mu_b_T)), rtol=0, atol=1e-15)
        zmax[year] = assert_posterior_within_mcse(mu_b_T, ps_T, np.load(GOLD / f"posterior_{year}.npz"))
        st, _ = h.chain_status()
        div = h.write_array(5, 6, 1000)                     # divergent__ of the saved (sampling) draws
        assert st == [0] * 4 and div.mean() < 0.01, (year, st, div.mean())
        h.close()
    print("README deltas:", {y: (w, s) for y, (w, s, _) in report.items()}, "worst z against the oracle's posteriors:", zmax)
    for year, (worst, sc, meta) in report.items():
        assert worst["mean"] <= TOL_MEAN and worst["low"] <= TOL_END and worst["high"] <= TOL_END and worst["prob"] <= TOL_PROB, (year, worst)
        assert abs(sc["ev_wtd_brier"] - meta["ev_wtd_brier"]) <= TOL_BRIER and abs(sc["unwtd_brier"] - meta["unwtd_brier"]) <= TOL_BRIER, (year, sc, meta)
        assert sc["states_correct"] == int(meta["states_correct"]), (year, sc, meta)
        assert abs(sc["rmse_ex_dc"] - meta["rmse_ex_dc"]) <= TOL_RMSE, (year, sc, meta)


@pytest.mark.parametrize("what,factor", [("sigma_m", 1.5), ("sigma_pop", 1.5)])
def test_the_readme_pins_notice_a_wrong_mode_or_population_effect(cases, what, factor):
    """What the pins to the reference are worth for the parts of the model that election-day predicted_score only feels indirectly
    (VERDICT r02): with the prior scale of the poll-mode / poll-population effects off by half, the 2016 backtest no longer meets
    the published EV-weighted Brier score and RMSE within the tolerances test_readme_tables_of_the_three_backtests uses
    (scripts/pin_sensitivity.py -> profiles/r03_pin_sensitivity.txt lists every scale: of the nine, only the pollster scale
    sigma_c moves no pin; mu_c rests on the transcription test and finite differences)."""
    from conftest import rmse_ex_dc
    data, variant = cases["2016"]
    d = dict(data)
    d[what] = float(data[what]) * factor
    meta_d = dataprep.load_npz(GOLD / "data_2016.npz")["meta"]
    pub, rows = _readme("2016")
    states, ev = list(meta_d["states"]), np.asarray(meta_d["ev_state"], dtype=np.float64)
    h = Handle(d, variant, chains=4, num_warmup=1000, num_samples=1000, seed=1843)
    h.init(); h.run(2000)
    sm = h.posterior_summary(ev)
    h.close()
    T = int(d["T"])
    won = np.array([int(next(r for r in rows if r["state"] == s)["won_readme"]) for s in states])
    sc = backtest_scores(sm, ev, won)
    assert abs(sc["ev_wtd_brier"] - pub["ev_wtd_brier"]) > TOL_BRIER, sc
    assert abs(rmse_ex_dc(states, sm["state"][T - 1, :, 2], rows) - pub["rmse_ex_dc"]) > TOL_RMSE, sc


def test_summaries_beyond_one_lds_sort_and_over_several_handles(cases):
    """More pooled draws than one 16 384-element LDS sort holds (the selection over several sorted runs), the chains
    of the posterior spread over two handles: equal to the numpy restatement of final_2016.R:708-762, 799-823."""
    import sys
    sys.path.insert(0, str(GOLD.parent.parent / "oracle"))
    from posterior_summary_ref import posterior_summary as ref_summary
    data, variant = cases["small_full"]
    S, T = int(data["S"]), int(data["T"])
    ns = 3400
    from conftest import second_device
    hs = [Handle(data, variant, chains=c, chain_id_offset=o, num_warmup=100, num_samples=ns, seed=5, device=dev)
          for c, o, dev in ((3, 0, 0), (2, 3, second_device()))]                # two GPUs wherever the box has them: the peer copy of the pooled summary
    for h in hs:
        h.init()
    run_many(hs, 100 + ns)
    ev = np.arange(3, 3 + S, dtype=np.float64) * (538.0 / np.arange(3, 3 + S).sum())
    got = posterior_summary(hs, ev)
    a, b, _ = hs[0].layout["predicted_score"]
    ps = np.concatenate([h.write_array(a, b, ns).reshape(-1, S, T) for h in hs]).transpose(0, 2, 1)     # [draw, T, S]
    assert ps.shape[0] == 5 * ns > 16384
    ref = ref_summary(ps, data["state_weights"], ev)
    for k in ("state", "national", "electoral_votes"):
        assert np.allclose(got[k], ref[k], rtol=1e-12, atol=1e-12), (k, np.abs(got[k] - ref[k]).max())
    assert np.array_equal(got["state"][..., 3], ref["state"][..., 3])
    one = hs[0].posterior_summary(ev)                                   # a single handle: one sorted run, straight from LDS
    ref1 = ref_summary(hs[0].write_array(a, b, ns).reshape(-1, S, T).transpose(0, 2, 1), data["state_weights"], ev)
    assert np.allclose(one["state"], ref1["state"], rtol=1e-12, atol=1e-12)
    for h in hs:
        h.close()


def test_handles_are_recycled(cases):
    data, variant = cases["small_full"]
    a = Handle(data, variant, chains=1, num_warmup=2, num_samples=2)
    ha = a.h
    a.close()
    b = Handle(data, variant, chains=1, num_warmup=2, num_samples=2)
    assert b.h == ha
    b.close()


@pytest.mark.timeout(120)
def test_watchdog_turns_a_missing_member_into_an_error(cases):
    """A cluster whose members are not all running (here: member 3 leaves at once, as if another process held its
    compute unit) must not hang or trap: the launch gives up, potus_run reports POTUS_ERR_WATCHDOG, the process and
    the GPU stay usable."""
    data, variant = cases["small_full"]
    os.environ["POTUS_DEBUG_DROP_MEMBER"] = "4"
    try:
        h = Handle(data, variant, chains=2, num_warmup=10, num_samples=0, cus_per_chain=8, seed=3)
    finally:
        del os.environ["POTUS_DEBUG_DROP_MEMBER"]
    h.init()
    with pytest.raises(sampler.PotusError, match="error 8"):
        h.run(3)
    h.close()
    g = Handle(data, variant, chains=2, num_warmup=10, num_samples=0, cus_per_chain=8, seed=3)
    g.init(); g.run(3)
    assert np.isfinite(g.draws_saved()) and g.total_leapfrogs() > 0
    g.close()


def test_bench_two_ranks_end_to_end_gloo_development_mode(tmp_path):
    """bench.py --gpus 2 as the driver launches it (torch.distributed.run, one process per rank), in the development
    mode that puts both ranks on GPU 0 with gloo collectives: chain blocks keyed by global chain id, potus_run_many
    per rank, device-side write_array, pooled R-hat / ESS on rank 0, ONE JSON line."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, POTUS_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT="29541")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29541", str(ROOT / "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "0", "--chunk", "10",
           "--chains-per-gpu", "4", "--no-cpu-baseline", "--no-saturated"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300, cwd=str(ROOT))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["config"]["total_chains"] == 8 and d["config"]["iter_sampling"] == 20
    assert d["config"]["posteriors"]["2016"]["pooled_draws"] == 8 * 20 and d["leapfrogs"] > 0 and d["roofline"]["frac"] > 0


def test_dot_call_wrappers_fill_r_matrices_in_place(cases, tmp_path):
    """R/src/potus_call.c driven through the stub R API (tests/r_stub/: R is not in the image): potus_call_extract allocates ONE [draws, columns] matrix
    and potus_extract_matrix fills it in R's column-major order, chains merged chain after chain over TWO handles (the second on `second_device()`) --
    equal, element for element, to what the .C() path + the shim's aperm / rbind produce (StanFit.extract restates that); the sampler columns and the
    device diagnostics likewise.  This is rstan::extract(out, pars = "predicted_score")[[1]] of final_2016.R:708 without its two extra copies."""
    from conftest import build_call_wrapper, call_wrapper_int, second_device
    W = build_call_wrapper(tmp_path)
    data, variant = cases["small_full"]
    kw = dict(num_warmup=20, num_samples=12, seed=1843)
    hs = [Handle(data, variant, chains=3, chain_id_offset=0, **kw), Handle(data, variant, chains=2, chain_id_offset=3, device=second_device(), **kw)]
    for h in hs:
        h.init(); h.run(32)
    ids = call_wrapper_int(W, [h.h for h in hs])
    lay = hs[0].layout
    for name in ("predicted_score", "mu_b", "raw_mu_c"):
        a, b_, dims = lay[name]
        r = W.stub_call3(C.cast(W.potus_call_extract, C.c_void_p), ids, call_wrapper_int(W, [a]), call_wrapper_int(W, [b_]))
        assert W.stub_last_error() == b"" and W.XLENGTH(r) == 5 * 12 * (b_ - a) and W.stub_protect_depth() == 0
        got = np.ctypeslib.as_array(W.REAL(r), shape=(b_ - a, 5 * 12)).T            # column-major [draws, columns]
        want = np.concatenate([h.write_array(a, b_, 12).transpose(1, 0, 2).reshape(-1, b_ - a) for h in hs])   # chain-major merge, handle after handle
        assert np.array_equal(got, want), name
    r = W.stub_call1(C.cast(W.potus_call_sampler_params, C.c_void_p), ids)
    sp = np.ctypeslib.as_array(W.REAL(r), shape=(7, 60)).T
    assert np.array_equal(sp, np.concatenate([h.draws()[:, :, :7].reshape(-1, 7) for h in hs]))
    a, b_, _ = lay["mu_b"]
    r = W.stub_call3(C.cast(W.potus_call_diagnostics, C.c_void_p), ids, call_wrapper_int(W, [a]), call_wrapper_int(W, [b_]))
    dgm = np.ctypeslib.as_array(W.REAL(r), shape=(2, b_ - a))
    rh, es = sampler.device_diagnostics(hs, a, b_)
    assert np.array_equal(dgm[0], rh, equal_nan=True) and np.array_equal(dgm[1], es, equal_nan=True)
    bad = W.stub_call3(C.cast(W.potus_call_extract, C.c_void_p), ids, call_wrapper_int(W, [5]), call_wrapper_int(W, [5]))   # an empty range is an R error
    assert b"bad column range" in W.stub_last_error() and W.XLENGTH(bad) == 0 and W.stub_protect_depth() == 0
    W.stub_release_all()
    for h in hs:
        h.close()


def test_bench_single_process_gives_the_pooled_diagnostics_of_the_two_rank_run(tmp_path):
    """`bench.py --gpus 2 --single-process`: the path the reference-side binding takes -- R is ONE process, potus_sample(gpus = 0:1),
    final_2016.R:536 -- two handles of four chains under potus_run_many, the second on `second_device()` where the box has one (else both on GPU 0), pooled
    R-hat / bulk ESS through potus_diagnostics over the two handles.  One line with "launcher": "single_process"; the same chains (global chain ids), hence
    the same leapfrog count and, to 1e-9, the same pooled R-hat / ESS as the two-rank run of the same command (development mode: both ranks on GPU 0, gloo)."""
    import json
    import subprocess
    import sys
    from conftest import ROOT, second_device
    common = ["--gpus", "2", "--steps", "4", "--warmup", "0", "--chunk", "10", "--chains-per-gpu", "4", "--no-cpu-baseline", "--no-saturated"]
    env = dict(os.environ, POTUS_BENCH_DEVICES=f"0,{second_device()}")
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--single-process"] + common, capture_output=True, text=True, env=env, timeout=300, cwd=str(ROOT))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    sp = json.loads(lines[0])
    assert sp["launcher"] == "single_process" and sp["n_gpus"] == 2 and sp["config"]["total_chains"] == 8 and sp["config"]["devices"] == [0, second_device()]
    assert sp["roofline"]["frac"] > 0 and abs(sp["value"] - sp["leapfrogs"] / sp["seconds"]) < 1e-6 * sp["value"]
    # ... and the two-rank run carries the single-process run as side.single_process (rank 0 starts it once both ranks have closed their samplers; the other
    # rank waits on the job's TCP store, not inside a collective: an RCCL barrier would hold compute units the child's cluster launches need)
    env = dict(os.environ, POTUS_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT="29543", POTUS_BENCH_FORCE_SP_SIDE="1", POTUS_BENCH_DEVICES=f"0,{second_device()}")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29543", str(ROOT / "bench.py")] + \
          common + ["--full"]                                   # the side measurements run with --full only
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=str(ROOT))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    mp_ = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert mp_["leapfrogs"] == sp["leapfrogs"] and "launcher" not in mp_
    side = mp_["side"]["single_process"]
    assert side.get("launcher") == "single_process" and side["n_gpus"] == 2 and side["leapfrogs"] == sp["leapfrogs"], side
    assert abs(side["rhat_max"] - sp["rhat_max"]) <= 1e-9 * sp["rhat_max"]
    assert abs(mp_["rhat_max"] - sp["rhat_max"]) <= 1e-9 * sp["rhat_max"] and abs(mp_["ess_bulk_min"] - sp["ess_bulk_min"]) <= 1e-9 * sp["ess_bulk_min"], (mp_["rhat_max"], sp["rhat_max"])


def test_bench_starts_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2 ...` WITHOUT a launcher around it -- the command the driver issues for its scaling runs -- starts two ranks
    by itself (re-execution under torch.distributed.run on 127.0.0.1 with a free port) and prints ONE line with n_gpus = 2, 16 chains,
    configs[2] (until round 4 the bare command ran one rank and printed an n_gpus = 1 line).  On a one-GPU box: the
    development mode (both ranks on GPU 0, gloo collectives, clusters of 8 so that the two processes' workgroups fit the chip together);
    with two GPUs: one rank per GPU over RCCL."""
    import json
    import subprocess
    import sys
    from conftest import ROOT, gpu_count
    two = gpu_count() >= 2
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "POTUS_DIST_BACKEND")}
    if not two:
        env["POTUS_DIST_BACKEND"] = "gloo"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "0", "--chunk", "10", "--no-cpu-baseline", "--no-saturated"] + \
          ([] if two else ["--cus-per-chain", "8"])
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=str(ROOT))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["total_chains"] == 16 and d["config"]["baseline_config_index"] == 2 and "configs[2]" in d["config"]["workload"]
    assert d["config"]["posteriors"]["2016"]["pooled_draws"] == 16 * 10 and d["leapfrogs"] > 0


def test_bench_dump_outputs_hold_the_last_steps_draws(cases, tmp_path):
    """bench.dump_outputs on a handle of the small posterior: every per-draw file holds the LAST n_last saved draws of its columns -- equal to the
    handle's own write_array (host path) of those rows, and not to its first ones -- and the adaptation files equal potus_get_adaptation."""
    import importlib.util
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("bench_dump", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    data, variant = cases["small_full"]
    h = Handle(data, variant, chains=3, num_warmup=10, num_samples=20, seed=1843)
    h.init()
    h.run(30)
    bench.dump_outputs(tmp_path, [("s_", h)], 20, 10)
    host = h.write_array(0, h.n_cols, 20).transpose(1, 0, 2)                     # [chain, draw, column]
    S, T = int(data["S"]), int(data["T"])
    a_mu, a_ps = h.layout["mu_b"][0], h.layout["predicted_score"][0]
    k = np.load(tmp_path / "s_draws_sample.npy").shape[2]
    for name, cols in (("sampler_params", np.arange(7)), ("mu_b_T", a_mu + S * (T - 1) + np.arange(S)),
                       ("predicted_score_T", a_ps + (T - 1) + T * np.arange(S)), ("draws_sample", 7 + bench._seeded_sample(h.n_cols - 7, k))):
        got = np.load(tmp_path / f"s_{name}.npy")
        assert np.array_equal(got, host[:, 10:, cols]), name
        assert not np.array_equal(got, host[:, :10, cols]), name
    eps, minv = h.adaptation()
    assert np.array_equal(np.load(tmp_path / "s_stepsize.npy"), eps) and np.array_equal(np.load(tmp_path / "s_inv_metric.npy"), minv)
    h.close()


def test_bench_plain_run_is_lean_and_dumps_the_same_outputs_twice(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` without --full: the headline line and nothing measured beside it (no CPU baseline, saturated point or
    side runs); --steps sets the timed steps and ms_per_step is their time per step.  --dump-outputs: float64 .npy files within 64 MiB, the same bytes
    from two runs of the same command, predicted_score[T, :] the inverse logit of mu_b[:, T] draw for draw (stan:137)."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "POTUS_DIST_BACKEND")}
    lines, dirs = [], [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--chunk", "10", "--dump-outputs", str(d)]
        out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300, cwd=str(ROOT))
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        got = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(got) == 1
        lines.append(json.loads(got[0]))
    line = lines[0]
    assert line["metric"] == "leapfrog_steps_per_sec" and line["unit"] == "leapfrogs/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == 3 and line["config"]["iter_warmup"] == 10 and line["config"]["iter_sampling"] == 20
    assert abs(line["ms_per_step"] - 1e3 * line["seconds"] / 3) <= 1e-9 * line["ms_per_step"]
    assert not {"cpu_baseline", "saturated", "side"} & set(line) and line["leapfrogs"] == lines[1]["leapfrogs"]
    names = sorted(p.name for p in dirs[0].glob("*.npy"))
    assert names == sorted(p.name for p in dirs[1].glob("*.npy")) and "2016_draws_sample.npy" in names and "2016_rhat.npy" in names
    assert sum((dirs[0] / n).stat().st_size for n in names) <= 64 * 2 ** 20
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype == np.float64 and a.tobytes() == b.tobytes(), n
    sp, mu, ps = (np.load(dirs[0] / f"2016_{n}.npy") for n in ("sampler_params", "mu_b_T", "predicted_score_T"))
    assert sp.shape == (8, 10, 7) and mu.shape == ps.shape == (8, 10, 51) and np.isfinite(sp).all()
    assert np.allclose(ps, 1.0 / (1.0 + np.exp(-mu)), rtol=1e-10, atol=0)


def test_rccl_collectives_on_device_buffers_one_rank():
    """The collectives bench.py issues at N > 1 -- all_gather_into_tensor of the [draws, chains, columns] block, MAX / SUM
    all-reduces of a double, barrier -- on the "nccl" backend (= RCCL) with device tensors.  One GPU here, so a group of
    one rank: shapes, dtypes (f64) and devices go through RCCL as they will on the 8-GPU node."""
    import subprocess
    import sys
    from conftest import ROOT
    code = (
        "import os, torch, torch.distributed as dist\n"
        "os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='29547', RANK='0', WORLD_SIZE='1', LOCAL_RANK='0')\n"
        "from us_potus_model_amd import parallel\n"
        "torch.cuda.set_device(0)\n"
        "dist.init_process_group(backend='nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))\n"
        "dev = torch.device('cuda', 0)\n"
        "x = torch.arange(5 * 8 * 52, dtype=torch.float64, device=dev).reshape(5, 8, 52)\n"
        "y = parallel.all_gather_chains(x, dev)\n"
        "assert y.shape == (5, 8, 52) and y.device.type == 'cuda' and torch.equal(y, x)\n"
        "assert parallel.max_over_ranks(3.5, dev) == 3.5 and parallel.sum_over_ranks(2.25, dev) == 2.25\n"
        # round 6: the all-reduces of the pooled dense metric (parallel.pool_window_moments: count, count x mean, and M2 slice by slice) on device buffers
        "g = torch.Generator(device='cpu').manual_seed(3)\n"
        "w = torch.randn(40, 37, dtype=torch.float64, generator=g).to(dev)\n"
        "mean = w.mean(dim=0); m2 = torch.zeros(37, 40, dtype=torch.float64, device=dev); m2[:, :37] = (w - mean).T @ (w - mean); ref = m2.clone()\n"
        "n, gm = parallel.pool_window_moments(40.0, mean, m2, dev)\n"
        "assert n == 40.0 and torch.allclose(gm, mean, rtol=1e-15, atol=1e-16) and torch.allclose(m2, ref, rtol=1e-14, atol=1e-14) and m2.is_cuda\n"
        "ref2 = m2.clone(); parallel.pool_window_m2(m2, dev, slice_bytes=640)\n"
        "assert torch.equal(m2, ref2)\n"
        "parallel.barrier(); torch.cuda.synchronize(); dist.destroy_process_group(); print('rccl ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=str(ROOT),
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0 and "rccl ok" in out.stdout, out.stdout[-1500:] + out.stderr[-1500:]


# ---------------------------------------------------------------------------------------------------- round 4: diagnostics on the device
def _device_block(block):
    """a host array copied to device memory through the HIP runtime (no torch): returns (pointer, free)"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), block.nbytes) == 0
    assert hip.hipMemcpy(p, block.ctypes.data_as(C.c_void_p), block.nbytes, 1) == 0     # hipMemcpyHostToDevice
    return p, lambda: hip.hipFree(p)


def _numpy_diagnostics(block):
    """us_potus_model_amd/diagnostics.py (the CPU restatement) column by column: block [draws, chains, columns]"""
    from us_potus_model_amd import diagnostics as dg
    x = np.transpose(block, (1, 0, 2))
    return (np.array([dg.rhat(x[:, :, j]) for j in range(x.shape[2])]), np.array([dg.ess_bulk(x[:, :, j]) for j in range(x.shape[2])]))


@pytest.mark.gpu
@pytest.mark.parametrize("draws,chains,ncols", [(301, 4, 37), (1000, 8, 70), (500, 40, 3), (8, 2, 5)])
def test_device_diagnostics_match_the_numpy_restatement(draws, chains, ncols):
    """potus_diagnostics_device against diagnostics.py to 1e-10: AR(1) columns of every autocorrelation from -0.6 to 0.98 (Geyer's
    sequence stops anywhere between lag 2 and a few hundred), chains with different means and scales (R-hat well above 1), a column
    with runs of tied draws (a sampler that keeps its point; ranks by position), a constant-shift column, an odd number of draws
    (the middle one is dropped by the split), 40 x 500 = 20 000 pooled draws (more than one LDS sort: order statistics across runs)."""
    rng = np.random.default_rng(draws + chains)
    blk = np.zeros((draws, chains, ncols))
    for j in range(ncols):
        rho = np.linspace(-0.6, 0.98, ncols)[j]
        e = rng.standard_normal((draws, chains))
        x = np.zeros((draws, chains))
        x[0] = e[0]
        for t in range(1, draws):
            x[t] = rho * x[t - 1] + np.sqrt(1 - rho * rho) * e[t]
        if j % 5 == 1:
            x = x * (1.0 + 0.5 * np.arange(chains)) + 0.7 * np.arange(chains)            # chains that disagree
        if j % 5 == 2:
            x = np.repeat(x[::3], 3, axis=0)[:draws]                                      # every draw three times in a row: ties
        if j % 5 == 3:
            x = np.round(x, 1)                                                            # heavy ties across chains too
        blk[:, :, j] = x
    L = sampler.load_library()
    p, free = _device_block(blk)
    rhat, ess = np.zeros(ncols), np.zeros(ncols)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = L.potus_diagnostics_device(0, p, draws, chains, ncols, dp(rhat), dp(ess))
    free()
    assert rc == 0
    r_ref, e_ref = _numpy_diagnostics(blk)
    assert np.allclose(rhat, r_ref, rtol=1e-10, atol=0, equal_nan=True), np.nanmax(np.abs(rhat / r_ref - 1))
    assert np.allclose(ess, e_ref, rtol=1e-10, atol=0, equal_nan=True), np.nanmax(np.abs(ess / e_ref - 1))


@pytest.mark.gpu
def test_device_diagnostics_of_non_finite_columns_and_saved_warmup_rows(cases):
    """a column holding a NaN or an infinite draw gets NaN for both diagnostics (numpy propagates it; the padding key of the
    bitonic sort is a NaN pattern); with save_warmup = 1 the warm-up rows are left out, as rstan::monitor / extract() leave them out;
    more pooled chains than the kernel's tables hold are refused before anything is allocated."""
    from us_potus_model_amd import device_diagnostics
    rng = np.random.default_rng(3)
    blk = rng.standard_normal((200, 4, 4))
    blk[17, 2, 1] = np.nan
    blk[5, 0, 2] = np.inf
    blk[199, 3, 3] = -np.inf
    L = sampler.load_library()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    p, free = _device_block(blk)
    rhat, ess = np.zeros(4), np.zeros(4)
    assert L.potus_diagnostics_device(0, p, 200, 4, 4, dp(rhat), dp(ess)) == 0
    r_ref, e_ref = _numpy_diagnostics(blk[:, :, :1])
    assert np.allclose(rhat[0], r_ref[0], rtol=1e-10) and np.allclose(ess[0], e_ref[0], rtol=1e-10)
    assert np.isnan(rhat[1:]).all() and np.isnan(ess[1:]).all()
    assert L.potus_diagnostics_device(0, p, 2, 600, 1, dp(rhat), dp(ess)) != 0            # 600 chains pooled: refused up front
    free()
    data, variant = cases["small_full"]
    h = Handle(data, variant, chains=3, num_warmup=40, num_samples=30, seed=5, save_warmup=1)
    h.init(); h.run(70)
    a = h.layout["mu_b"][0]
    for cb, ce in ((0, 1), (a, a + 12)):
        rhat, ess = device_diagnostics([h], cb, ce)
        r_ref, e_ref = _numpy_diagnostics(h.write_array(cb, ce, 70)[40:])                 # the 30 sampling rows only
        assert np.allclose(rhat, r_ref, rtol=1e-10, equal_nan=True) and np.allclose(ess, e_ref, rtol=1e-10, equal_nan=True)
    h.close()


@pytest.mark.gpu
def test_device_diagnostics_over_the_chains_of_several_handles(cases):
    """potus_diagnostics pools the chains of the listed handles (chain ids 1-3 and 4-5 of one posterior): lp__ and a block of mu_b
    columns against diagnostics.py on the same rows fetched with potus_write_array."""
    from us_potus_model_amd import device_diagnostics
    data, variant = cases["small_full"]
    from conftest import second_device
    hs = [Handle(data, variant, chains=c, chain_id_offset=off, num_warmup=100, num_samples=60, seed=3, cus_per_chain=k, device=dev)
          for c, off, k, dev in ((3, 0, 1, 0), (2, 3, 4, second_device()))]
    for h in hs:
        h.init(); h.run(160)
    a = hs[0].layout["mu_b"][0]
    for cb, ce in ((0, 1), (a, a + 40)):
        rhat, ess = device_diagnostics(hs, cb, ce)
        blk = np.concatenate([h.write_array(cb, ce, 60) for h in hs], axis=1)            # [draws, chains, columns]
        r_ref, e_ref = _numpy_diagnostics(blk)
        assert np.allclose(rhat, r_ref, rtol=1e-10, equal_nan=True) and np.allclose(ess, e_ref, rtol=1e-10, equal_nan=True)
    for h in hs:
        h.close()


@pytest.mark.gpu
def test_pooled_entry_points_accept_and_refuse_the_same_handle_lists(cases):
    """What every call that pools the chains of several handles does with a list of handles: `a` and `b` hold chains 1-2 and 3-4 of one posterior
    (b on `second_device()`), `g` the other variant (another number of columns), `o` other poll counts (same columns), `short` the posterior of
    `a` with fewer saved draws, `few` fewer than four.  [a, b] is pooled; [a, a] is refused as listed twice, [a, g] and [a, o] as another
    posterior (potus_extract_matrix only looks at the number of columns, in its own words), [a, short] for its unequal counts except by the
    summary, the outcomes and the scenario, which pool whatever is saved; potus_check_convergence says "not yet" before it looks at the list while the first handle holds
    fewer than four draws.  (PSIS-LOO's own refusals: tests/test_gpu_loo.py.)"""
    from conftest import second_device
    from us_potus_model_amd import check_convergence, device_diagnostics, loo as loo_mod, monitor as monitor_mod, outcomes as outcomes_mod, scenario as scenario_mod
    from us_potus_model_amd.sampler import PotusError
    data, variant = cases["small_full"]
    kw = dict(num_warmup=30, num_samples=20, seed=11, cus_per_chain=1, twin=0)

    def fit(d, v, n_iter, **more):
        h = Handle(d, v, chains=2, **kw, **more)
        h.init(); h.run(n_iter)
        return h

    a = fit(data, variant, 50)
    b = fit(data, variant, 50, chain_id_offset=2, device=second_device())
    g = fit(*cases["small_nomode"], 50)
    o = fit(dict(data, n_democrat_state=np.asarray(data["n_democrat_state"]) // 2), variant, 50)
    short = fit(data, variant, 40, chain_id_offset=2)
    few = fit(data, variant, 32, chain_id_offset=2)
    S = int(data["S"])
    L = a.L
    L.potus_extract_matrix.argtypes = [IP, C.c_int, C.c_int, C.c_int, DP, C.c_longlong, C.POINTER(C.c_longlong)]

    def extract(hs):
        ids, rows = (C.c_int * len(hs))(*[h.h for h in hs]), C.c_longlong()
        sampler._check(L, L.potus_extract_matrix(ids, len(hs), 0, 3, None, 0, C.byref(rows)))
        out = np.zeros((3, rows.value))
        sampler._check(L, L.potus_extract_matrix(ids, len(hs), 0, 3, out.ctypes.data_as(DP), rows.value, None))
        return out

    calls = {"extract": extract, "summary": lambda hs: posterior_summary(hs, np.ones(S)), "diagnostics": lambda hs: device_diagnostics(hs, 0, 3),
             "check_convergence": check_convergence, "loo": loo_mod.loo, "monitor": lambda hs: monitor_mod.monitor(hs, cols=(0, 3)),
             "outcomes": lambda hs: outcomes_mod.outcomes(hs, np.ones(S)), "scenario": scenario_mod.scenario}
    for name, call in calls.items():
        call([a, b])
        with pytest.raises(PotusError, match="twice"):
            call([a, a])
        with pytest.raises(PotusError, match="different posteriors" if name == "extract" else "another posterior"):
            call([a, g])
        if name == "extract":
            assert call([a, o]).shape == (3, 80)                       # same columns: taken
        else:
            with pytest.raises(PotusError, match="another posterior"):
                call([a, o])
        if name in ("summary", "outcomes", "scenario"):
            call([a, short])                                           # 2 x 20 + 2 x 10 draws
        else:
            with pytest.raises(PotusError, match="libpotus_hmc error 4.*saved"):
                call([a, short])
    assert extract([a, b]).shape == (3, 80)
    assert np.array_equal(extract([a, b])[:, :40], extract([a]))
    assert check_convergence([few, few]) == (False, pytest.approx(np.nan, nan_ok=True), pytest.approx(np.nan, nan_ok=True))
    with pytest.raises(PotusError, match="at least four"):
        device_diagnostics([few], 0, 3)
    for h in (a, b, g, o, short, few):
        h.close()


@pytest.mark.gpu
def test_device_entry_points_refuse_what_is_not_their_device_memory():
    """The *_device entry points that take a block of the caller's and a device number, with the smallest valid arguments and no sampler: a
    block in device memory of the named GPU is taken; a host pointer (a NumPy array's), a device number past the last GPU and, where there
    are two GPUs, a block of the other one are refused -- each before anything is launched, so no kernel ever sees such a pointer."""
    import torch
    from conftest import gpu_count
    L = sampler.load_library()
    LLP, I32P = C.POINTER(C.c_longlong), C.POINTER(C.c_int32)
    rng = np.random.default_rng(5)
    cols = rng.normal(size=(8, 2, 3))                                  # [draws, chains, columns]
    ll = rng.normal(-3.0, 0.7, (3, 2, 8))                              # [polls, chains, draws]
    items = rng.uniform(0.3, 0.7, (8, 1, 3))                           # [draws, days, states]
    w, ev, probs = np.full(3, 1.0 / 3), np.array([3, 4, 5], dtype=np.int32), np.array([0.5])
    out = np.zeros(64)
    nk = C.c_longlong(0)
    o, o2 = out[:32].ctypes.data_as(DP), out[32:].ctypes.data_as(DP)
    calls = {
        "potus_diagnostics_device": (cols, lambda dev, p: L.potus_diagnostics_device(dev, p, 8, 2, 3, o, o2)),
        "potus_monitor_device": (cols, lambda dev, p: L.potus_monitor_device(dev, p, 8, 2, 3, probs.ctypes.data_as(DP), 1, o)),
        "potus_loo_device": (ll, lambda dev, p: L.potus_loo_device(dev, p, 3, 2, 8, None, o, o2)),
        "potus_outcomes_device": (items, lambda dev, p: L.potus_outcomes_device(dev, p, 8, 1, 3, w.ctypes.data_as(DP), ev.ctypes.data_as(I32P), 7, None,
                                                                                 None, None, None, None, out.ctypes.data_as(LLP))),
        "potus_scenario_device": (items, lambda dev, p: L.potus_scenario_device(dev, p, 8, 1, 3, w.ctypes.data_as(DP), 0, None, None, None, 7, C.byref(nk),
                                                                                 o, None, None, None, None)),
    }

    def message():
        buf = C.create_string_buffer(512)
        L.potus_last_error(buf, 512)
        return buf.value.decode()
    for name, (host, call) in calls.items():
        host = np.ascontiguousarray(host)
        here = torch.tensor(host, device="cuda:0")
        torch.cuda.synchronize()
        assert call(0, C.c_void_p(here.data_ptr())) == 0, (name, message())
        assert call(0, C.c_void_p(host.ctypes.data)) == 1 and "not device memory" in message() and name in message()
        assert call(gpu_count(), C.c_void_p(here.data_ptr())) == 2 and "no HIP device" in message() and name in message()   # POTUS_ERR_DEVICE
        if gpu_count() >= 2:
            there = torch.tensor(host, device="cuda:1")
            torch.cuda.synchronize()
            assert call(0, C.c_void_p(there.data_ptr())) == 1 and "not device memory" in message()


@pytest.mark.gpu
def test_bench_two_ranks_over_rccl_on_two_gpus():
    """bench.py --gpus 2 exactly as the driver launches it -- torch.distributed.run, one rank per GPU, backend "nccl" (= RCCL over
    xGMI): chains sharded by global chain id, the device-side all-gather of lp__ + mu_b, pooled R-hat / ESS on the device, ONE JSON
    line labelled configs[2].  Needs two GPUs: skipped on the one-GPU boxes of the build rounds, run by an 8-GPU driver box."""
    import json
    import subprocess
    import sys
    from conftest import ROOT, gpu_count
    if gpu_count() < 2:
        pytest.skip("one GPU on this box: the two-rank RCCL run needs two")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29551", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("POTUS_DIST_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29551", str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--chunk", "20", "--no-cpu-baseline", "--no-saturated"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=str(ROOT))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["total_chains"] == 16 and d["config"]["baseline_config_index"] == 2 and "configs[2]" in d["config"]["workload"]
    post = d["config"]["posteriors"]["2016"]
    assert post["pooled_draws"] == 16 * 20 and post["device_diagnostics"]["columns"] == 12955 + 51 and d["leapfrogs"] > 0
