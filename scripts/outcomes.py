#!/usr/bin/env python3
"""Joint election outcomes of a backtest (us_potus_model_amd/outcomes.py): fits the design, then prints the election-day tipping-point
table (final_2012.R:836-843), the summary of the electoral-vote distribution (final_2016.R:904-920), the probabilities of a split between
popular vote and electoral college, and the p-values of the certified result (README.Rmd:481-502; `actual` of tests/golden/readme_<year>.csv),
and times the call (all days, after one untimed call that loads the kernels).

    python scripts/outcomes.py --design 2016 --chains 8 --warmup 1000 --samples 1000 --out profiles/outcomes_2016.txt

--timing (2016 design): the comparison of DESIGN.md section 4f instead, in one process that alternates the calls compared --
(a) potus_outcomes over all days, (b) potus_outcomes_device on a built block of --block-draws draws, (c) potus_posterior_summary_many on the
same handles, (d) the host route (potus_extract_matrix of predicted_score, then tests/outcomes_ref.py vectorised over the draws) -- as the
median of --repeats calls with the spread beside it.
"""
import argparse
import csv
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from us_potus_model_amd import dataprep, outcomes as oc  # noqa: E402
from us_potus_model_amd.sampler import PotusModel, posterior_summary  # noqa: E402

VARIANT = {"2016": "full", "2012": "no_mode_adjustment", "2008": "no_mode_adjustment"}
HBM_PEAK = 8.0e12      # bytes / s, MI355X


def certified(year, states):
    lines = (ROOT / "tests" / "golden" / f"readme_{year}.csv").read_text().splitlines()
    rows = csv.DictReader(ln for ln in lines if not ln.startswith("#"))
    act = {r["state"]: float(r["actual"]) for r in rows if r["state"] != "--"}
    return np.array([act[s] for s in states])


def fit_design(a):
    npz = dataprep.load_npz(ROOT / "tests" / "golden" / f"data_{a.design}.npz")
    data, meta = npz["data"], npz["meta"]
    states, ev = [str(s) for s in meta["states"]], np.asarray(meta["ev_state"], dtype=np.int64)
    t0 = time.perf_counter()
    fit = PotusModel(VARIANT[a.design]).sample(data, seed=a.seed, chains=a.chains, iter_warmup=a.warmup, iter_sampling=a.samples, refresh=0)
    return data, states, ev, fit, time.perf_counter() - t0


def stats(ms):
    ms = np.asarray(ms)
    return f"median {np.median(ms):9.3f}  min {ms.min():9.3f}  max {ms.max():9.3f}"


def report(a):
    data, states, ev, fit, t_fit = fit_design(a)
    actual = certified(a.design, states)
    T = int(data["T"])
    fit.outcomes(ev, actual=actual)                                      # loads the kernels
    t0 = time.perf_counter()
    allday = fit.outcomes(ev, actual=actual)
    t_all = time.perf_counter() - t0
    ph = oc.last_timing()
    t0 = time.perf_counter()
    o = oc.outcomes(fit._hs, ev, actual=actual, days=(T - 1, T), states=states)
    t_last = time.perf_counter() - t0
    sm = fit.summary(ev.astype(np.float64))
    lines = [f"# joint outcomes: design {a.design} ({VARIANT[a.design]}), {a.chains} chains, warm-up {a.warmup}, sampling {a.samples}, seed {a.seed}; "
             f"{o.n_draws} draws, {T} days (fit {t_fit:.1f} s)",
             f"# potus_outcomes: all {T} days {t_all * 1e3:.1f} ms (produce + gather {ph[0]:.1f}, day range {ph[1]:.1f}, counting kernel {ph[2]:.2f}); "
             f"election day alone {t_last * 1e3:.1f} ms", "",
             "## tipping-point state on election day (final_2012.R:836-843): state, prop"]
    lines += [f"{s:4s}{p:8.4f}" for s, p in o.tipping_point()]
    s = o.ev_summary()
    a_, b_ = o.popular_vote_split()
    lines += ["", "## Democratic electoral votes on election day (final_2016.R:904-920)",
              f"mean {s['mean']:.2f}  median {s['median']:.1f}  95 % interval [{s['low']:.1f}, {s['high']:.1f}]  P(>= 270) {s['prob']:.4f}  "
              f"mode {int(np.argmax(o.ev_hist[-1]))} ({o.ev_distribution().max():.4f})",
              f"P(popular-vote win, electoral-college loss) {a_:.4f}   P(popular-vote loss, electoral-college win) {b_:.4f}",
              f"P(electoral-college win) on the first / middle / last day of the series: "
              f"{allday.win_probability()[0]:.4f} / {allday.win_probability()[T // 2]:.4f} / {allday.win_probability()[-1]:.4f}", "",
              "## p-value of the certified result among the draws (README.Rmd:481-502), sorted; * = outside the 95 % interval",
              "state  actual   p_value"]
    pv, out = o.p_values(), o.outside_ci(sm)
    for i in np.argsort(pv, kind="stable"):
        lines.append(f"{states[i]:5s}{actual[i]:8.4f}{pv[i]:10.4f}{' *' if out[i] else ''}")
    lines += ["", f"outside the 95 % interval: {int(out.sum())} of {len(states)} states"]
    return "\n".join(lines) + "\n"


def timing(a):
    import torch
    sys.path.insert(0, str(ROOT / "tests"))
    import outcomes_ref
    data, states, ev, fit, t_fit = fit_design(a)
    hs = fit._hs
    L = hs[0].L
    S, T = int(data["S"]), int(data["T"])
    actual = certified(a.design, states)
    evf = ev.astype(np.float64)
    w = outcomes_ref.normalised_weights(data["state_weights"])
    nd = sum(h.opts.chains * h.post_warmup_saved() for h in hs)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    blk = 0.5 + 0.05 * torch.randn((a.block_draws, T, S), dtype=torch.float64, device="cuda:0", generator=g)
    import ctypes as C
    ids = (C.c_int * len(hs))(*[h.h for h in hs])
    lo, hi, _ = hs[0].layout["predicted_score"]

    def host_route():
        rows = C.c_longlong(0)
        L.potus_extract_matrix.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_longlong)]
        assert L.potus_extract_matrix(ids, len(hs), lo, hi, None, 0, C.byref(rows)) == 0
        m = np.zeros((hi - lo, rows.value))                                          # column-major [rows, columns]
        assert L.potus_extract_matrix(ids, len(hs), lo, hi, m.ctypes.data_as(C.POINTER(C.c_double)), rows.value, C.byref(rows)) == 0
        t1 = time.perf_counter()
        ps = m.reshape(S, T, rows.value).transpose(2, 1, 0)                          # [draw, T, S]
        r = outcomes_ref.outcomes_vectorised(ps, w, ev, 270, actual)
        return r, t1

    calls = {"a": [], "a_produce": [], "a_days": [], "a_count": [], "b": [], "b_count": [], "c": []}
    fit.outcomes(ev, actual=actual); oc.outcomes_of_block(blk, w, ev, actual=actual); posterior_summary(hs, evf)      # untimed
    for _ in range(a.repeats):
        t0 = time.perf_counter(); ra = fit.outcomes(ev, actual=actual); calls["a"].append((time.perf_counter() - t0) * 1e3)
        p = oc.last_timing(); calls["a_produce"].append(p[0]); calls["a_days"].append(p[1]); calls["a_count"].append(p[2])
        t0 = time.perf_counter(); oc.outcomes_of_block(blk, w, ev, actual=actual); calls["b"].append((time.perf_counter() - t0) * 1e3)
        calls["b_count"].append(oc.last_timing()[2])
        t0 = time.perf_counter(); posterior_summary(hs, evf); calls["c"].append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    rd, t1 = host_route()
    t_d = (t1 - t0, time.perf_counter() - t1)
    same = all(np.array_equal(getattr(ra, k), rd[k]) for k in ("ev_hist", "tipping", "joint", "below_actual"))
    med = {k: float(np.median(v)) for k, v in calls.items()}
    spread_c = max(calls["c"]) - min(calls["c"])
    bytes_b = a.block_draws * T * S * 8
    lines = [f"# joint outcomes, timing: design {a.design}, {a.chains} chains, warm-up {a.warmup}, sampling {a.samples}, seed {a.seed} (fit {t_fit:.1f} s); one MI355X, warm,",
             f"# one process alternating (a), (b), (c); {a.repeats} repeats each after one untimed call; host clock around each call (every call ends",
             "# synchronised), counting kernel by HIP events; milliseconds", "",
             f"(a) potus_outcomes, {nd} draws x {T} days x {S} states            {stats(calls['a'])}",
             f"      produce + gather predicted_score (k_write_array)      {stats(calls['a_produce'])}",
             f"      day range -> [draw][day][S] (k_oc_days)                {stats(calls['a_days'])}",
             f"      counting kernel (k_oc_count, HIP events)               {stats(calls['a_count'])}",
             f"(b) potus_outcomes_device, built block of {a.block_draws} draws       {stats(calls['b'])}",
             f"      counting kernel (k_oc_count, HIP events)               {stats(calls['b_count'])}",
             f"      = {bytes_b / 1e9:.2f} GB read once: {bytes_b / (med['b_count'] * 1e-3) / 1e12:.3f} TB/s, {100 * bytes_b / (med['b_count'] * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak",
             f"(c) potus_posterior_summary_many, the same handles           {stats(calls['c'])}",
             f"(d) host route, once: potus_extract_matrix of predicted_score {t_d[0] * 1e3:.0f} ms, then tests/outcomes_ref.py vectorised {t_d[1] * 1e3:.0f} ms;",
             f"      its counts equal those of (a): {'yes' if same else 'NO'}", "",
             f"gate: (a) median {med['a']:.3f} <= (c) median {med['c']:.3f} + spread of (c) {spread_c:.3f} = {med['c'] + spread_c:.3f}: "
             f"{'ok' if med['a'] <= med['c'] + spread_c else 'NOT MET'}"]
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=("2016", "2012", "2008"), default="2016")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--block-draws", type=int, default=64000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    torch.cuda.init()                                  # torch's GPU runtime first, as bench.py does
    text = timing(a) if a.timing else report(a)
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
