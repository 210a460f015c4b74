#!/usr/bin/env python3
"""Conditional forecast of a backtest (us_potus_model_amd/scenario.py): fits the design, then prints P(condition), the win probability, the
summary of the electoral-vote distribution and the tipping point GIVEN the condition beside the unconditional ones, the election-day
correlation of AL, CA, FL, MN, NC, NM, RI, WI (the eight of final_2016.R:714), and the timing table of DESIGN.md section 4h: in one
process that alternates the calls -- potus_scenario without a condition, potus_scenario with a condition that keeps about a quarter of the
draws (the national vote within mean +- 0.674 sd, the quartiles of a normal with its moments, and one close state won), potus_outcomes on the same handles -- the median of
--repeats calls with the spread, the split of potus_scenario_timing, and the host route once (potus_extract_matrix, tests/scenario_ref.py).

    python scripts/scenario.py --design 2016 --given FL=lose,PA=lose,national=0.48:0.52 --out profiles/scenario_2016.txt
"""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from us_potus_model_amd import dataprep, outcomes as oc, scenario as sc  # noqa: E402
from us_potus_model_amd.sampler import PotusModel  # noqa: E402

VARIANT = {"2016": "full", "2012": "no_mode_adjustment", "2008": "no_mode_adjustment"}
EIGHT = ("AL", "CA", "FL", "MN", "NC", "NM", "RI", "WI")
HBM_PEAK = 8.0e12      # bytes / s, MI355X


def parse_given(text):
    """FL=lose,PA=win,national=0.48:0.52 -> {"FL": "lose", "PA": "win", "national": (0.48, 0.52)}; a missing side of lo:hi is free"""
    given = {}
    for item in filter(None, (text or "").split(",")):
        key, _, val = item.partition("=")
        if val in ("win", "lose"):
            given[key] = val
        else:
            lo, _, hi = val.partition(":")
            given[key] = (float(lo) if lo else None, float(hi) if hi else None)
    return given


def stats(ms):
    ms = np.asarray(ms)
    return f"median {np.median(ms):9.3f}  min {ms.min():9.3f}  max {ms.max():9.3f}"


def side_by_side(title, a, b):
    return f"{title:44s}{a:>22s}{b:>22s}"


def report(a, data, states, ev, fit):
    T = int(data["T"])
    given = parse_given(a.given)
    un = fit.scenario(ev, days=(T - 1, T), states=states)
    co = fit.scenario(ev, given=given, days=(T - 1, T), states=states)
    lines = [f"## given {a.given} on election day: P(condition) = {co.n_kept} / {co.n_draws} = {co.probability:.4f}", "",
             side_by_side("", "unconditional", "given the condition")]
    if co.n_kept == 0:
        return lines + ["no draw meets the condition", ""]
    su, sc_ = un.outcomes.ev_summary(), co.outcomes.ev_summary()
    lines += [side_by_side("P(electoral-college win)", f"{un.outcomes.win_probability()[-1]:.4f}", f"{co.outcomes.win_probability()[-1]:.4f}"),
              side_by_side("P(popular-vote win)", f"{un.outcomes.joint[-1, -1, -1] / un.n_kept:.4f}", f"{co.outcomes.joint[-1, -1, -1] / co.n_kept:.4f}"),
              side_by_side("Democratic electoral votes: mean", f"{su['mean']:.2f}", f"{sc_['mean']:.2f}"),
              side_by_side("  median", f"{su['median']:.1f}", f"{sc_['median']:.1f}"),
              side_by_side("  95 % interval", f"[{su['low']:.1f}, {su['high']:.1f}]", f"[{sc_['low']:.1f}, {sc_['high']:.1f}]"),
              side_by_side("national vote: mean (sd)", f"{un.mean[-1, -1]:.4f} ({un.sd()[-1]:.4f})", f"{co.mean[-1, -1]:.4f} ({co.sd()[-1]:.4f})")]
    tu, tc = un.outcomes.tipping_point()[:6], co.outcomes.tipping_point()[:6]
    for k in range(max(len(tu), len(tc))):
        f = lambda t: f"{t[k][0]} {t[k][1]:.4f}" if k < len(t) else ""   # noqa: E731
        lines.append(side_by_side("tipping point (state, share)" if k == 0 else "", f(tu), f(tc)))
    idx = [states.index(s) for s in EIGHT if s in states]
    for title, r in (("unconditional", un), ("given the condition", co)):
        cor = r.cor()[np.ix_(idx, idx)]
        lines += ["", f"## election-day correlation of the state scores, {title} (final_2016.R:710-715)", "      " + "".join(f"{states[i]:>7s}" for i in idx)]
        lines += [f"{states[i]:6s}" + "".join(f"{v:7.3f}" for v in row) for i, row in zip(idx, cor)]
    return lines + [""]


def timing(a, data, states, ev, fit):
    sys.path.insert(0, str(ROOT / "tests"))
    import outcomes_ref
    import scenario_ref
    hs = fit._hs
    L = hs[0].L
    S, T = int(data["S"]), int(data["T"])
    w = outcomes_ref.normalised_weights(data["state_weights"])
    nd = sum(h.opts.chains * h.post_warmup_saved() for h in hs)
    # about a quarter: the national vote within mean +- 0.674 sd (a normal's quartiles, not the draws' own), and the state closest to even won
    un = fit.scenario(ev, days=(T - 1, T))
    share = np.diagonal(un.outcomes.joint[-1])[:S] / un.n_kept
    i = int(np.argmin(np.abs(share - 0.5)))
    z = 0.6744897501960817
    m, s = un.mean[-1, S], un.sd()[S]
    quarter = {i: "win", "national": (m - z * s, m + z * s)}
    calls = {k: [] for k in ("u", "c", "o", "o_count")}
    split = {k: [[] for _ in range(5)] for k in ("u", "c")}
    fit.scenario(ev); fit.scenario(ev, given=quarter); fit.outcomes(ev)                         # untimed: loads the kernels
    for _ in range(a.repeats):
        t0 = time.perf_counter(); ru = fit.scenario(ev); calls["u"].append((time.perf_counter() - t0) * 1e3)
        for k, v in enumerate(sc.last_timing()):
            split["u"][k].append(v)
        t0 = time.perf_counter(); rc = fit.scenario(ev, given=quarter); calls["c"].append((time.perf_counter() - t0) * 1e3)
        for k, v in enumerate(sc.last_timing()):
            split["c"][k].append(v)
        t0 = time.perf_counter(); fit.outcomes(ev); calls["o"].append((time.perf_counter() - t0) * 1e3)
        calls["o_count"].append(oc.last_timing()[2])
    # the host route, once
    ids = (C.c_int * len(hs))(*[h.h for h in hs])
    lo, hi, _ = hs[0].layout["predicted_score"]
    rows = C.c_longlong(0)
    L.potus_extract_matrix.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_longlong)]
    t0 = time.perf_counter()
    assert L.potus_extract_matrix(ids, len(hs), lo, hi, None, 0, C.byref(rows)) == 0
    mat = np.zeros((hi - lo, rows.value))                                                        # column-major [rows, columns]
    assert L.potus_extract_matrix(ids, len(hs), lo, hi, mat.ctypes.data_as(C.POINTER(C.c_double)), rows.value, C.byref(rows)) == 0
    t1 = time.perf_counter()
    ps = mat.reshape(S, T, rows.value).transpose(2, 1, 0)[:, T - 1:, :]                          # election day alone: the restatement is a Python loop per item
    blo, bhi = sc.parse_given(quarter, S)
    want = scenario_ref.scenario(ps, w, 0, blo, bhi, ev=ev)
    t2 = time.perf_counter()
    same = (want["n_kept"] == rc.n_kept and all(np.array_equal(getattr(rc.outcomes, k)[-1], want[k][0]) for k in ("ev_hist", "tipping", "joint")))
    v = np.sqrt(np.diagonal(want["cov"][0]))
    cov_err = float((np.abs(rc.cov[-1] - want["cov"][0]) / (v[:, None] * v[None, :])).max())
    med = {k: [float(np.median(x)) for x in split[k]] for k in split}
    block_bytes = nd * T * S * 8
    lines = [f"## timing: {nd} draws x {T} days x {S} states, all days; one MI355X, warm, one process alternating the three calls; {a.repeats} repeats each",
             "## after one untimed call; host clock around each call (every call ends synchronised); milliseconds", "",
             f"potus_scenario, no condition                          {stats(calls['u'])}",
             f"    produce + gather predicted_score                  {stats(split['u'][0])}",
             f"    day cut, chain after chain (k_oc_days)            {stats(split['u'][1])}",
             f"    moments (k_sc_nat / _sum / _gram / _finish_*; HIP events) {stats(split['u'][3])}",
             f"    counting (k_oc_count, HIP events)                 {stats(split['u'][4])}",
             f"potus_scenario given {quarter[i]} of {states[i]} and the national vote within mean +- 0.674 sd (a normal's quartiles): kept {rc.n_kept} of {rc.n_draws}",
             f"                                                      {stats(calls['c'])}",
             f"    produce + gather predicted_score                  {stats(split['c'][0])}",
             f"    day cut, chain after chain (k_oc_days)            {stats(split['c'][1])}",
             f"    keep + compact (k_sc_keep, k_sc_scan, k_sc_compact) {stats(split['c'][2])}",
             f"    moments (HIP events)                              {stats(split['c'][3])}",
             f"    counting (k_oc_count, HIP events)                 {stats(split['c'][4])}",
             f"potus_outcomes, the same handles                      {stats(calls['o'])}",
             f"    counting (k_oc_count, HIP events)                 {stats(calls['o_count'])}",
             f"host route, once: potus_extract_matrix {(t1 - t0) * 1e3:.0f} ms, then tests/scenario_ref.py on ELECTION DAY ALONE {(t2 - t1) * 1e3:.0f} ms;",
             f"    its counts equal the conditional call's: {'yes' if same else 'NO'}; max |cov - ref| / (sd_i sd_j) = {cov_err:.2e}", "",
             f"gate: moments without a condition, median {med['u'][3]:.3f} <= k_oc_count on the same block in the same run, median {med['u'][4]:.3f}: "
             f"{'ok' if med['u'][3] <= med['u'][4] else 'NOT MET'}",
             f"the moments read the block three times (k_sc_nat, k_sc_sum, k_sc_gram): {3 * block_bytes / 1e9:.2f} GB in {med['u'][3]:.3f} ms = "
             f"{3 * block_bytes / (med['u'][3] * 1e-3) / 1e12:.3f} TB/s, {100 * 3 * block_bytes / (med['u'][3] * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak",
             ""]
    assert ru.n_kept == nd
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=("2016", "2012", "2008"), default="2016")
    ap.add_argument("--given", default="FL=lose,PA=lose,national=0.48:0.52")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--out", default=None, help="default: profiles/scenario_<design>.txt")
    a = ap.parse_args(argv)
    import torch
    torch.cuda.init()                                  # torch's GPU runtime first, as bench.py does
    npz = dataprep.load_npz(ROOT / "tests" / "golden" / f"data_{a.design}.npz")
    data, meta = npz["data"], npz["meta"]
    states, ev = [str(s) for s in meta["states"]], np.asarray(meta["ev_state"], dtype=np.int64)
    t0 = time.perf_counter()
    fit = PotusModel(VARIANT[a.design]).sample(data, seed=a.seed, chains=a.chains, iter_warmup=a.warmup, iter_sampling=a.samples, refresh=0)
    t_fit = time.perf_counter() - t0
    lines = [f"# conditional forecast: design {a.design} ({VARIANT[a.design]}), {a.chains} chains, warm-up {a.warmup}, sampling {a.samples}, seed {a.seed} "
             f"(fit {t_fit:.1f} s)", ""]
    lines += report(a, data, states, ev, fit)
    if not a.no_timing:
        lines += timing(a, data, states, ev, fit)
    text = "\n".join(lines)
    print(text, end="")
    out = Path(a.out) if a.out else ROOT / "profiles" / f"scenario_{a.design}.txt"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
