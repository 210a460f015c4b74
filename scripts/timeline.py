#!/usr/bin/env python3
"""The forecast timeline of a campaign: N run dates fitted as chains of one launch and summarised on the device, next to the loop of
stand-alone fits it replaces (us_potus_model_amd.timeline).

  python scripts/timeline.py --design 2016 --dates 32 --chains 4 [--warmup 200 --samples 200] [--no-loop] [--lfo]

Reads tests/golden/data_2016.npz and tests/golden/timeline_2016.npz (the masks, priors and scales of 32 run dates, every fourth day up to
election day; scripts/make_timeline_fixture.py).  --design small: four data sets of the synthetic design instead.
Prints the wall time of the one-launch fit, of the loop of stand-alone fits of the same dates (skipped with --no-loop), potus_timeline's
kernel times next to the numpy restatement's, and the election-day forecast per run date.  --lfo adds leave-future-out (Timeline.lfo,
DESIGN.md section 4j): per run date the exact log predictive density of the polls that arrived before the next run date, under the date's
own draws, with no refit."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from us_potus_model_amd import dataprep, synthetic, timeline  # noqa: E402
from us_potus_model_amd.sampler import Handle  # noqa: E402


def load(design, n_dates):
    if design == "2016":
        built = dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")
        d = timeline.load_fixture(ROOT / "tests" / "golden" / "timeline_2016.npz", built["data"], built["meta"])
        ev, variant = np.asarray(built["meta"]["ev_state"], dtype=np.float64), "full"
    else:
        data = synthetic.small("full")
        Ns, Nn = int(data["N_state_polls"]), int(data["N_national_polls"])
        cut = np.linspace(6, int(data["T"]), 4).astype(int)
        d = timeline.design_of(data, np.asarray(data["day_state"])[None] <= cut[:, None], np.asarray(data["day_national"])[None] <= cut[:, None],
                               np.tile(data["mu_b_prior"], (4, 1)), data["mu_b_T_scale"] * np.linspace(1.5, 1.0, 4), [f"day {c}" for c in cut])
        assert d["keep_state"].shape == (4, Ns) and d["keep_national"].shape == (4, Nn)
        ev, variant = np.array([100, 90, 80, 70, 60, 138.0]), "full"
    n = d["keep_state"].shape[0]
    if not 1 <= n_dates <= n:
        raise SystemExit(f"--dates {n_dates}: the design holds {n} run dates")
    sel = np.unique(np.round(np.linspace(0, n - 1, n_dates)).astype(int))
    d = timeline.design_of(d["data"], d["keep_state"][sel], d["keep_national"][sel], d["mu_b_prior"][sel], d["mu_b_T_scale"][sel],
                           [d["run_dates"][i] for i in sel], d["meta"])
    return d, variant, ev


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=["2016", "small"], default="2016")
    ap.add_argument("--dates", type=int, default=32)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--no-loop", action="store_true", help="skip the loop of stand-alone fits")
    ap.add_argument("--lfo", action="store_true", help="leave-future-out: score every run date on the polls that arrived before the next one")
    ap.add_argument("--loop-one-workgroup", action="store_true", help="the loop's fits with one workgroup per chain (the bytes of the one launch) "
                                                                      "instead of the layout the library picks for a 4-chain handle")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    design, variant, ev = load(a.design, a.dates)
    n, T = design["keep_state"].shape[0], int(design["data"]["T"])
    opts = dict(num_warmup=a.warmup, num_samples=a.samples, seed=a.seed)
    print(f"design {a.design}: {n} run dates x {a.chains} chains, {a.warmup} + {a.samples} transitions, T = {T}")

    t0 = time.perf_counter()
    tl = timeline.fit(design, variant, a.chains, **opts)
    wall_one = time.perf_counter() - t0
    lf_one = tl.handle.total_leapfrogs()
    print(f"one launch      : {wall_one:8.2f} s wall ({tl.wall_s:.2f} s init + run), {lf_one} leapfrogs, {lf_one / tl.wall_s / 1e3:.1f} k leapfrogs/s")

    t0 = time.perf_counter()
    s = tl.summary(ev, diagnostics=False)
    wall_sum = time.perf_counter() - t0
    ms = s["timing"]
    print(f"potus_timeline  : {wall_sum * 1e3:8.2f} ms wall (election day; kernels: scores {ms['scores_ms']:.3f} ms, summary {ms['summary_ms']:.3f} ms)")
    import timeline_ref
    x = tl.handle.timeline_scores_device().cpu().numpy()
    t0 = time.perf_counter()
    ref = [timeline_ref.summary(x[d], design["data"]["state_weights"], ev) for d in range(n) if s["n_draws"][d]]
    print(f"numpy restatement: {(time.perf_counter() - t0) * 1e3:7.2f} ms (scores already on the host)")
    ok = [d for d in range(n) if s["n_draws"][d]]
    err = max(np.abs(s["state"][d][..., [0, 1, 3]] - ref[i]["state"][..., [0, 1, 3]]).max() for i, d in enumerate(ok)) if ok else float("nan")
    print(f"max |device - numpy| over quantiles and probabilities: {err:.3g}")
    sd = tl.summary(ev)
    print("run date     polls  national vote (low, mean, high)   EV mean  P(win)   rhat_max  ess_bulk_min")
    for d in range(n):
        na, e = s["national"][d, 0], s["electoral_votes"][d, 0]
        polls = int(design["keep_state"][d].sum() + design["keep_national"][d].sum())
        print(f"{str(design['run_dates'][d]):12s} {polls:5d}  {na[0]:.4f} {na[2]:.4f} {na[1]:.4f}            {e[0]:7.1f}  {e[4]:.3f}    {sd['rhat_max'][d]:.3f}   {sd['ess_bulk_min'][d]:.0f}")
    if a.lfo:
        t0 = time.perf_counter()
        f = tl.lfo()
        wall_lfo = time.perf_counter() - t0
        ms = tl.handle.cv_timing()
        print(f"leave-future-out: {wall_lfo * 1e3:8.2f} ms wall, one potus_cv_lpd call, {int(f['n_held'].sum())} (date, poll) pairs "
              f"(kernels: k_cv_loglik {ms['loglik_ms']:.3f} ms, k_cv_reduce {ms['reduce_ms']:.3f} ms)")
        print("run date     polls arriving before the next date   elpd (sum)   elpd per poll")
        for d in range(n):
            k = int(f["n_held"][d])
            print(f"{str(design['run_dates'][d]):12s} {k:5d}                                 {f['elpd'][d]:10.2f}   {f['elpd'][d] / k if k else float('nan'):8.3f}")
        print(f"total: {int(f['n_held'].sum())} polls, elpd_lfo {np.nansum(f['elpd']):.1f}")
    tl.close()

    if not a.no_loop:
        t0 = time.perf_counter()
        lf = 0
        layout = dict(cus_per_chain=1, twin=0) if a.loop_one_workgroup else {}
        for d in range(n):
            h = Handle(timeline.data_of(design, d), variant, chains=a.chains, chain_id_offset=d * a.chains, **layout, **opts)
            h.init()
            h.run(a.warmup + a.samples)
            h.posterior_summary(ev)
            lf += h.total_leapfrogs()
            k = (h.cus_per_chain, h.clusters_per_chain)
            h.close()
        wall_loop = time.perf_counter() - t0
        print(f"loop of {n} stand-alone {a.chains}-chain fits ({k[0]} workgroup(s) x {k[1]} cluster(s) per chain, with potus_posterior_summary): "
              f"{wall_loop:8.2f} s wall, {lf} leapfrogs, {lf / wall_loop / 1e3:.1f} k leapfrogs/s")
        print(f"one launch / loop: {wall_loop / wall_one:.2f} x")


if __name__ == "__main__":
    main()
