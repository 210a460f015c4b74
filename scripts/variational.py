#!/usr/bin/env python3
"""Mean-field ADVI on the device (potus_advi): the stage times, where the runs stop, the agreement with NUTS.

  python scripts/variational.py --design 2016 --runs 8 --draws 1000 [--timeline 32] [--out profiles/variational_2016.txt]

Reads tests/golden/data_<design>.npz (--design small: the synthetic design).  Writes -- to --out, default profiles/variational_<design>.txt --
for each tol_rel_obj of --tols (default: CmdStan's 0.01, then 0.001):
  * the stage times of potus_advi_timing (HIP events; one warm-up call, then --reps calls, the median) for --runs runs of --draws draws each,
    and the wall time of the call;
  * the same call with the ELBO evaluations inside as many workgroups as there are tracks (POTUS_ADVI_G = the tracks of the largest launch)
    instead of on the chip-wide grid: the ELBO stage's time, and the cost of the gradient steps between two evaluations to set it against;
  * per run: the code, the iterations, eta*, the last ELBO;
  * k-hat and the sd of the log importance ratio lp - lq over the pooled draws;
  * the election-day state means and 95 % intervals over the pooled draws against tests/golden/posterior_<design>.npz in units of its MCSE;
and with --timeline N: timeline.variational on N run dates of tests/golden/timeline_2016.npz, wall time."""
import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from us_potus_model_amd import _abi, dataprep, synthetic, timeline  # noqa: E402
from us_potus_model_amd.sampler import Handle, Variational  # noqa: E402

VARIANT = {"2016": "full", "2012": "no_mode_adjustment", "2008": "no_mode_adjustment", "small": "full"}


def timed(hd, reps, **kw):
    ms, wall, res = [], [], None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        res = hd.variational(**kw)
        if rep:
            wall.append(time.perf_counter() - t0)
            ms.append(hd.variational_timing())
    return {k: float(np.median([m[k] for m in ms])) for k in ms[0]}, float(np.median(wall)), res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=list(VARIANT), default="2016")
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--draws", type=int, default=1000, help="draws per run")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tols", type=float, nargs="+", default=[0.01, 0.001])
    ap.add_argument("--iter", type=int, default=10000)
    ap.add_argument("--timeline", type=int, default=0)
    ap.add_argument("--timeline-draws", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    variant = VARIANT[a.design]
    data = synthetic.small("full") if a.design == "small" else dataprep.load_npz(ROOT / "tests" / "golden" / f"data_{a.design}.npz")["data"]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    hd = Handle(data, variant, chains=1, num_warmup=0, num_samples=0, seed=a.seed, cus_per_chain=1, twin=0)
    D = hd.D
    G = torch.cuda.get_device_properties(0).multi_processor_count
    gold = ROOT / "tests" / "golden" / f"posterior_{a.design}.npz"
    say(f"mean-field ADVI, design {a.design} ({variant}), D = {D}: {a.runs} runs x {a.draws} draws, CmdStan's defaults (iter {a.iter}, grad_samples 1, "
        f"elbo_samples 100, eval_elbo 100, adapt_iter 50); HIP events, the median of {a.reps} calls after a warm-up call")
    for tol in a.tols:
        kw = dict(q0=None, runs=a.runs, output_samples=a.draws, tol_rel_obj=tol, iter=a.iter)
        os.environ.pop("POTUS_ADVI_G", None)
        med, wall, res = timed(hd, a.reps, **kw)
        ev = int(res["evaluations"].max())
        say(f"\ntol_rel_obj = {tol}:")
        say(f"  adaptation (k_vi_sga, {5 * a.runs} tracks x 50 steps at once): {med['adapt_ms']:.1f} ms")
        say(f"  gradient segments (k_vi_sga, {a.runs} tracks, {ev} segments of 100 steps): {med['grad_ms']:.1f} ms = {med['grad_ms'] * 1e3 / max(ev * 100, 1):.0f} us per step")
        say(f"  ELBO (k_vi_elbo on G = {G} workgroups, {ev + 1} launches; the first over {6 * a.runs} tracks x 100 draws): {med['elbo_ms']:.1f} ms")
        say(f"  draws (k_vi_draws and k_lap_lp): {med['draws_ms']:.1f} ms for {a.runs * a.draws} draws")
        say(f"  the call: {wall * 1e3:.0f} ms wall (with {a.runs * a.draws * D * 8 / 1e9:.2f} GB of draws copied to the host); the stages sum to {sum(med.values()):.0f} ms")
        # the design's argument: the evaluations on the chip-wide grid against the same evaluations at the cost of one workgroup per track.
        # Without the adaptation every ELBO launch is over the --runs main tracks, so G = --runs gives each workgroup one track's share.
        ok = res["eta_index"] >= 0
        eta = float(np.median(res["eta"][ok])) if ok.any() else 1.0
        kw0 = dict(kw, adapt_engaged=0, eta=eta)
        med0, _, res0 = timed(hd, a.reps, **kw0)
        os.environ["POTUS_ADVI_G"] = str(a.runs)
        med1, _, res1 = timed(hd, a.reps, **kw0)
        os.environ.pop("POTUS_ADVI_G", None)
        same = all(np.array_equal(res0[k], res1[k], equal_nan=True) for k in ("mu", "omega", "elbo", "q", "lp", "lq"))
        ev0 = int(res0["evaluations"].max())
        say(f"  without the adaptation (eta = {eta:g}; {ev0 + 1} ELBO launches over the {a.runs} main tracks x 100 draws, {ev0} segments): ELBO {med0['elbo_ms']:.1f} ms on G = {G} "
            f"workgroups, {med1['elbo_ms']:.1f} ms on G = {a.runs} (a track's 100 draws in one workgroup) = {med0['elbo_ms'] / (ev0 + 1):.2f} against "
            f"{med1['elbo_ms'] / (ev0 + 1):.2f} ms per evaluation; the 100 gradient steps between two evaluations cost {med0['grad_ms'] / max(ev0, 1):.2f} ms; outputs equal: {same}")
        for r in range(a.runs):
            say(f"  run {r}: code {_abi.ADVI_CODES[int(res['return_code'][r])]}, flags {int(res['flags'][r])}, {int(res['iterations'][r])} iterations, eta* {res['eta'][r]:g}, "
                f"ELBO {res['elbo'][r, int(res['evaluations'][r])]:.2f} (initial {res['elbo'][r, 0]:.2f}), {int(res['model_passes'][r])} model passes")
        vi = Variational(hd, res)
        lr = vi.log_ratio[np.isfinite(vi.log_ratio)]
        say(f"  log importance ratio over the {lr.size} pooled draws: mean {lr.mean():.3f}, sd {lr.std():.3f}, max {lr.max():.2f}; Pareto k-hat {vi.pareto_k:.3f}")
        say("  per run: sd of the log ratio " + ", ".join(f"{np.nanstd(r):.2f}" for r in (res["lp"] - res["lq"])))
        say(f"  sd = exp(omega) over the coordinates: {vi.sd.min():.3g} .. {vi.sd.max():.3g}, median {np.median(vi.sd):.3g}")
        if gold.exists():
            g = np.load(gold)
            sc = vi.scores().cpu().numpy()[:, 0, :]
            sc = sc[np.isfinite(sc).all(1)]
            mc = g["predicted_score_T__mcse"]
            say(f"  election-day predicted_score over the pooled draws against the NUTS fit of tests/golden/{gold.name} (its MCSE of the mean: {mc.min():.2e} .. {mc.max():.2e}):")
            for name, mine, ref in (("mean", sc.mean(0), g["predicted_score_T__mean"]), ("2.5 %", np.quantile(sc, 0.025, axis=0), g["predicted_score_T__q025"]),
                                    ("97.5 %", np.quantile(sc, 0.975, axis=0), g["predicted_score_T__q975"])):
                d = np.abs(mine - ref)
                say(f"    {name}: largest difference {d.max():.5f} = {(d / mc).max():.1f} MCSE (state {int(np.argmax(d / mc))}); mean difference {d.mean():.5f}")
    hd.close()

    if a.timeline:
        d16 = dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")["data"]
        full = timeline.load_fixture(ROOT / "tests" / "golden" / "timeline_2016.npz", d16)
        n = min(a.timeline, full["keep_state"].shape[0])
        pick = np.unique(np.linspace(0, full["keep_state"].shape[0] - 1, n).round().astype(int))
        design = timeline.design_of(d16, full["keep_state"][pick], full["keep_national"][pick], full["mu_b_prior"][pick], full["mu_b_T_scale"][pick],
                                    [full["run_dates"][i] for i in pick])
        for tol in a.tols:
            t0 = time.perf_counter()
            out = timeline.variational(design, "full", draws=a.timeline_draws, ev=np.ones(int(d16["S"])), seed=a.seed, tol_rel_obj=tol, iter=a.iter)
            w = time.perf_counter() - t0
            tm = out["timing"]
            say(f"\ntimeline.variational, tol_rel_obj = {tol}: {len(pick)} run dates of the 2016 campaign, one run of {a.timeline_draws} draws each: {w:.2f} s wall with the "
                f"handle's set-up; adaptation {tm['adapt_ms']:.0f} ms, gradient segments {tm['grad_ms']:.0f} ms, ELBO {tm['elbo_ms']:.0f} ms, draws {tm['draws_ms']:.0f} ms")
            say(f"  codes {sorted(set(int(c) for c in out['return_code'].ravel()))}, iterations {out['iterations'].min()} .. {out['iterations'].max()}, eta* "
                f"{sorted(set(float(e) for e in out['eta'].ravel()))}, log ratio sd per date {np.nanstd(out['log_ratio'], axis=2).min():.2f} .. {np.nanstd(out['log_ratio'], axis=2).max():.2f}")
            say("  national vote, mean [2.5 %, 97.5 %] by run date: " + ", ".join(
                f"{d} {v[2]:.4f} [{v[0]:.4f}, {v[1]:.4f}]" for d, v in list(zip(out["run_dates"], out["national"][:, 0, 0]))[::max(len(pick) // 8, 1)]))
    path = Path(a.out) if a.out else ROOT / "profiles" / f"variational_{a.design}.txt"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
