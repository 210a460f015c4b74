#!/usr/bin/env python3
"""Pathfinder on the device (potus_pathfinder): the stage times, where l* sits, the agreement with NUTS.

  python scripts/pathfinder.py --design 2016 --paths 8 --draws 1000 [--timeline 32] [--out profiles/pathfinder_2016.txt]

Reads tests/golden/data_<design>.npz (--design small: the synthetic design).  Writes -- to --out, default profiles/pathfinder_<design>.txt --
  * the stage times of potus_pathfinder_timing (HIP events; one warm-up call, then --reps calls, the median) for --paths paths of --draws draws
    each, the microseconds per model pass inside k_pf_elbo, and the wall time of the call;
  * per path: the iterations, l*, the ELBO there;
  * k-hat and the sd of the log importance ratio lp - lq over the pooled draws;
  * the election-day state means and 95 % intervals over the pooled draws against tests/golden/posterior_<design>.npz in units of its MCSE;
  * --timeline N: timeline.pathfinder on N run dates of tests/golden/timeline_2016.npz, wall time;
  * --inits: the warm-up leapfrogs of the headline configuration (8 chains, 1000 warm-up transitions, the library's own layout) started from
    PotusModel.pathfinder(paths=8, draws=1000).inits(8, seed=0) against the default U(-2, 2) starts."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from us_potus_model_amd import dataprep, synthetic, timeline  # noqa: E402
from us_potus_model_amd.sampler import Handle, Pathfinder, PotusModel  # noqa: E402

VARIANT = {"2016": "full", "2012": "no_mode_adjustment", "2008": "no_mode_adjustment", "small": "full"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=list(VARIANT), default="2016")
    ap.add_argument("--paths", type=int, default=8)
    ap.add_argument("--draws", type=int, default=1000, help="draws per path")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeline", type=int, default=0)
    ap.add_argument("--timeline-draws", type=int, default=1000)
    ap.add_argument("--inits", action="store_true")
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
    say(f"Pathfinder, design {a.design} ({variant}), D = {D}: {a.paths} paths x {a.draws} draws, history_size 6, 25 ELBO draws, max_lbfgs_iters 1000")
    ms, wall, res = [], [], None
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        res = hd.pathfinder(None, a.paths, num_draws=a.draws)
        if rep:
            wall.append(time.perf_counter() - t0)
            ms.append(hd.pathfinder_timing())
    med = {k: float(np.median([m[k] for m in ms])) for k in ms[0]}
    items = int(res["iterations"].sum())
    G = torch.cuda.get_device_properties(0).multi_processor_count
    seq = -(-items // G) * 25
    say(f"  L-BFGS (k_opt_lbfgs with the trajectory): {med['lbfgs_ms']:.1f} ms; alpha (k_pf_alpha): {med['alpha_ms']:.2f} ms")
    say(f"  ELBO (k_pf_elbo): {med['elbo_ms']:.1f} ms: {items} iterates x 25 draws = {items * 25} model passes on G = {G} workgroups, {seq} in a workgroup's sequence = "
        f"{med['elbo_ms'] * 1e3 / max(seq, 1):.0f} us per pass with the fit's share (Gram sums, QR, Cholesky once per 25 passes)")
    say(f"  draws (k_pf_draws): {med['draws_ms']:.1f} ms for {a.paths * a.draws} draws")
    say(f"  the call: {np.median(wall) * 1e3:.0f} ms wall (with {a.paths * a.draws * D * 8 / 1e9:.2f} GB of draws copied to the host); the stages sum to {sum(med.values()):.0f} ms")
    for p in range(a.paths):
        l = int(res["best_iteration"][p])
        say(f"  path {p}: code {int(res['return_code'][p])}, optimiser code {int(res['optimize_code'][p])}, L = {int(res['iterations'][p])}, l* = {l}, "
            f"ELBO {res['elbo'][p, l] if l else float('nan'):.2f}, kept pairs {int(res['kept'][p].sum())}")
    pf = Pathfinder(hd, res)
    lr = pf.log_ratio[np.isfinite(pf.log_ratio)]
    say(f"  log importance ratio over the {lr.size} pooled draws: mean {lr.mean():.3f}, sd {lr.std():.3f}, max {lr.max():.2f}; Pareto k-hat {pf.pareto_k:.3f}")
    per = (res["lp"] - res["lq"])
    say("  per path: sd of the log ratio " + ", ".join(f"{np.nanstd(r):.2f}" for r in per))

    gold = ROOT / "tests" / "golden" / f"posterior_{a.design}.npz"
    if gold.exists():
        g = np.load(gold)
        sc = pf.scores().cpu().numpy()[:, 0, :]
        sc = sc[np.isfinite(sc).all(1)]
        mc = g["predicted_score_T__mcse"]
        say(f"\nelection-day predicted_score over the pooled draws against the NUTS fit of tests/golden/{gold.name} (its MCSE of the mean: {mc.min():.2e} .. {mc.max():.2e}):")
        for name, mine, ref in (("mean", sc.mean(0), g["predicted_score_T__mean"]), ("2.5 %", np.quantile(sc, 0.025, axis=0), g["predicted_score_T__q025"]),
                                ("97.5 %", np.quantile(sc, 0.975, axis=0), g["predicted_score_T__q975"])):
            d = np.abs(mine - ref)
            say(f"  {name}: largest difference {d.max():.5f} = {(d / mc).max():.1f} MCSE (state {int(np.argmax(d / mc))}); mean difference {d.mean():.5f}")
    hd.close()

    if a.timeline:
        d16 = dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")["data"]
        full = timeline.load_fixture(ROOT / "tests" / "golden" / "timeline_2016.npz", d16)
        n = min(a.timeline, full["keep_state"].shape[0])
        pick = np.unique(np.linspace(0, full["keep_state"].shape[0] - 1, n).round().astype(int))
        design = timeline.design_of(d16, full["keep_state"][pick], full["keep_national"][pick], full["mu_b_prior"][pick], full["mu_b_T_scale"][pick],
                                    [full["run_dates"][i] for i in pick])
        t0 = time.perf_counter()
        out = timeline.pathfinder(design, "full", draws=a.timeline_draws, ev=np.ones(int(d16["S"])), seed=a.seed)
        w = time.perf_counter() - t0
        tm = out["timing"]
        say(f"\ntimeline.pathfinder: {len(pick)} run dates of the 2016 campaign, one path of {a.timeline_draws} draws each: {w:.2f} s wall with the handle's set-up; "
            f"L-BFGS {tm['lbfgs_ms']:.0f} ms, alpha {tm['alpha_ms']:.1f} ms, ELBO {tm['elbo_ms']:.0f} ms, draws {tm['draws_ms']:.0f} ms")
        say(f"  codes {sorted(set(int(c) for c in out['return_code'].ravel()))}, l* {out['best_iteration'].min()} .. {out['best_iteration'].max()} of "
            f"{out['iterations'].min()} .. {out['iterations'].max()}, log ratio sd per date {np.nanstd(out['log_ratio'], axis=2).min():.2f} .. {np.nanstd(out['log_ratio'], axis=2).max():.2f}")
        say("  national vote, mean [2.5 %, 97.5 %] by run date: " + ", ".join(
            f"{d} {v[2]:.4f} [{v[0]:.4f}, {v[1]:.4f}]" for d, v in list(zip(out["run_dates"], out["national"][:, 0, 0]))[::max(len(pick) // 8, 1)]))
    if a.inits:
        t0 = time.perf_counter()
        pfm = PotusModel(variant).pathfinder(data, paths=8, draws=1000, seed=a.seed)
        w = time.perf_counter() - t0
        init = pfm.inits(8, seed=0)
        pfm.close()
        say(f"\nwarm-up of the headline configuration ({a.design}, 8 chains, 1000 warm-up transitions, seed {a.seed}); PotusModel.pathfinder(paths=8, draws=1000): {w:.2f} s wall")
        for name, q0 in (("default inits U(-2, 2)", None), ("Pathfinder.inits(8, seed=0)", init)):
            hs = Handle(data, variant, chains=8, num_warmup=1000, num_samples=0, seed=a.seed)
            hs.init(q0)
            t0 = time.perf_counter()
            hs.run(1000)
            say(f"  {name}: {hs.total_leapfrogs()} leapfrogs, {time.perf_counter() - t0:.2f} s, chain status {hs.chain_status()[0]}")
            hs.close()
    path = Path(a.out) if a.out else ROOT / "profiles" / f"pathfinder_{a.design}.txt"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
