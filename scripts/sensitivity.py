#!/usr/bin/env python3
"""Prior sensitivity by refit: the one-at-a-time grid of the nine prior scales fitted as chains of one launch and compared with the
baseline on the device, next to the loop of stand-alone fits it replaces (us_potus_model_amd.sensitivity).

  python scripts/sensitivity.py --design 2016 --chains 4 [--warmup 200 --samples 200] [--no-loop] [--loo] > profiles/sensitivity_2016.txt

The settings are the ten cases of scripts/pin_sensitivity.py (the data as given and one scale changed at a time: sigma_e_bias x 2, the
others x 1.5) plus the null copy -- the data as given once more, with other chains -- whose distance to the baseline is the Monte-Carlo
floor.  --design small: the same grid on the synthetic design.  Prints the wall time of the one launch, of the loop of stand-alone handles
that gives the same bytes (one workgroup per chain) and of the loop in the layout the library picks for that many chains (both skipped with
--no-loop), potus_grid_compare's kernel times, and per setting the election-day distances with what is flagged."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from us_potus_model_amd import dataprep, sensitivity, synthetic, timeline  # noqa: E402
from us_potus_model_amd.sampler import Handle  # noqa: E402

SCALES = {"sigma_m": [1.5], "sigma_pop": [1.5], "sigma_c": [1.5], "sigma_e_bias": [2.0], "sigma_measure_noise_state": [1.5],
          "sigma_measure_noise_national": [1.5], "polling_bias_scale": [1.5], "random_walk_scale": [1.5], "mu_b_T_scale": [1.5]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=["2016", "small"], default="2016")
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--no-loop", action="store_true", help="skip the two loops of stand-alone fits")
    ap.add_argument("--loo", action="store_true", help="PSIS-LOO per setting (Grid.loo) and loo_compare")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    if a.design == "2016":
        built = dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")
        data, ev = built["data"], np.asarray(built["meta"]["ev_state"], dtype=np.float64)
    else:
        data, ev = synthetic.small("full"), np.array([100, 90, 80, 70, 60, 138.0])
    design = sensitivity.grid(data, SCALES)
    n, S = design["scales"].shape[0], int(data["S"])
    opts = dict(num_warmup=a.warmup, num_samples=a.samples, seed=a.seed)
    print(f"design {a.design}: {n} settings x {a.chains} chains, {a.warmup} + {a.samples} transitions, {a.chains * a.samples} draws per setting, seed {a.seed}")

    t0 = time.perf_counter()
    g = sensitivity.fit(design, "full", a.chains, **opts)
    wall_one = time.perf_counter() - t0
    lf_one = g.handle.total_leapfrogs()
    print(f"one launch      : {wall_one:8.2f} s wall ({g.wall_s:.2f} s init + run), {lf_one} leapfrogs, {lf_one / g.wall_s / 1e3:.1f} k leapfrogs/s")
    failed = [c for c, s in enumerate(g.handle.chain_status()[0]) if s != 0]
    print(f"failed chains   : {failed if failed else 'none'}")

    t0 = time.perf_counter()
    c = g.compare(ev)
    wall_cmp = time.perf_counter() - t0
    print(f"potus_grid_compare: {wall_cmp * 1e3:6.2f} ms wall (election day, {n} settings x {S + 2} columns; kernels: scores {c.timing['scores_ms']:.3f} ms, "
          f"k_sg_grid {c.timing['distance_ms']:.3f} ms)")
    x = g.handle.timeline_scores_device()
    per = x.shape[1]
    from us_potus_model_amd.sampler import ecdf_distance_device
    ecdf_distance_device(x[2].reshape(per, S), x[0].reshape(per, S))
    ms = g.handle.grid_timing()["distance_ms"]
    print(f"k_sg_distance   : {ms:8.3f} ms for the {S} state columns of one setting against the baseline ({per} + {per} draws per column)")
    fl = c.flag()
    k = c.kind_of_column
    print(f"floor (null copy), election day: largest state cjs {c.floor_of_kind()[0, 0]:.4f}, national {c.floor_of_kind()[0, 1]:.4f}, "
          f"electoral votes {c.floor_of_kind()[0, 2]:.4f}")
    print(c.table())
    print("flagged (sensitivity = cjs / |log2 factor| >= 0.05 and cjs above the largest floor of the column's kind), election day:")
    for d, lab in enumerate(design["labels"]):
        if fl[d, 0].any():
            print(f"  {lab:40s} {int(fl[d, 0][k == 0].sum()):2d} of {S} states, national {'yes' if fl[d, 0][k == 1][0] else 'no'}, "
                  f"electoral votes {'yes' if fl[d, 0][k == 2][0] else 'no'}")
    if not fl[:, 0].any():
        print("  none")
    s = g.summary(ev)
    print("setting                                      national vote (low, mean, high)   EV mean  P(win)   rhat_max  ess_bulk_min")
    for d, lab in enumerate(design["labels"]):
        na, e = s["national"][d, 0], s["electoral_votes"][d, 0]
        print(f"{lab:44s} {na[0]:.4f} {na[2]:.4f} {na[1]:.4f}            {e[0]:7.1f}  {e[4]:.3f}    {s['rhat_max'][d]:.3f}   {s['ess_bulk_min'][d]:.0f}")
    if a.loo:
        from us_potus_model_amd import loo
        t0 = time.perf_counter()
        ls = g.loo()
        print(f"Grid.loo        : {time.perf_counter() - t0:8.2f} s wall, {n} settings")
        for o in ls:
            print(f"  {o.name:40s} elpd_loo {o.elpd_loo:10.1f} (SE {o.se_elpd_loo:.1f})  k: {o.pareto_k_table()}")
        print(loo.loo_compare(*ls))
    g.close()

    if not a.no_loop:
        for what, layout in (("one workgroup per chain: the bytes of the one launch", dict(cus_per_chain=1, twin=0)), ("the layout the library picks", {})):
            t0 = time.perf_counter()
            lf = 0
            for d in range(n):
                h = Handle(timeline.data_of(design, d), "full", chains=a.chains, chain_id_offset=d * a.chains, **layout, **opts)
                h.init()
                h.run(a.warmup + a.samples)
                lf += h.total_leapfrogs()
                kk = (h.cus_per_chain, h.clusters_per_chain)
                h.close()
            wall_loop = time.perf_counter() - t0
            print(f"loop of {n} stand-alone {a.chains}-chain fits, {what} ({kk[0]} workgroup(s) x {kk[1]} cluster(s) per chain): "
                  f"{wall_loop:8.2f} s wall, {lf} leapfrogs, {lf / wall_loop / 1e3:.1f} k leapfrogs/s; loop / one launch: {wall_loop / wall_one:.2f} x")


if __name__ == "__main__":
    main()
