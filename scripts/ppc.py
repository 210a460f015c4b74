#!/usr/bin/env python3
"""Posterior predictive checks of a fit (us_potus_model_amd/ppc.py): the LOO-PIT histogram and coverage, the groups of
polls whose bias, dispersion or count the model cannot reproduce, for both model variants on the same polls, and the stage timings of
potus_ppc next to the numpy restatement (tests/ppc_ref.py) on blocks copied to the host.

    python scripts/ppc.py --design 2016 --chains 8 --warmup 1000 --samples 1000 --out profiles/ppc_2016.txt
"""
import argparse
import ctypes
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import ppc_ref  # noqa: E402
from us_potus_model_amd import dataprep, loo, ppc, synthetic  # noqa: E402
from us_potus_model_amd.sampler import Handle  # noqa: E402

VARIANTS = ("full", "no_mode_adjustment")


def extra_groups(data):
    """mode and population of every poll from the data list, for the variant that does not model them"""
    out = {}
    for name, key, cnt in (("mode", "poll_mode", "M"), ("population", "poll_pop", "Pop")):
        if f"{key}_state" in data:
            lab = np.concatenate([np.asarray(data[f"{key}_state"]), np.asarray(data[f"{key}_national"])]).astype(np.int64) - 1
            out[name] = (lab, [str(k + 1) for k in range(int(lab.max()) + 1)])
    return out


def host_restatement(h, ck, gs):
    """the blocks of the device copied to the host, then tests/ppc_ref.py on them: (seconds of the PIT sums, of the group sums and tables, largest
    differences against the device)"""
    N = h.n_polls
    y, n = (a.astype(np.float64) for a in loo.poll_vectors(h.data))
    blocks = list(loo._pooled_ratio_blocks([h], True))
    import torch
    r = torch.cat([b[2] for b in blocks])
    re = np.concatenate([b[3][:, 4] for b in blocks])
    lw, _ = loo.psis_weights(r, np.where(np.isfinite(re) & (re > 0), re, 1.0))
    lw = lw.reshape(N, -1).cpu().numpy()
    del r, blocks
    a1, a2 = (t.reshape(N, -1).cpu().numpy() for t in h.poll_share_device(0, N, integrate=True))
    yr = h.poll_rep_device(0, N, integrate=True).reshape(N, -1).cpu().numpy()
    t0 = time.perf_counter()
    lo, eq = ppc_ref.pit_sums(yr, y)
    llo, leq = ppc_ref.pit_sums(yr, y, lw)
    t_pit = time.perf_counter() - t0
    t0 = time.perf_counter()
    worst = 0.0
    for name, (lab, names) in gs.items():
        T, cnt = ppc_ref.group_sums(yr, a1, a2, y, n, lab, len(names))
        tab = ppc_ref.group_table(T, cnt)
        g = ck.groups[name]
        used = cnt > 0
        worst = max(worst, float(np.abs(tab[used, :, 5] - np.stack([g["p_bias"], g["p_dispersion"], g["p_count"]], axis=1)[used]).max()))
    t_grp = time.perf_counter() - t0
    ok = n > 0
    d_pit = max(float(np.abs(lo[ok] - ck.pit_lo[ok]).max()), float(np.abs(llo[ok] - ck.loo_pit_lo[ok]).max()), float(np.abs(leq[ok] - ck.loo_pit_eq[ok]).max()))
    return t_pit, t_grp, d_pit, worst


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=("2016", "small"), default="small")
    ap.add_argument("--variant", default=None, help="one variant (default: both, on the same polls)")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--alpha", type=float, default=0.01)
    ap.add_argument("--out", default=None, help="the report's file (default for --design 2016: profiles/ppc_2016.txt)")
    a = ap.parse_args(argv)
    if a.out is None and a.design == "2016":
        a.out = str(ROOT / "profiles" / "ppc_2016.txt")
    import torch
    torch.cuda.init()
    if a.design == "small":
        data, pollsters = synthetic.small("full"), None
    else:
        z = dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")
        data, pollsters = z["data"], [str(p) for p in z["meta"]["pollsters"]]
    N = int(data["N_state_polls"]) + int(data["N_national_polls"])
    lines = [f"# python scripts/ppc.py --design {a.design} --chains {a.chains} --warmup {a.warmup} --samples {a.samples}   (one MI355X)",
             f"# posterior predictive checks: design {a.design}, {a.chains} chains, warm-up {a.warmup}, sampling {a.samples}, seed {a.seed}: {N} polls; integrate = 1 (a new poll), rep = 0"]
    flagged = {}
    for variant in ([a.variant] if a.variant else VARIANTS):
        t0 = time.perf_counter()
        h = Handle(data, variant, chains=a.chains, num_warmup=a.warmup, num_samples=a.samples, seed=a.seed, cus_per_chain=1, twin=0)
        h.init()
        h.run(a.warmup + a.samples)
        t_fit = time.perf_counter() - t0
        extra = {} if variant == "full" else extra_groups(data)
        run = lambda: ppc.check(h, groups=extra)
        run()                                                                    # loads the kernels
        ms, wall = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            ck = run()
            wall.append(time.perf_counter() - t0)
            ms.append(ck.ms)
        ms = np.median(np.array(ms), axis=0)
        h.poll_rep_device(0, N, integrate=True)
        rep_ms = np.zeros(4)
        h.L.potus_ppc_timing(rep_ms.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        t0 = time.perf_counter()
        loo.loo([h])
        t_loo = time.perf_counter() - t0
        gs = ppc.groupings(data, variant)
        gs.update({k: (np.asarray(v[0], dtype=np.int32), v[1]) for k, v in extra.items()})
        t_pit, t_grp, d_pit, d_p = host_restatement(h, ck, gs)
        S = ck.n_draws
        lines += ["", f"## {variant}: fit {t_fit:.1f} s, {S} draws, {sum(len(v[1]) for v in gs.values())} groups in {len(gs)} groupings",
                  "stages of potus_ppc (potus_ppc_timing, HIP events, median of three calls after a warm-up call; ms)",
                  f"  log-likelihood and PSIS {ms[0]:9.2f}   shares and replicate {ms[1]:9.2f}   PIT {ms[2]:9.2f}   groups {ms[3]:9.2f}   wall {np.median(wall) * 1e3:9.1f}",
                  f"  k_ppc_rep alone over all polls (potus_poll_rep_device) {rep_ms[1]:9.2f} ms;   potus_loo (log-likelihood + PSIS), wall {t_loo * 1e3:9.1f} ms",
                  f"tests/ppc_ref.py in numpy on host-resident blocks: PIT sums {t_pit * 1e3:9.1f} ms, group sums and tables {t_grp * 1e3:9.1f} ms; "
                  f"largest |device - numpy|: PIT sums {d_pit:.2e}, p-values {d_p:.2e}"]
        thr = min(1.0 - 1.0 / np.log10(S), 0.7)
        hist = ck.pit_hist(10)
        u = ck.pit(loo=True, seed=1)
        from scipy import stats
        lines += [f"LOO-PIT histogram (10 bins, non-randomised; uniform = 0.100 each): {' '.join(f'{v:.3f}' for v in hist)}",
                  f"posterior PIT histogram:                                            {' '.join(f'{v:.3f}' for v in ck.pit_hist(10, loo=False))}",
                  f"coverage of the central intervals, LOO: 50 % {ck.coverage(0.5):.3f}, 95 % {ck.coverage(0.95):.3f};  posterior: 50 % {ck.coverage(0.5, loo=False):.3f}, 95 % {ck.coverage(0.95, loo=False):.3f}",
                  f"KS p-value of the randomised LOO-PIT against the uniform: {stats.kstest(u[np.isfinite(u)], 'uniform').pvalue:.4f};  Pareto k above {thr:.2f}: {int((ck.pareto_k > thr).sum())} of {N} polls"]
        fl = ck.flag(a.alpha, 5)
        flagged[variant] = {(g, lab, st) for g, lab, st, _, _ in fl}
        lines += [f"groups of five or more polls with a p-value below {a.alpha} or above {1 - a.alpha}: {len(fl)}",
                  f"  {'grouping':12s}{'label':>32s}{'statistic':>12s}{'polls':>7s}{'p':>9s}{'T_obs':>12s}{'T_rep':>12s}"]
        for g, lab, st, p, cnt in sorted(fl, key=lambda f: (f[0], min(f[3], 1 - f[3]))):
            t = ck.groups[g]
            j, k = t["labels"].index(lab), ppc.STATS.index(st)
            name = pollsters[int(lab) - 1] if (g == "pollster" and pollsters) else lab
            lines.append(f"  {g:12s}{name[:31]:>32s}{st:>12s}{cnt:7d}{p:9.4f}{t['T_obs'][j, k]:12.3f}{t['T_rep'][j, k]:12.3f}")
        for g in ("mode", "population", "all"):
            if g in ck.groups:
                t = ck.groups[g]
                lines.append(f"  {g}: " + "; ".join(f"{lab} ({int(c)} polls) p_bias {pb:.3f} p_dispersion {pd:.3f}" for lab, c, pb, pd in zip(t["labels"], t["n_polls"], t["p_bias"], t["p_dispersion"])))
        h.close()
    if len(flagged) == 2:
        only = sorted(f for f in flagged["no_mode_adjustment"] - flagged["full"] if f[0] in ("mode", "population"))
        lines += ["", "## mode and population groups flagged for the no-mode variant and not for the full model: " + (", ".join(f"{g} {lab} ({st})" for g, lab, st in only) if only else "none")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
