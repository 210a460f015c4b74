#!/usr/bin/env python3
"""Simulation-based calibration of the sampler on the GPU (us_potus_model_amd/sbc.py): a text report of the rank histograms, the
chi-square p-value of every column, failed replicates, wall time, leapfrogs per second, R-hat and divergences.

    python scripts/sbc.py --design 2016 --sims 128 --chains 2 --warmup 1000 --samples 1000 --thin 10 --out profiles/sbc_2016.txt
    python scripts/sbc.py --design small --sims 64 --metric dense_e --pooled-metric 1      # one handle per replicate
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from us_potus_model_amd import _abi, dataprep, sbc, synthetic  # noqa: E402


def design(name, variant):
    if name == "small":
        v = variant or "full"
        return synthetic.small(v), v
    d = dataprep.load_npz(ROOT / "tests" / "golden" / f"data_{name}.npz")["data"]
    return d, variant or ("full" if name == "2016" else "no_mode_adjustment")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=("small", "2016", "2012", "2008"), default="small")
    ap.add_argument("--variant", choices=tuple(_abi.VARIANTS), default=None)
    ap.add_argument("--sims", type=int, default=128)
    ap.add_argument("--chains", type=int, default=2, help="chains per replicate")
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--thin", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--bins", type=int, default=20)
    ap.add_argument("--columns", default=None, help="comma-separated CmdStan column names (default: sbc.default_columns)")
    ap.add_argument("--metric", choices=tuple(_abi.METRICS), default="diag_e")
    ap.add_argument("--pooled-metric", type=int, default=0)
    ap.add_argument("--cus-per-chain", type=int, default=None, help="default: 1 (replicates as chains of one launch) for the diagonal metric, "
                                                                      "else the library's choice")
    ap.add_argument("--twin", type=int, default=None)
    ap.add_argument("--max-depth", type=int, default=10)
    ap.add_argument("--delta", type=float, default=0.8)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="write the report here as well")
    a = ap.parse_args(argv)
    data, variant = design(a.design, a.variant)
    batchable = a.metric == "diag_e" and not a.pooled_metric
    if a.cus_per_chain is None:
        a.cus_per_chain = 1 if batchable else 0
    if a.twin is None:
        a.twin = 0 if batchable else -1
    cols = a.columns.split(",") if a.columns else None
    r = sbc.run(data, variant, n_sims=a.sims, chains_per_sim=a.chains, num_warmup=a.warmup, num_samples=a.samples, thin=a.thin,
                seed=a.seed, columns=cols, metric=_abi.METRICS[a.metric], pooled_metric=a.pooled_metric, cus_per_chain=a.cus_per_chain,
                twin=a.twin, max_depth=a.max_depth, delta=a.delta, device=a.device)
    ok = ~r["failed"]
    L = r["L"]
    p = sbc.uniformity(r["ranks"][ok], L, a.bins) if ok.any() and L else np.full(len(r["columns"]), np.nan)
    counts, edges = sbc.histograms(r["ranks"][ok], L, a.bins) if ok.any() and L else (None, None)
    lines = [f"# SBC: design {a.design} ({variant}), {a.sims} replicates x {a.chains} chains, warm-up {a.warmup}, sampling {a.samples}, thin {a.thin}, "
             f"seed {a.seed}, metric {a.metric}, pooled_metric {a.pooled_metric}, cus_per_chain {a.cus_per_chain}, twin {a.twin}",
             f"# {'replicates as chains of one launch per handle' if r['batched'] else 'one handle per replicate, one after another'}",
             f"wall time {r['wall_s']:.1f} s (simulation, fits, ranks), {r['leapfrogs']} leapfrogs, {r['leapfrogs'] / r['wall_s'] / 1e3:.1f} k leapfrogs/s",
             f"failed replicates {int(r['failed'].sum())} of {a.sims}; L = {L} draws compared per replicate",
             f"max split R-hat (lp__ and unconstrained coordinates) per replicate: median {np.nanmedian(r['rhat']):.4f}, max {np.nanmax(r['rhat']):.4f}"
             if np.isfinite(r["rhat"]).any() else "R-hat: none",
             f"post-warm-up divergences: {int(r['divergent'].sum())} in {int((r['divergent'] > 0).sum())} replicates",
             f"Bonferroni bar p > {0.001 / len(r['columns']):.2e}: {'all columns pass' if (p > 0.001 / len(p)).all() else 'FAILS'}", ""]
    if counts is not None:
        lines.append(f"{'column':34s} {'p':>8s}  rank histogram ({counts.shape[1]} bins over 0..{L}; expected ~{ok.sum() / counts.shape[1]:.1f} each)")
        for c, pv, h in zip(r["columns"], p, counts):
            lines.append(f"{c:34s} {pv:8.4f}  " + " ".join(f"{x:3d}" for x in h))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
