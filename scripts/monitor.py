#!/usr/bin/env python3
"""The posterior summary table of a fit (us_potus_model_amd/monitor.py), and what it costs beside potus_diagnostics and the host restatement.

    python scripts/monitor.py --design 2016 --chains 8 --warmup 1000 --samples 1000 --out profiles/monitor_2016.txt

Prints the table of --pars, then the wall time of potus_monitor (after one untimed call that loads the kernels) over (a) lp__ + mu_b and (b) the
whole output row, of potus_diagnostics over the same columns, and of diagnostics.monitor_row on a sample of --host-cols columns fetched to the
host: the ratio table / diagnostics and the speed-up over the host, per column.
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from us_potus_model_amd import dataprep, device_diagnostics, diagnostics as dg, monitor as mn, synthetic  # noqa: E402
from us_potus_model_amd.sampler import PotusModel  # noqa: E402


def timed(f, reps=3):
    f()                                                # loads the kernels, grows the allocator's pools
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return r, sorted(ts)[len(ts) // 2]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=("2016", "small"), default="small")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--pars", nargs="*", default=["lp__", "mu_c", "polling_bias", "mu_e_bias", "rho_e_bias", "sigma_rho"])
    ap.add_argument("--host-cols", type=int, default=500, help="columns of the host restatement's sample")
    ap.add_argument("--rows", type=int, default=40, help="rows of the table that are printed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    data = synthetic.small("full") if a.design == "small" else dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")["data"]
    t0 = time.perf_counter()
    fit = PotusModel("full").sample(data, seed=a.seed, chains=a.chains, iter_warmup=a.warmup, iter_sampling=a.samples, refresh=0)
    t_fit = time.perf_counter() - t0
    hs, h = fit._hs, fit._hs[0]
    lines = [f"# summary table: design {a.design}, {a.chains} chains, warm-up {a.warmup}, sampling {a.samples}, seed {a.seed} (fit {t_fit:.1f} s); "
             f"{h.n_cols} columns in the output row"]
    m = fit.monitor(pars=a.pars)
    text = str(m).splitlines()
    lines += ["", "## " + " ".join(a.pars)] + text[:3 + a.rows] + ([f"... ({len(m) - a.rows} more rows)"] if len(m) > a.rows else []) + text[3 + len(m):]

    a_mu, b_mu, _ = h.layout["mu_b"]
    lines += ["", "## wall time per call, median of 3 (potus_monitor forms four ESS sequences per column, potus_diagnostics one)",
              f"{'columns':<28s}{'n':>8s}{'potus_monitor':>16s}{'potus_diagnostics':>20s}{'ratio':>8s}"]
    for label, ranges in (("lp__ + mu_b", [(0, 1), (a_mu, b_mu)]), ("the whole row", [(0, h.n_cols)])):
        _, t_m = timed(lambda: [mn.monitor(hs, cols=r) for r in ranges])
        _, t_d = timed(lambda: [device_diagnostics(hs, *r) for r in ranges])
        n = sum(r[1] - r[0] for r in ranges)
        lines += [f"{label:<28s}{n:8d}{t_m * 1e3:13.1f} ms{t_d * 1e3:17.1f} ms{t_m / t_d:8.2f}"]
        if label == "the whole row":
            per_col_dev = t_m / n
    # the host restatement on a sample of columns spread over the row
    k = min(a.host_cols, h.n_cols)
    cols = np.unique(np.linspace(0, h.n_cols - 1, k).astype(int))
    nsave = h.draws_saved()
    first = nsave - h.post_warmup_saved()
    t0 = time.perf_counter()
    blk = np.concatenate([np.concatenate([x.write_array(int(c), int(c) + 1, nsave)[first:] for x in hs], axis=1) for c in cols], axis=2)
    t_fetch = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = np.array([dg.monitor_row(blk[:, :, j].T, m.probs) for j in range(len(cols))])
    t_host = time.perf_counter() - t0
    dev = np.concatenate([mn.monitor(hs, cols=(int(c), int(c) + 1), probs=m.probs).table for c in cols])
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.nanmax(np.abs(dev / ref - 1), initial=0.0)
    lines += ["", f"host restatement (diagnostics.monitor_row, numpy) on {len(cols)} columns spread over the row: {t_host:.2f} s "
                  f"({t_host / len(cols) * 1e3:.2f} ms per column, the draws already on the host; fetching them took {t_fetch:.2f} s)",
              f"device, whole row: {per_col_dev * 1e6:.1f} us per column: {t_host / len(cols) / per_col_dev:.0f} x the host's rate; "
              f"largest relative |device / host - 1| over the sample: {rel:.2e}; NaN in the same places: {np.array_equal(np.isnan(dev), np.isnan(ref))}"]
    out = "\n".join(lines) + "\n"
    print(out, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
