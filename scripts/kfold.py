#!/usr/bin/env python3
"""Exact K-fold cross-validation of the two model variants on a design, every fold refitted in one launch, next to the PSIS-LOO it checks
(us_potus_model_amd.crossval).

  python scripts/kfold.py --design 2016 --folds 10 --by pollster|random|state --chains 4 [--warmup 200 --samples 200] [--out FILE]

Reads tests/golden/data_2016.npz (--design small: the synthetic design).  Prints -- and with --out also writes -- elpd_kfold +- se per variant
and loo_compare of the two, against() the PSIS-LOO of a plain 8-chain fit of each variant, the polls PSIS flags side by side with their exact
values, the wall time of the one-launch fit, potus_cv_timing, and the time of the numpy restatement of the same values from write_array
columns on the host."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from us_potus_model_amd import crossval, dataprep, loo as loo_mod, synthetic, timeline  # noqa: E402
from us_potus_model_amd.sampler import Handle  # noqa: E402

VARIANTS = ("full", "no_mode_adjustment")


def restatement(tl, data, fold, n_samples):
    """The k-fold values again on the host: the logit_pi and noise columns of every chain through write_array, the integrated likelihood of
    the held-out polls by the numpy quadrature of tests/psis_ref.py, logsumexp over the fold's draws.  Returns (elpd [N], seconds)."""
    import psis_ref
    from scipy.special import logsumexp
    h = tl.handle
    y, n = (a.astype(float) for a in loo_mod.poll_vectors(data))
    Ns, Nn = int(data["N_state_polls"]), int(data["N_national_polls"])
    sig = np.concatenate([np.full(Ns, float(data["sigma_measure_noise_state"])), np.full(Nn, float(data["sigma_measure_noise_national"]))])
    t0 = time.perf_counter()
    cols = {}
    for k in ("logit_pi_democrat_state", "logit_pi_democrat_national", "raw_measure_noise_state", "raw_measure_noise_national"):
        cols[k] = h.write_array(h.layout[k][0], h.layout[k][1], n_samples)                # [iteration, chain, column]
    lp = np.concatenate([cols["logit_pi_democrat_state"], cols["logit_pi_democrat_national"]], axis=2)
    z = np.concatenate([cols["raw_measure_noise_state"], cols["raw_measure_noise_national"]], axis=2)
    eta = lp - sig * z
    cpf = tl.chains_per_date
    out = np.zeros(fold.size)
    for i in range(fold.size):
        e = eta[:, fold[i] * cpf:(fold[i] + 1) * cpf, i].reshape(-1)
        l = psis_ref.log_lik_integrated(y[i], n[i], e, sig[i])                             # with log C(n, y)
        out[i] = logsumexp(l) - np.log(l.size)
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=["2016", "small"], default="2016")
    ap.add_argument("--folds", type=int, default=10)
    ap.add_argument("--by", choices=list(crossval.BY), default="pollster")
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--loo-chains", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say(f"design {a.design}: {a.folds} folds by {a.by} x {a.chains} chains, {a.warmup} + {a.samples} transitions, both variants")
    opts = dict(num_warmup=a.warmup, num_samples=a.samples, seed=a.seed)
    kfs, loos = {}, {}
    for v in VARIANTS:
        data = dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")["data"] if a.design == "2016" else synthetic.small("full")
        fold = crossval.folds(data, a.folds, a.by)
        hs, hn = crossval.held_masks(data, fold)
        say(f"\n== {v}: {fold.size} polls, fold sizes {np.bincount(fold).tolist()}")
        tl = timeline.fit(crossval.design(data, fold), v, chains_per_date=a.chains, **opts)
        say(f"one-launch fit of {a.folds} folds x {a.chains} chains: {tl.wall_s:.2f} s wall (init + run), {tl.handle.total_leapfrogs()} leapfrogs")
        t0 = time.perf_counter()
        lpd, cnt = tl.handle.cv_lpd(hs, hn, True)
        wall = time.perf_counter() - t0
        ms = tl.handle.cv_timing()
        y, n = loo_mod.poll_vectors(data)
        kf = crossval.of_lpd(lpd, cnt, fold, name=v, y=y, n=n, integrate=True, wall_s=tl.wall_s, timing=ms)
        kf.rhat_max, kf.ess_bulk_min = tl.diagnostics(n_draws=cnt)
        say(f"potus_cv_lpd: {wall * 1e3:.2f} ms wall; kernels (potus_cv_timing): k_cv_loglik {ms['loglik_ms']:.3f} ms, k_cv_reduce {ms['reduce_ms']:.3f} ms "
            f"({fold.size} pairs x {int(cnt[0])} draws; {a.folds * a.chains * a.samples} rows of {tl.handle.n_cols} columns rebuilt)")
        ref, sec = restatement(tl, data, fold, a.samples)
        say(f"numpy restatement from write_array columns on the host: {sec * 1e3:.1f} ms; max |device - numpy| = {np.abs(ref - kf.elpd).max():.3g}")
        tl.close()
        say(f"elpd_kfold {kf.elpd_kfold:.1f} +- {kf.se:.1f}; per fold rhat_max {np.nanmax(kf.rhat_max):.3f} (worst), ess_bulk_min {np.nanmin(kf.ess_bulk_min):.0f} (worst); "
            f"largest pointwise mcse {kf.mcse.max():.3f}")
        h = Handle(data, v, chains=a.loo_chains, **opts)
        h.init()
        h.run(a.warmup + a.samples)
        lo = loo_mod.loo([h], integrate=True, name=v)
        h.close()
        say(f"PSIS-LOO of a plain {a.loo_chains}-chain fit: elpd_loo {lo.elpd_loo:.1f} +- {lo.se_elpd_loo:.1f}, Pareto k {lo.pareto_k_table()}")
        t = kf.against(lo)
        for key, lab in (("all", "all polls"), ("high_k", f"polls with k > {lo.k_threshold():.2f}")):
            r = t[key]
            say(f"  elpd_kfold_i - elpd_loo_i, {lab}: n {r['n']}, mean {r['mean']:+.4f}, max |.| {r['max_abs']:.4f}, outside 4 k-fold mcse {r['outside']}")
        flagged = np.flatnonzero(lo.pareto_k > lo.k_threshold())
        if flagged.size:
            say("  poll   fold  pareto_k   elpd_loo_i  elpd_kfold_i   mcse")
            for i in flagged:
                say(f"  {i:5d}  {fold[i]:4d}  {lo.pareto_k[i]:8.2f}  {lo.pointwise[i, 0]:10.4f}  {kf.elpd[i]:12.4f}  {kf.mcse[i]:.4f}")
        kfs[v], loos[v] = kf, lo
    say("\n== loo_compare of the two k-fold results (as_loo())")
    say(loo_mod.format_compare(loo_mod.loo_compare(*[kfs[v].as_loo() for v in VARIANTS])))
    say("== loo_compare of the two PSIS-LOOs")
    say(loo_mod.format_compare(loo_mod.loo_compare(*[loos[v] for v in VARIANTS])))
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
