#!/usr/bin/env python3
"""Which polls move the forecast, and what the model expected of each poll (us_potus_model_amd/loo.py: influence, predict; DESIGN.md
section 4r): the ten polls that move P(electoral-college win) most and the ten that move Pennsylvania most, the pollster table of
leave-one-out z-scores, the stage timings for election day and for all days, and the same expectations by numpy on the host from the
weights block copied off the device.

    python scripts/influence.py --design 2016 --chains 8 --warmup 1000 --samples 1000 --out profiles/eloo_2016.txt

The fit runs one workgroup per chain (influence reads the scores through potus_timeline_scores_device).
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from us_potus_model_amd import dataprep, loo, synthetic  # noqa: E402
from us_potus_model_amd.sampler import Handle  # noqa: E402


def timed(f):
    f()                                                # loads the kernels
    t0 = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=("2016", "small"), default="small")
    ap.add_argument("--variant", default="full")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--state", default="PA", help="the state of the second top-ten table")
    ap.add_argument("--out", default=None, help="the report's file (default for --design 2016: profiles/eloo_2016.txt)")
    a = ap.parse_args(argv)
    if a.out is None and a.design == "2016":
        a.out = str(ROOT / "profiles" / "eloo_2016.txt")
    import torch
    torch.cuda.init()
    if a.design == "small":
        data = synthetic.small(a.variant)
        S = int(data["S"])
        states, pollsters, ev = [f"s{s}" for s in range(S)], None, 3.0 + (7 * np.arange(S)) % 11
        win = int(ev.sum()) // 2 + 1
    else:
        z = dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")
        data, meta = z["data"], z["meta"]
        S = int(data["S"])
        states, pollsters, ev, win = [str(s) for s in meta["states"]], [str(p) for p in meta["pollsters"]], np.asarray(meta["ev_state"], dtype=np.float64), 270
    T, N = int(data["T"]), int(data["N_state_polls"]) + int(data["N_national_polls"])
    t0 = time.perf_counter()
    h = Handle(data, a.variant, chains=a.chains, num_warmup=a.warmup, num_samples=a.samples, seed=a.seed, cus_per_chain=1, twin=0)
    h.init()
    h.run(a.warmup + a.samples)
    t_fit = time.perf_counter() - t0
    lines = [f"# E_loo: design {a.design} ({a.variant}), {a.chains} chains, warm-up {a.warmup}, sampling {a.samples}, seed {a.seed}: {N} polls, {S} states, {T} days; fit {t_fit:.1f} s"]
    inf, t_day = timed(lambda: h.loo_influence(ev, ev_to_win=win))
    _, t_day0 = timed(lambda: h.loo_influence(ev, ev_to_win=win, diag=False))
    infd, t_all = timed(lambda: h.loo_influence(ev, ev_to_win=win, days=(0, T), diag=False))
    pr, t_pred = timed(lambda: h.loo_predict())
    lo, t_loo = timed(lambda: loo.loo([h]))
    thr = inf.k_threshold()
    ok = inf.pareto_k <= thr
    lines += ["", "## timings (wall, second call; stages from potus_e_loo_timing: pointwise, column means + products, chunk sums + ess, diagnostic; ms)",
              f"potus_loo alone (log-likelihood + PSIS)            {t_loo * 1e3:9.1f} ms",
              f"influence, election day, k of every mean           {t_day * 1e3:9.1f} ms   stages {np.round(inf.ms, 2)}",
              f"influence, election day, k of the ratios only      {t_day0 * 1e3:9.1f} ms",
              f"influence, election day + all {T} days ({T * (S + 1)} columns) {t_all * 1e3:9.1f} ms   stages, both products {np.round(infd.ms, 2)}",
              f"predict                                            {t_pred * 1e3:9.1f} ms"]
    flop = 2.0 * 2 * N * inf.n_draws * (T * (S + 1) + 2 * S + 3)
    lines += [f"column means and products of that call: {flop / max(infd.ms[1], 1e-9) / 1e9:.2f} TFLOP/s fp64 over both moments (k_dn_pool_mm 44 - 50, k_lap_solve_* 15.8)"]
    # ---- the pooled call against the device forms composed block by block (poll_share_device -> e_loo), at this size
    worst = 0.0
    for b0, b1, rb, pw, a1, _ in loo._pooled_ratio_blocks([h], True, shares=True):
        worst = max(worst, float(np.abs(loo.e_loo(a1, rb, "mean", None, pw[:, 4]).mean - pr.mean[b0:b1]).max()))
    lines += [f"predict's mean against potus_poll_share_device -> potus_e_loo_device composed per block: largest difference {worst:.2e}"]
    # ---- the same by numpy on the host from the weights block copied off the device
    blocks = list(loo._pooled_ratio_blocks([h], True))
    r = torch.cat([b[2] for b in blocks])
    lw, _ = loo.psis_weights(r, np.concatenate([b[3][:, 4] for b in blocks]))
    sc = h.timeline_scores_device((0, T))[0]                                  # [draws, days, S]
    X1 = loo.influence_columns(sc[:, T - 1].contiguous(), data["state_weights"], ev, win).cpu().numpy()
    w = np.asarray(data["state_weights"], dtype=np.float64)
    Xd = torch.cat([sc, (sc @ torch.as_tensor(w / w.sum(), device=sc.device))[:, :, None]], dim=2).permute(1, 2, 0).reshape(T * (S + 1), -1).cpu().numpy()
    lwh = lw.reshape(N, -1).cpu().numpy()
    t0 = time.perf_counter()
    W = np.exp(lwh)
    m1 = W @ X1.T
    t_h1 = time.perf_counter() - t0
    t0 = time.perf_counter()
    md = W @ Xd.T
    t_hd = time.perf_counter() - t0
    lines += [f"numpy on the host, means only, weights already there: election day {t_h1 * 1e3:.1f} ms, all days {t_hd * 1e3:.1f} ms; "
              f"largest |device - numpy|: {np.abs(m1 - inf.loo_mean).max():.2e}, {np.abs(md - infd.loo_mean_days.reshape(N, -1)).max():.2e}"]
    # ---- what it finds
    col_ec, col_st, col_nat = 2 * S + 1, states.index(a.state) if a.state in states else 0, S
    lines += ["", "## Pareto k of the ratios (potus_loo's)", f"threshold {thr:.2f}: usable (k <= threshold) {int(ok.sum())} of {N} polls; k <= 0.5: {int((inf.pareto_k <= 0.5).sum())}; "
              f"k of the ec_win mean above the threshold: {int((inf.khat[:, col_ec] > thr).sum())}, of the national mean: {int((inf.khat[:, col_nat] > thr).sum())}",
              f"largest |delta| among usable polls: national {np.abs(inf.delta[ok, col_nat]).max():.2e}, P(electoral-college win) {np.abs(inf.delta[ok, col_ec]).max():.2e}, "
              f"electoral votes {np.abs(inf.delta[ok, 2 * S + 2]).max():.2f}, a state score {np.abs(inf.delta[ok][:, :S]).max():.2e}; posterior P(ec win) {inf.post_mean[col_ec]:.4f}"]
    Ns = int(data["N_state_polls"])

    def poll_label(i):
        if i < Ns:
            st, day, pl = int(data["state"][i]) - 1, int(data["day_state"][i]), int(data["poll_state"][i]) - 1
            where = states[st]
        else:
            day, pl, where = int(data["day_national"][i - Ns]), int(data["poll_national"][i - Ns]) - 1, "national"
        return f"{where:>9s} day {day:3d} n {int(pr.n[i]):5d} share {pr.share[i]:.3f} {pollsters[pl] if pollsters else pl}"
    for title, c in ((f"the ten polls that move P(electoral-college win) most (posterior {inf.post_mean[col_ec]:.4f})", col_ec),
                     (f"the ten polls that move the score of {states[col_st]} most (posterior {inf.post_mean[col_st]:.4f})", col_st)):
        lines += ["", f"## {title}", f"{'poll':>6s}{'delta':>11s}{'k':>7s}{'ess':>8s}  poll"]
        for i, d, k in inf.top(c, 10):
            lines.append(f"{i:6d}{d:+11.2e}{k:7.2f}{inf.ess[i]:8.0f}  {poll_label(i)}")
    mz, cnt = pr.by_pollster()
    lines += ["", "## predict: leave-one-out z-scores (share - LOO mean) / LOO sd", f"all polls: mean z {pr.z.mean():+.3f}, sd of z {pr.z.std():.3f}, |z| > 2: {int((np.abs(pr.z) > 2).sum())} of {N}, "
              f"|z| > 3: {int((np.abs(pr.z) > 3).sum())}; largest |LOO mean - in-sample mean| {np.abs(pr.mean - pr.in_sample_mean).max():.2e}; k of the a1 mean above the threshold: {int((pr.pareto_k > thr).sum())}",
              f"{'pollster':>30s}{'polls':>7s}{'mean z':>9s}{'mean z sqrt(n)':>16s}"]
    for j in np.argsort(-np.abs(np.nan_to_num(mz) * np.sqrt(cnt))):
        if cnt[j]:
            lines.append(f"{(pollsters[j] if pollsters else str(j)):>30s}{cnt[j]:7d}{mz[j]:+9.2f}{mz[j] * np.sqrt(cnt[j]):+16.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    h.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
