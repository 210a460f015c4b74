#!/usr/bin/env python3
"""Score the joint forecast against the certified result (us_potus_model_amd.scoring) and write profiles/scoring_<design>.txt.

    python scripts/scoring.py --design 2016 [--backtests] [--timeline 32] [--grid] [--host]

The design is fitted (8 chains, 1 000 + 1 000 transitions: 8 000 draws) and scored against the `actual` column of
tests/golden/readme_<design>.csv, DC left out of the multivariate scores and of the RMSE as the reference leaves it out.  Reported:
  the call over all days (wall clock: median and range of the repeats after one warm-up call) and its four kernel groups (HIP events);
  k_fs_energy's fp64 rate against the vector peak;
  the same energy scores from a torch.cdist loop over the days on the same GPU, what a user would write with PyTorch;
  --host        the numpy restatement (tests/scoring_ref.py) of the energy score of election day on the host, about a minute;
  --backtests   the election-day scores of the three backtests 2008, 2012, 2016, each with both model variants where the data allow;
  --timeline N  the run dates of tests/golden/timeline_2016.npz as data sets of one handle (scripts/timeline.py): the scores by run date;
  --grid        the ten one-at-a-time prior settings of scripts/sensitivity.py against the baseline, the null copy as the Monte-Carlo floor."""
import argparse
import csv
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))

# The vector fp64 peak: the MI355X's vector fp32 peak is 157.3 Tflop/s (256 CUs x 4 SIMDs x 32 lanes x 2 flop x 2.4 GHz); a SIMD issues a
# wave's fp64 instruction over 16 lanes a clock, half the fp32 width, hence 78.65 Tflop/s.
FP32_VECTOR_PEAK = 157.3e12
FP64_VECTOR_PEAK = FP32_VECTOR_PEAK / 2
VARIANTS = ("full", "no_mode_adjustment")
OWN_VARIANT = {"2016": "full", "2012": "no_mode_adjustment", "2008": "no_mode_adjustment"}


def certified(year, states):
    lines = (ROOT / "tests" / "golden" / f"readme_{year}.csv").read_text().splitlines()
    rows = csv.DictReader(ln for ln in lines if not ln.startswith("#"))
    act = {r["state"]: float(r["actual"]) for r in rows if r["state"] != "--"}
    return np.array([act[s] for s in states])


def load(year):
    from us_potus_model_amd import dataprep
    npz = dataprep.load_npz(ROOT / "tests" / "golden" / f"data_{year}.npz")
    data, meta = npz["data"], npz["meta"]
    states = [str(s) for s in meta["states"]]
    ev = np.asarray(meta["ev_state"], dtype=np.float64)
    use = np.array([s != "DC" for s in states], dtype=np.int32)
    return data, states, ev, use, certified(year, states)


def cdist_energy(x, y, used):
    """A loop over the days, the n x n matrix of every day stored and read again."""
    import torch
    out = torch.empty(x.shape[1], dtype=torch.float64, device=x.device)
    yu = torch.as_tensor(y, device=x.device)[used]
    for d in range(x.shape[1]):
        xd = x[:, d, used]
        out[d] = (xd - yu).norm(dim=1).mean() - torch.cdist(xd, xd).sum() / (2.0 * xd.shape[0] ** 2)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def timed(f, repeats):
    f()                                                                    # warm-up: code objects loaded, the allocator's buffers in place
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = f()
        t.append((time.perf_counter() - t0) * 1e3)
    return r, float(np.median(t)), float(min(t)), float(max(t))


def line_of(r, d=None):
    """election day of a ForecastScores (data set d of it): the figures of one table line"""
    i = (-1,) if d is None else (d, -1)
    S = r.S
    return (f"rmse {float(r.rmse()[d] if d is not None else r.rmse()):.5f}  mean state crps {r.crps[i][:S][r.use].mean():.5f}  national crps {r.crps[i][S]:.5f}  "
            f"EV crps {r.crps[i][S + 1]:7.2f}  energy {r.energy[i]:.5f}  variogram {r.variogram[i]:.5f}  joint dss {r.dss_joint[i]:9.2f}")


def headline(a, out):
    import torch
    from us_potus_model_amd import scoring as fs
    from us_potus_model_amd.sampler import PotusModel
    data, states, ev, use, actual = load(a.design)
    T, S = int(data["T"]), int(data["S"])
    t0 = time.perf_counter()
    fit = PotusModel(OWN_VARIANT[a.design]).sample(data, seed=a.seed, chains=a.chains, iter_warmup=a.warmup, iter_sampling=a.samples, refresh=0)
    out(f"design {a.design} ({OWN_VARIANT[a.design]}): {a.chains} chains, {a.warmup} + {a.samples} transitions, seed {a.seed}; fit {time.perf_counter() - t0:.1f} s")
    out(f"device: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})")
    r, med, lo, hi = timed(lambda: fit.forecast_scores(ev, actual, use=use, days=(0, T), states=states), a.repeats)
    ms = fs.last_timing()
    n, m = int(r.n_draws), int(use.sum())
    flops = 3.0 * m * n * (n - 1) / 2.0 * T
    out(f"potus_forecast_scores, all {T} days, {n} draws, {m} of {S} states used (DC left out)")
    out(f"  the call, host wall clock (gathers predicted_score of every draw, then the kernels), {a.repeats} repeats after one warm-up call: "
        f"median {med:.1f} ms (min {lo:.1f}, max {hi:.1f})")
    out(f"  kernels of the last call, HIP events: columns {ms[0]:.2f} ms, energy {ms[1]:.2f} ms, variogram {ms[2]:.2f} ms, joint DSS {ms[3]:.2f} ms")
    out(f"  k_fs_energy: {flops:.3e} useful flop (a subtraction and a fused multiply-add per pair and used state) in {ms[1]:.2f} ms = "
        f"{flops / ms[1] / 1e9:.1f} Tflop/s fp64, {100 * flops / (ms[1] * 1e-3) / FP64_VECTOR_PEAK:.1f} % of the vector fp64 peak of "
        f"{FP64_VECTOR_PEAK / 1e12:.2f} Tflop/s (half the vector fp32 peak of {FP32_VECTOR_PEAK / 1e12:.1f}: an fp64 instruction issues over 16 lanes a clock)")
    out(f"  election day: {line_of(r)}")
    out(f"  energy score on days 1, {T // 2}, {T}: {r.energy[0]:.5f}, {r.energy[T // 2 - 1]:.5f}, {r.energy[-1]:.5f}")
    # the same energy scores with torch.cdist, on the draws themselves
    x = torch.as_tensor(np.ascontiguousarray(fit.extract("predicted_score")), device="cuda:0")
    used = torch.as_tensor(np.flatnonzero(use), device="cuda:0")
    blk, bmed, blo, bhi = timed(lambda: fs.score_of_block(x, data["state_weights"], ev, actual, use=use), a.repeats)
    bms = fs.last_timing()
    e, cmed, clo, chi = timed(lambda: cdist_energy(x, actual, used), a.repeats)
    out(f"  on the same draws as a block on the GPU (potus_forecast_scores_device), host wall clock of the whole call, every score: median {bmed:.1f} ms "
        f"(min {blo:.1f}, max {bhi:.1f}); its k_fs_energy + finish by HIP events: {bms[1]:.2f} ms")
    out(f"  torch.cdist loop over the {T} days (the energy score ALONE), same GPU, host wall clock with one synchronise at the end, run after the calls "
        f"above, not alternated with them: median {cmed:.1f} ms (min {clo:.1f}, max {chi:.1f}); max |cdist - kernel| = {float(np.abs(e - blk.energy).max()):.2e}")
    out(f"  like with like (host wall clock, both on the block): the whole scoring call {bmed:.1f} ms against the cdist loop's {cmed:.1f} ms, {cmed / bmed:.2f} x"
        + ("" if cmed > bmed else "  -- the hand-written path does NOT beat the cdist loop"))
    if a.host:
        import scoring_ref as ref
        x1 = x[:, -1].cpu().numpy()
        t0 = time.perf_counter()
        want = ref.energy(x1[:, use != 0], actual[use != 0])
        out(f"  numpy restatement (tests/scoring_ref.py), the energy score of election day alone, on the host: {time.perf_counter() - t0:.1f} s; "
            f"|restatement - kernel| = {abs(want - blk.energy[-1]):.2e}")
    fit.close() if hasattr(fit, "close") else None


def backtests(a, out):
    from us_potus_model_amd.sampler import PotusModel
    out("")
    out(f"election-day scores of the three backtests, both variants ({a.bt_chains} chains, {a.bt_warmup} + {a.bt_samples} transitions; DC left out)")
    for year in ("2008", "2012", "2016"):
        data, states, ev, use, actual = load(year)
        for variant in VARIANTS:
            try:
                fit = PotusModel(variant).sample(data, seed=a.seed, chains=a.bt_chains, iter_warmup=a.bt_warmup, iter_sampling=a.bt_samples, refresh=0)
            except Exception as exc:                                       # the 2008 / 2012 lists carry no mode and population adjustments
                out(f"  {year} {variant:18s} not fitted: {str(exc)[:110]}")
                continue
            r = fit.forecast_scores(ev, actual, use=use)
            out(f"  {year} {variant:18s} {line_of(r)}")
            if hasattr(fit, "close"):
                fit.close()


def run_dates(a, out):
    import timeline as tl_script
    design, variant, ev = tl_script.load("2016", a.timeline)
    _, states, _, use, actual = load("2016")
    from us_potus_model_amd import scoring as fs, timeline
    t = timeline.fit(design, variant, 4, num_warmup=200, num_samples=200, seed=a.seed)
    r = t.forecast_scores(ev, actual, use=use)
    ms = fs.last_timing()
    out("")
    out(f"the 2016 timeline: {t.n_dates} run dates x 4 chains, 200 + 200 transitions, election day scored for every date in one call "
        f"(kernels: columns {ms[0]:.2f}, energy {ms[1]:.2f}, variogram {ms[2]:.2f}, joint DSS {ms[3]:.2f} ms)")
    for d in range(t.n_dates):
        out(f"  {str(design['run_dates'][d]):12s} draws {int(r.n_draws[d]):4d}  {line_of(r, d)}")
    t.close()


def grid(a, out):
    import sensitivity as sens_script
    from us_potus_model_amd import sensitivity
    data, states, ev, use, actual = load("2016")
    design = sensitivity.grid(data, sens_script.SCALES)
    g = sensitivity.fit(design, "full", 4, num_warmup=200, num_samples=200, seed=a.seed)
    r = g.forecast_scores(ev, actual, use=use)
    base, null = int(design.get("base", 0) or 0), design.get("null")
    S = r.S
    out("")
    out(f"the prior grid of scripts/sensitivity.py on 2016: {g.n_settings} settings x 4 chains, 200 + 200 transitions; election day; setting minus baseline "
        f"(negative: nearer the result); the null copy (the baseline's data, other chains) is the Monte-Carlo floor")
    out(f"  {'setting':44s} {'rmse':>9s} {'d rmse':>9s} {'d energy':>9s} {'d variogram':>11s} {'d joint dss':>11s} {'d natl crps':>11s} {'d EV crps':>9s}")
    for d, lab in enumerate(design["labels"]):
        tag = "  <- baseline" if d == base else "  <- null copy: the floor" if null is not None and d == int(null) else ""
        out(f"  {lab:44s} {r.rmse()[d]:9.5f} {r.rmse()[d] - r.rmse()[base]:+9.5f} {r.energy[d, -1] - r.energy[base, -1]:+9.5f} "
            f"{r.variogram[d, -1] - r.variogram[base, -1]:+11.5f} {r.dss_joint[d, -1] - r.dss_joint[base, -1]:+11.2f} "
            f"{r.crps[d, -1, S] - r.crps[base, -1, S]:+11.5f} {r.crps[d, -1, S + 1] - r.crps[base, -1, S + 1]:+9.2f}{tag}")
    g.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=["2016", "2012", "2008"], default="2016")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host", action="store_true", help="also the numpy restatement of election day's energy score (about a minute)")
    ap.add_argument("--backtests", action="store_true")
    ap.add_argument("--bt-chains", type=int, default=4)
    ap.add_argument("--bt-warmup", type=int, default=500)
    ap.add_argument("--bt-samples", type=int, default=500)
    ap.add_argument("--timeline", type=int, default=0, metavar="N", help="N run dates of the 2016 campaign")
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    path = Path(a.out) if a.out else ROOT / "profiles" / f"scoring_{a.design}.txt"
    path.parent.mkdir(parents=True, exist_ok=True)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        path.write_text("\n".join(lines) + "\n")                           # kept as far as the run got
    headline(a, out)
    if a.backtests:
        backtests(a, out)
    if a.timeline:
        run_dates(a, out)
    if a.grid:
        grid(a, out)


if __name__ == "__main__":
    main()
