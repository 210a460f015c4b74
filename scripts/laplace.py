#!/usr/bin/env python3
"""The Laplace approximation on the device (potus_laplace): the step table, the stage times, the agreement with NUTS.

  python scripts/laplace.py --design 2016 --draws 8000 [--timeline 32] [--host-linalg] [--out profiles/laplace_2016.txt]

Reads tests/golden/data_<design>.npz (--design small: the synthetic design).  Writes -- to --out, default profiles/laplace_<design>.txt --
  * on the small synthetic design, max|P_dev - P_ref| against torch autograd for h = 1e-3 .. 1e-6 (tests/laplace_ref.py);
  * on the design, for the same steps, the identity (x - q^) . (-H)(x - q^) = |u|^2 of three draws, the product by central differences of the
    oracle gradient (optimize_ref.Objective.hess_vec): no D x D matrix on the host;
  * the stage times of potus_laplace_timing (HIP events; one warm-up call, then --reps calls, the median) for --draws draws, with the
    rates they imply, and the wall time of the call;
  * --host-linalg: numpy.linalg.cholesky + scipy solve_triangular on this host for the same D and draws (a random SPD matrix);
  * the election-day state means and 95 % intervals of Laplace.summary against tests/golden/posterior_2016.npz in units of its MCSE, and k-hat;
  * --timeline N: timeline.laplace on N run dates of tests/golden/timeline_2016.npz, wall time."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from us_potus_model_amd import dataprep, synthetic, timeline  # noqa: E402
from us_potus_model_amd.sampler import Handle, Laplace  # noqa: E402

VARIANT = {"2016": "full", "2012": "no_mode_adjustment", "2008": "no_mode_adjustment", "small": "full"}
STEPS = (1e-3, 1e-4, 1e-5, 1e-6)
MODE = dict(jacobian=1, tol_obj=0.0, tol_rel_obj=0.0, tol_grad=1e-2, tol_rel_grad=0.0, tol_param=0.0, iter=5000)


def identity_error(obj, mode, x, u):
    """max over the draws of |d . (-H) d - |u|^2| / |u|^2, d = x - mode, (-H) d from two oracle gradients."""
    worst = 0.0
    for xi, ui in zip(x, u):
        d = xi - mode
        uu = float(ui @ ui)
        worst = max(worst, abs(float(d @ obj.hess_vec(mode, d)) - uu) / uu)
    return worst


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=list(VARIANT), default="2016")
    ap.add_argument("--draws", type=int, default=8000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeline", type=int, default=0)
    ap.add_argument("--timeline-draws", type=int, default=1000)
    ap.add_argument("--host-linalg", action="store_true")
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import laplace_ref as lref
    import optimize_ref as oref
    variant = VARIANT[a.design]
    data = synthetic.small("full") if a.design == "small" else dataprep.load_npz(ROOT / "tests" / "golden" / f"data_{a.design}.npz")["data"]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    # ---- the step on the small design: against autograd
    say("small synthetic design (full, D = 292), Jacobian on, at the mode of tests/optimize_ref.py: max|P_dev - P_ref| (P_ref: torch autograd), max|P| 153.8")
    r = lref.small_precision("full", True)
    hs = Handle(r["data"], "full", chains=1, seed=a.seed, cus_per_chain=1, twin=0)
    u3 = np.random.default_rng(5).standard_normal((3, hs.D))
    for h in STEPS:
        res = hs.laplace(r["q"], 3, u=u3, precision=True, h=h)
        say(f"  h = {h:g}: device {np.abs(res['precision'][0] - r['P']).max():.3e}, oracle differences {np.abs(lref.precision_fd(r['obj'], r['q'], h) - r['P']).max():.3e}, "
            f"identity by hess_vec {identity_error(r['obj'], r['q'], res['q'][0], u3):.3e}")
    hs.close()

    # ---- the design itself
    hd = Handle(data, variant, chains=1, seed=a.seed, cus_per_chain=1, twin=0)
    D = hd.D
    opt = hd.optimize(np.zeros((1, D)), **MODE)
    mode = opt["q"][0]
    say(f"\ndesign {a.design} ({variant}, D = {D}): mode by potus_optimize(tol_grad = 1e-2 alone, jacobian = 1): code {int(opt['return_code'][0])}, "
        f"{int(opt['iterations'][0])} iterations, ||g||_2 {opt['grad_norm'][0]:.3g}, lp {opt['lp'][0]:.4f}")
    obj = oref.Objective(data, variant, True)
    u64 = np.random.default_rng(6).standard_normal((64, D))
    say("the identity (x - q^).(-H)(x - q^) = |u|^2 of three draws, -H d by central differences of the oracle gradient (relative error, worst draw):")
    for h in STEPS:
        res = hd.laplace(mode, 64, u=u64, h=h)
        say(f"  h = {h:g}: {identity_error(obj, mode, res['q'][0][:3], u64[:3]):.3e}   (code {int(res['return_code'][0])}, log det P {res['log_det'][0]:.6f}, "
            f"smallest pivot {res['min_pivot'][0]:.6f})")

    o = hd.laplace_opts()
    say(f"\nstage times, {a.draws} draws, h = {o.h:g} (the default), the library's normals; HIP events, median of {a.reps} calls after one warm-up call:")
    hd.laplace(mode, a.draws)
    ms, wall = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = hd.laplace(mode, a.draws)
        wall.append(time.perf_counter() - t0)
        ms.append(hd.laplace_timing())
    med = {k: float(np.median([m[k] for m in ms])) for k in ms[0]}
    G = min(D, 512)
    passes = 2 * D + 1
    say(f"  Hessian (k_lap_hess + k_lap_sym): {med['hessian_ms']:.1f} ms: {passes} model passes on G = {G} workgroups of 512 threads = {-(-passes // G)} in sequence per workgroup, "
        f"{med['hessian_ms'] * 1e3 / -(-passes // G):.0f} us per pass in a workgroup's sequence")
    say(f"  factor (dense_cholesky_launch + k_lap_diag): {med['factor_ms']:.1f} ms = {D ** 3 / 3 / med['factor_ms'] / 1e9:.2f} TFLOP/s (D^3 / 3 flops)")
    nb, panel, col_blocks, launches = -(-D // 64), 4, 0, 0                              # LAP_PANEL: U left of a panel is rewritten once per panel
    pe = nb
    while pe > 0:
        pb = max(0, pe - panel)
        col_blocks += sum(b - pb for b in range(pb, pe)) + pb
        launches += 2 * (pe - pb) - 1 + (1 if pb else 0)
        pe = pb
    upd_bytes = 2 * a.draws * 64 * 8 * col_blocks                                       # U read and written by the update kernels
    say(f"  solve (normals, |u|^2, k_lap_solve_*, rows): {med['solve_ms']:.1f} ms = {a.draws * D * D / med['solve_ms'] / 1e9:.2f} TFLOP/s (draws x D^2 flops); {nb} blocks of 64 rows in "
        f"panels of {panel}, {launches} launches; the update kernels read and write {upd_bytes / 1e9:.1f} GB of U ({upd_bytes / med['solve_ms'] / 1e9:.2f} TB/s) and read L's "
        f"{D * D * 4 / 1e9:.2f} GB once per tile row of 64 draws")
    say(f"  lp__ (k_lap_lp): {med['lp_ms']:.1f} ms = {med['lp_ms'] * 1e3 / -(-a.draws // 1024):.0f} us per pass in a workgroup's sequence (1024 workgroups)")
    say(f"  the call: {np.median(wall) * 1e3:.0f} ms wall (with {a.draws * D * 8 / 1e9:.2f} GB of draws copied to the host); the stages sum to {sum(med.values()):.0f} ms")
    lp0 = hd.log_prob_grad(mode)[0][0]
    la = Laplace(hd, mode, res, lp0, True)
    say(f"  log importance ratio over the {a.draws} draws: mean {la.log_ratio.mean():.3f}, sd {la.log_ratio.std():.3f}, max {la.log_ratio.max():.2f}; Pareto k-hat {la.pareto_k:.3f}")

    gold = ROOT / "tests" / "golden" / f"posterior_{a.design}.npz"
    if gold.exists():
        g = np.load(gold)
        ev = np.ones(int(data["S"]))
        sm = la.summary(ev)
        st = sm["state"][0]                                                              # [S, 4]: low, high, mean, P(> 0.5)
        mc = g["predicted_score_T__mcse"]
        say(f"\nelection-day predicted_score against the NUTS fit of tests/golden/{gold.name} (its MCSE of the mean: {mc.min():.2e} .. {mc.max():.2e}):")
        for name, mine, ref in (("mean", st[:, 2], g["predicted_score_T__mean"]), ("2.5 %", st[:, 0], g["predicted_score_T__q025"]), ("97.5 %", st[:, 1], g["predicted_score_T__q975"])):
            d = np.abs(mine - ref)
            say(f"  {name}: largest difference {d.max():.5f} = {(d / mc).max():.1f} MCSE (state {int(np.argmax(d / mc))}); mean difference {d.mean():.5f}")
    hd.close()

    if a.host_linalg:
        from scipy.linalg import solve_triangular
        rng = np.random.default_rng(0)
        A = rng.standard_normal((D, 64))
        P = A @ A.T + np.eye(D) * D
        U = rng.standard_normal((D, a.draws))
        t0 = time.perf_counter()
        Lh = np.linalg.cholesky(P)
        t1 = time.perf_counter()
        solve_triangular(Lh.T, U, lower=False, check_finite=False)
        t2 = time.perf_counter()
        say(f"\nthis host, the same D and draws: numpy.linalg.cholesky {t1 - t0:.2f} s, scipy solve_triangular {t2 - t1:.2f} s")

    if a.timeline:
        d16 = dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")["data"]
        full = timeline.load_fixture(ROOT / "tests" / "golden" / "timeline_2016.npz", d16)
        n = min(a.timeline, full["keep_state"].shape[0])
        pick = np.unique(np.linspace(0, full["keep_state"].shape[0] - 1, n).round().astype(int))
        design = timeline.design_of(d16, full["keep_state"][pick], full["keep_national"][pick], full["mu_b_prior"][pick], full["mu_b_T_scale"][pick],
                                    [full["run_dates"][i] for i in pick])
        t0 = time.perf_counter()
        out = timeline.laplace(design, "full", draws=a.timeline_draws, ev=np.ones(int(d16["S"])), seed=a.seed)
        wall = time.perf_counter() - t0
        tm = out["timing"]
        say(f"\ntimeline.laplace: {len(pick)} run dates of the 2016 campaign, {a.timeline_draws} draws each: {wall:.2f} s wall with both handles' set-up and the modes "
            f"(k_opt_lbfgs {out['optimize']['ms']:.0f} ms); Hessian {tm['hessian_ms']:.0f} ms, factor {tm['factor_ms']:.0f} ms, solve {tm['solve_ms']:.0f} ms, lp__ {tm['lp_ms']:.0f} ms")
        say(f"  codes {sorted(set(int(c) for c in out['return_code']))}, ||g||_2 at the modes {out['grad_norm'].min():.2e} .. {out['grad_norm'].max():.2e}, "
            f"log ratio sd per date {np.nanstd(out['log_ratio'], axis=1).min():.2f} .. {np.nanstd(out['log_ratio'], axis=1).max():.2f}")
        w = np.asarray(d16["state_weights"], dtype=np.float64)
        say("  national vote, mean [2.5 %, 97.5 %] by run date: " + ", ".join(
            f"{d} {v[2]:.4f} [{v[0]:.4f}, {v[1]:.4f}]" for d, v in list(zip(out["run_dates"], out["national"][:, 0]))[::max(len(pick) // 8, 1)]))
    path = Path(a.out) if a.out else ROOT / "profiles" / f"laplace_{a.design}.txt"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
