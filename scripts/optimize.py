#!/usr/bin/env python3
"""The posterior mode on the device next to the same optimisation by scipy on the CPU oracle (potus_optimize).

  python scripts/optimize.py --design 2016 --paths 8 [--timeline 32] [--jacobian] [--tol-grad 1e-2] [--out profiles/optimize_2016.txt]

Reads tests/golden/data_<design>.npz (--design small: the synthetic design).  Writes -- to --out, default profiles/optimize_<design>.txt --
the wall time of the call, potus_optimize_timing, iterations and gradient evaluations per path, the return codes, the spread of the
election-day scores across the paths, and for comparison scipy's L-BFGS (history 5) on the oracle's fast gradient from the first start,
with seconds and iterations.  --timeline N: also the modes of the first N run dates of tests/golden/timeline_2016.npz in one launch
(timeline.modes)."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from us_potus_model_amd import _abi, dataprep, synthetic, timeline  # noqa: E402
from us_potus_model_amd.sampler import Handle  # noqa: E402

VARIANT = {"2016": "full", "2012": "no_mode_adjustment", "2008": "no_mode_adjustment", "small": "full"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=list(VARIANT), default="2016")
    ap.add_argument("--paths", type=int, default=8)
    ap.add_argument("--timeline", type=int, default=0)
    ap.add_argument("--jacobian", action="store_true")
    ap.add_argument("--tol-grad", type=float, default=None, help="stop on ||g|| < this alone (default: CmdStan's default tolerances)")
    ap.add_argument("--iter", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    variant = VARIANT[a.design]
    data = synthetic.small("full") if a.design == "small" else dataprep.load_npz(ROOT / "tests" / "golden" / f"data_{a.design}.npz")["data"]
    opts = dict(jacobian=int(a.jacobian), iter=a.iter)
    if a.tol_grad is not None:
        opts.update(tol_obj=0.0, tol_rel_obj=0.0, tol_grad=a.tol_grad, tol_rel_grad=0.0, tol_param=0.0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    S, T = int(data["S"]), int(data["T"])
    h = Handle(data, variant, chains=1, seed=a.seed, cus_per_chain=1, twin=0)
    say(f"design {a.design} ({variant}, D = {h.D}): {a.paths} paths (zeros and U(-2, 2) starts), jacobian = {int(a.jacobian)}, "
        f"{'tol_grad = %g alone' % a.tol_grad if a.tol_grad is not None else 'default tolerances'}, iter = {a.iter}")
    q0 = np.vstack([np.zeros(h.D), np.random.default_rng(a.seed).uniform(-2, 2, (max(a.paths - 1, 0), h.D))])[:a.paths]
    c0 = h.layout["predicted_score"][0]
    cols = (c0 + T - 1, c0 + T * (S - 1) + T)
    h.optimize(q0[:1], cols=cols, iter=2)                                    # first launch: code object load
    for rep in range(2):
        t0 = time.perf_counter()
        res = h.optimize(q0, cols=cols, **opts)
        wall = time.perf_counter() - t0
        say(f"call {rep + 1}: {wall * 1e3:.1f} ms wall, k_opt_lbfgs {h.optimize_timing():.2f} ms (potus_optimize_timing)")
    score = res["rows"][:, ::T]
    say(f"codes {[_abi.OPTIMIZE_CODES[int(c)] for c in res['return_code']]}")
    say(f"iterations {res['iterations'].tolist()}")
    say(f"gradient evaluations {res['grad_evals'].tolist()}  (k_opt_lbfgs per evaluation of the slowest path: {h.optimize_timing() * 1e3 / res['grad_evals'].max():.1f} us)")
    say(f"||g||_2 {np.array2string(res['grad_norm'], precision=3)}")
    say(f"lp {np.array2string(res['lp'], precision=6, floatmode='fixed')}")
    say(f"election-day predicted_score: spread across paths max {np.ptp(score, axis=0).max():.3g} (over {S} states)")
    h.close()

    import optimize_ref as ref
    from oracle_lib import OracleModel
    m, irho = OracleModel(data, variant), ref.rho_index(data, variant)

    class Obj:
        D = m.D

        @staticmethod
        def neg(q):
            lp, g = m.log_prob_grad(q, fast=True)
            if not a.jacobian:
                lp, g = ref.remove_jacobian(lp, g, q, irho)
            return -lp, -g
    t0 = time.perf_counter()
    qs, nit, nfev = ref.scipy_lbfgs(Obj, q0[0])
    sec = time.perf_counter() - t0
    lp_s, g_s = Obj.neg(qs)
    sc_s = m.write_array(qs)[c0 - 7:][T - 1::T][:S]
    say(f"scipy L-BFGS-B (history 5, ftol = gtol = 0) on the CPU oracle's fast gradient, from the first start, one host core: {sec:.2f} s, {nit} iterations, "
        f"{nfev} evaluations, ||g||_2 {np.linalg.norm(g_s):.3g}, lp {-lp_s:.6f}")
    say(f"election-day predicted_score, device paths against scipy: max {np.abs(score - sc_s).max():.3g}")

    if a.timeline:
        d16 = dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")["data"]
        full = timeline.load_fixture(ROOT / "tests" / "golden" / "timeline_2016.npz", d16)
        n = min(a.timeline, full["keep_state"].shape[0])
        pick = np.unique(np.linspace(0, full["keep_state"].shape[0] - 1, n).round().astype(int))
        design = timeline.design_of(d16, full["keep_state"][pick], full["keep_national"][pick], full["mu_b_prior"][pick], full["mu_b_T_scale"][pick],
                                    [full["run_dates"][i] for i in pick])
        t0 = time.perf_counter()
        out = timeline.modes(design, "full", paths_per_date=1, seed=a.seed, **opts)
        wall = time.perf_counter() - t0
        say(f"\ntimeline.modes: {len(pick)} run dates of the 2016 campaign, one path each, ONE launch: k_opt_lbfgs {out['ms']:.2f} ms, {wall:.2f} s wall with the handle's set-up")
        say(f"codes {sorted(set(_abi.OPTIMIZE_CODES[int(c)] for c in out['return_code'].ravel()))}, iterations {out['iterations'].min()}..{out['iterations'].max()}, "
            f"evaluations {out['grad_evals'].min()}..{out['grad_evals'].max()}")
        w = np.asarray(d16["state_weights"], dtype=np.float64)
        nat = (out["predicted_score"][:, 0] * (w / w.sum())).sum(1)
        say("national vote at the mode, by run date: " + ", ".join(f"{d} {v:.4f}" for d, v in list(zip(out["run_dates"], nat))[::max(len(pick) // 8, 1)]))
    path = Path(a.out) if a.out else ROOT / "profiles" / f"optimize_{a.design}.txt"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
