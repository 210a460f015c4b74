#!/usr/bin/env python3
"""PSIS-LOO of both poll models fitted to the same polls (us_potus_model_amd/loo.py): both LOO tables with their Pareto k tables,
loo_compare, and the wall time of every potus_loo call (after one untimed call that loads the kernels).

    python scripts/loo.py --design 2016 --chains 8 --warmup 1000 --samples 1000 --plain --out profiles/loo_2016_full_vs_nomode.txt

The no-mode variant takes the full data dict (its extra entries are ignored).  --plain also prints the plain form's k table (each
poll's noise coordinate not integrated out).  --host-ref DIR times tests/psis_ref.py (the numpy restatement) on the same block.
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from us_potus_model_amd import dataprep, loo, synthetic  # noqa: E402
from us_potus_model_amd.sampler import PotusModel  # noqa: E402


def timed_loo(fit, integrate):
    fit.loo(integrate=integrate)                       # loads the kernels
    t0 = time.perf_counter()
    r = fit.loo(integrate=integrate)
    return r, time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=("2016", "small"), default="small")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--host-ref", action="store_true", help="time tests/psis_ref.py on the integrated block of the full model")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    torch.cuda.init()                                  # torch's GPU runtime first, as bench.py does (--host-ref copies through torch)
    data = synthetic.small("full") if a.design == "small" else dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")["data"]
    lines = [f"# PSIS-LOO: design {a.design}, {a.chains} chains, warm-up {a.warmup}, sampling {a.samples}, seed {a.seed}; both variants on the same polls"]
    loos = {}
    for v in ("full", "no_mode_adjustment"):
        t0 = time.perf_counter()
        fit = PotusModel(v).sample(data, seed=a.seed, chains=a.chains, iter_warmup=a.warmup, iter_sampling=a.samples, refresh=0)
        t_fit = time.perf_counter() - t0
        r, t_int = timed_loo(fit, True)
        rp, t_plain = timed_loo(fit, False)
        r.name = v
        loos[v] = r
        lines += ["", f"## {v} (fit {t_fit:.1f} s; potus_loo {t_int * 1e3:.1f} ms integrated, {t_plain * 1e3:.1f} ms plain)", str(r)]
        if a.plain:
            lines += [f"plain form (noise coordinate at the draw): elpd_loo {rp.elpd_loo:.1f} (SE {rp.se_elpd_loo:.1f}), k table {rp.pareto_k_table()}"]
        if a.host_ref and v == "full":
            import numpy as np
            import torch
            sys.path.insert(0, str(ROOT / "tests"))
            import psis_ref
            h = fit._hs[0]
            blk = torch.empty((h.n_polls, h.opts.chains, h.post_warmup_saved()), dtype=torch.float64, device=f"cuda:{h.opts.device}")
            ll = h.log_lik_device(0, h.n_polls, blk, integrate=True).cpu().numpy()
            t0 = time.perf_counter()
            ref = psis_ref.loo_pointwise(ll)
            t_ref = time.perf_counter() - t0
            lines += [f"host restatement (tests/psis_ref.py, numpy, one poll at a time) on the same block: {t_ref:.2f} s; "
                      f"largest |device - host| of elpd_loo_i: {np.abs(ref[:, 0] - r.pointwise[:, 0]).max():.2e}"]
    lines += ["", "## loo_compare", loo.format_compare(loo.loo_compare(loos["full"], loos["no_mode_adjustment"]))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
