#!/usr/bin/env python3
"""Development (GPU box): sha256 of what the PSIS and sorted-run entries return, with the library POTUS_LIB selects -- two builds that claim
the same arithmetic must print the same lines (scripts/dev/lib_digest.py's idea, for potus_psis.hpp and the kernels that call it).

    psis_digest.py                 one line per entry, output and shape, then the differences BETWEEN entries that share their ratios
    psis_digest.py --time          median wall time of 10 calls per entry (after one warm-up call) on blocks of 512 polls / columns
    psis_digest.py --table P N P N P N     the timing table of alternated --time outputs of a parent (P) and a new (N) build

Inputs: tests/sorted_run_cases.py, at its PSIS_SHAPES and at the smallest shapes that still take another path."""
import hashlib
import re
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

E_PROBS = (0.05, 0.5, 0.95)
SMALL_SHAPES = ((1, 20), (2, 10),   # Mt = 4: no smoothing
                (1, 25),            # Mt = 5: the smallest tail that is fitted
                (1, 8))             # the smallest r_eff that reads more than one lag pair
TIME_SHAPES = ((512, 8, 1000), (512, 8, 2048))   # one run in LDS, two runs


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()[:16]


def digests():
    import torch
    import sorted_run_cases as cases
    from us_potus_model_amd import loo, monitor, sampler

    def dev(a):
        return torch.tensor(np.array(a, dtype=np.float64), device="cuda:0")

    def psis_entries(tag, ll, rg, x, re):
        """ll [polls, chains, draws] through k_loo_psis, k_el_pointwise (ratios -ll) and k_mm_psis (ratios -ll and rg), r_eff computed and given"""
        lld, nld, xd = dev(ll), dev(-ll), dev(x)
        for name, r in (("computed", None), ("given", re)):
            lo = loo.loo_of_block(lld, r_eff=r)
            print(f"loo_of_block r_eff {name} {tag}: pointwise {sha(lo.pointwise)} estimates {sha(lo.estimates)}")
            e = loo.e_loo(xd, nld, "quantile", E_PROBS, r)
            print(f"e_loo r_eff {name} {tag}: mean {sha(e.mean)} variance {sha(e.variance)} quantile {sha(e.quantiles)} khat {sha(e.khat)}")
            if r is None:                                   # feeding k_loo_psis's r_eff to k_el_pointwise: what it computed itself?
                e2 = loo.e_loo(xd, nld, "quantile", E_PROBS, lo.r_eff) if np.isfinite(lo.r_eff).all() else None
                same = e2 is not None and sha(e2.mean, e2.variance, e2.quantiles, e2.khat) == sha(e.mean, e.variance, e.quantiles, e.khat)
                print(f"cross {tag}: e_loo under loo_of_block's computed r_eff {'equals' if same else 'DIFFERS from (or r_eff not finite)'} e_loo under its own")
            else:
                lw, k = loo.psis_weights(nld, r)
                fin = np.isfinite(k) & np.isfinite(lo.pareto_k) & np.isfinite(e.khat[:, 2])
                d1 = float(np.abs(k - lo.pareto_k)[fin].max()) if fin.any() else 0.0
                d2 = float(np.abs(e.khat[:, 2] - lo.pareto_k)[fin].max()) if fin.any() else 0.0
                same = k.tobytes() == lo.pareto_k.tobytes() == np.ascontiguousarray(e.khat[:, 2]).tobytes()
                print(f"cross {tag}: k-hat of loo_of_block, psis_weights(-ll), e_loo {'byte-equal' if same else 'NOT byte-equal'}: "
                      f"max |psis_weights - loo| = {d1:.3e}, max |e_loo - loo| = {d2:.3e}")
        lw, k = loo.psis_weights(dev(rg), re)
        print(f"psis_weights {tag}: weights {sha(lw.cpu().numpy())} k {sha(k)}")

    for chains, draws in cases.PSIS_SHAPES + SMALL_SHAPES:
        tag = f"{chains} x {draws}"
        psis_entries(tag, cases.log_lik_block(chains, draws), cases.ratio_block(chains, draws), cases.quantity_block(chains, draws, "continuous"),
                     np.array(cases.GENERAL_R_EFF))
        blk = dev(cases.column_block(draws, chains))
        rhat, ess = sampler.device_diagnostics_of_block(blk)
        print(f"potus_diagnostics_device {tag}: rhat {sha(rhat)} ess_bulk {sha(ess)}")
        print(f"potus_monitor_device {tag}: table {sha(monitor.monitor_of_block(blk, cases.MONITOR_PROBS).table)}")
    r = cases.many_ratios()
    psis_entries(f"many_ratios {cases.MANY_CHAINS} x {cases.MANY_DRAWS}", -r, r, cases.many_quantities(), np.array(cases.GENERAL_R_EFF)[np.arange(cases.N_MANY) % 3])


def timings():
    import torch
    from us_potus_model_amd import loo, monitor, sampler

    def timed(name, shape, call):
        call()
        ms = []
        for _ in range(10):
            t0 = time.perf_counter()
            call()                                          # (every entry ends in a copy to the host or a synchronise)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        print(f"time {name} {shape[0]} x {shape[1]} x {shape[2]}: {statistics.median(ms):.3f} ms", flush=True)

    for shape in TIME_SHAPES:
        polls, chains, draws = shape
        g = torch.Generator(device="cuda:0").manual_seed(polls * chains * draws)
        ll = torch.randn(shape, dtype=torch.float64, device="cuda:0", generator=g) * 0.7 - 3.0
        x = torch.randn(shape, dtype=torch.float64, device="cuda:0", generator=g)
        nl = (-ll).contiguous()
        blk = x.permute(2, 1, 0).contiguous()              # [draws, chains, columns]
        re = np.full(polls, 0.6)
        timed("loo_of_block r_eff computed", shape, lambda: loo.loo_of_block(ll))
        timed("loo_of_block r_eff given", shape, lambda: loo.loo_of_block(ll, r_eff=re))
        timed("psis_weights", shape, lambda: loo.psis_weights(nl, re))
        timed("e_loo mean", shape, lambda: loo.e_loo(x, nl, "mean"))
        timed("e_loo quantile", shape, lambda: loo.e_loo(x, nl, "quantile", E_PROBS))
        timed("potus_diagnostics_device", shape, lambda: sampler.device_diagnostics_of_block(blk))
        timed("potus_monitor_device", shape, lambda: monitor.monitor_of_block(blk))


def table(files):
    """files: parent, new, parent, new, ... -- per entry the median of each side's medians, the parent's spread (max - min of its medians) and
    the margin new <= parent + 3 spread (docs/HISTORY.md, round 7)"""
    runs = [{m.group(1): float(m.group(2)) for m in re.finditer(r"^time (.+): ([0-9.]+) ms$", Path(f).read_text(), re.M)} for f in files]
    par, new = runs[0::2], runs[1::2]
    print(f"{'entry':58s} {'parent ms':>10s} {'spread':>8s} {'new ms':>10s} {'margin':>10s}  within")
    worst, bad = None, 0
    for name in par[0]:
        p, n = [r[name] for r in par], [r[name] for r in new]
        pm, nm, spread = statistics.median(p), statistics.median(n), max(p) - min(p)
        ok = nm <= pm + 3 * spread
        bad += not ok
        used = (nm - pm) / (3 * spread) if spread > 0 else float("inf") if nm > pm else 0.0
        if worst is None or used > worst[1]:
            worst = (name, used)
        print(f"{name:58s} {pm:10.3f} {spread:8.3f} {nm:10.3f} {pm + 3 * spread:10.3f}  {'yes' if ok else 'NO'}")
    print(f"closest to its margin: {worst[0]} ((new - parent) / (3 spread) = {worst[1]:.2f})")
    return 1 if bad else 0


if __name__ == "__main__":
    if "--table" in sys.argv:
        sys.exit(table(sys.argv[sys.argv.index("--table") + 1:]))
    timings() if "--time" in sys.argv else digests()
