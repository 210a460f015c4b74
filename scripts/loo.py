#!/usr/bin/env python3
"""PSIS-LOO of both poll models fitted to the same polls (us_potus_model_amd/loo.py): both LOO tables with their Pareto k tables,
loo_compare, and the wall time of every potus_loo call (after one untimed call that loads the kernels).

    python scripts/loo.py --design 2016 --chains 8 --warmup 1000 --samples 1000 --plain --out profiles/loo_2016_full_vs_nomode.txt

The no-mode variant takes the full data dict (its extra entries are ignored).  --plain also prints the plain form's k table (each
poll's noise coordinate not integrated out).  --host-ref DIR times tests/psis_ref.py (the numpy restatement) on the same block.

--moment-match runs loo.moment_match on both forms of both variants: the k table before and after, the rounds per
poll, the device time of every stage and the call's wall time, model passes per second and the bytes per second of the moments kernel,
loo_compare before and after.  --exact refits the integrated-form polls above 0.7, one data set per poll in ONE timeline.fit launch, and
evaluates each under the fit that did not see it (potus_cv_lpd, as crossval.kfold does): |elpd_psis - exact| and |elpd_mm - exact| per poll.

    python scripts/loo.py --design 2016 --moment-match --exact --out profiles/loo_mm_2016.txt
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


def mm_passes_and_bytes(mm, S, D, batch):
    """Model passes and bytes of draws the moments kernel read in one moment_match call, from mm_info: the polls that entered the loop go in
    batches of `batch` (ascending poll number); a batch runs one start pass per poll, then lockstep rounds of its still-active polls (tiles
    of 16 polls read the draws once each), then the split's pass; two more moment passes give the base moments."""
    import numpy as np
    work = np.flatnonzero(mm.mm_info[:, 2] > 0)
    row_bytes = S * (7 + D) * 8
    passes, nbytes = 0, 2 * row_bytes
    for b0 in range(0, work.size, batch):
        w = work[b0:b0 + batch]
        rounds = mm.mm_info[w, 2]
        passes += S * int(w.size + rounds.sum() + mm.mm_info[w, 3].sum())
        for r in range(1, int(rounds.max()) + 1):
            nbytes += -(-int((rounds >= r).sum()) // 16) * row_bytes
    return passes, nbytes


def mm_batch(S, D):
    """the polls per batch potus_loo_moment_match works on (its chunk partials within 128 MB, at most 64, a multiple of 16 from 16 up)"""
    b = max(1, min(64, (128 << 20) // (-(-S // 512) * 2 * D * 8)))
    return b - b % 16 if b >= 16 else b


def moment_match_report(fit, r, form, a):
    import numpy as np
    hs = fit._hs
    t0 = time.perf_counter()
    mm = loo.moment_match(hs, r, max_iters=a.max_iters)
    wall = time.perf_counter() - t0
    S, D = r.n_draws, hs[0].D
    info, thr = mm.mm_info, r.k_threshold()
    work = np.flatnonzero(info[:, 2] > 0)
    acc = info[:, 0] + info[:, 1]
    passes, nbytes = mm_passes_and_bytes(mm, S, D, mm_batch(S, D))
    ms = mm.mm_ms
    out = [f"### {form}: moment matching of the {work.size} polls above {thr:.2f} (max_iters {a.max_iters}, split on, S = {S}, D = {D})",
           f"k table before {r.pareto_k_table()}", f"k table after  {mm.pareto_k_table()}",
           f"polls above 0.7: before {int((r.pareto_k > 0.7).sum())}, after {int((mm.pareto_k > 0.7).sum())}; polls with an accepted step {int((acc > 0).sum())} "
           f"(T1 steps {int(info[:, 0].sum())}, T2 steps {int(info[:, 1].sum())}), both candidates rejected at once {int(((acc == 0) & (info[:, 2] > 0)).sum())}",
           f"candidates evaluated per poll: min {int(info[work, 2].min()) if work.size else 0}, median {float(np.median(info[work, 2])) if work.size else 0:.0f}, "
           f"max {int(info[work, 2].max()) if work.size else 0}; stop reasons (1 below, 2 max_iters, 3 rejected) { {int(k_): int(c_) for k_, c_ in zip(*np.unique(info[work, 4], return_counts=True))} if work.size else {} }",
           f"elpd_loo {r.elpd_loo:.1f} (SE {r.se_elpd_loo:.1f}) -> {mm.elpd_loo:.1f} (SE {mm.se_elpd_loo:.1f})",
           f"wall {wall:.2f} s; device stages (potus_loo_mm_timing): passes {ms[0]:.1f} ms, moments {ms[1]:.1f} ms, PSIS {ms[2]:.1f} ms, final {ms[3]:.2f} ms",
           f"model passes {passes} in {ms[0]:.1f} ms = {passes / max(ms[0], 1e-9) * 1e3:.3g} passes/s (each with the row and the poll term; k_lap_hess: 2 x 15 098 passes in 7.8 ms = 3.87e6/s)",
           f"k_mm_moments + k_mm_moments_sum: {nbytes / 1e9:.2f} GB of draws in {ms[1]:.1f} ms = {nbytes / max(ms[1], 1e-9) / 1e6:.1f} GB/s (weights, partials and the downloads' launches not counted)"]
    rows = [f"  poll {i}: k {r.pareto_k[i]:.3f} -> {mm.pareto_k[i]:.3f}, elpd {r.pointwise[i, 0]:.3f} -> {mm.pointwise[i, 0]:.3f}, T1 {info[i, 0]} T2 {info[i, 1]} "
            f"evaluated {info[i, 2]} split {info[i, 3]} stop {info[i, 4]}" for i in work[:40]]
    return mm, out + rows


def exact_report(data, variant, r, mm, a):
    """The polls of r above 0.7 refitted without them, one data set each, in one launch; their exact elpd_i beside PSIS and moment matching."""
    import numpy as np
    from us_potus_model_amd import timeline
    polls = np.flatnonzero(r.pareto_k > 0.7)
    if polls.size == 0:
        return ["### exact: no poll above 0.7"]
    Ns, N = int(data["N_state_polls"]), r.pointwise.shape[0]
    held = np.zeros((polls.size, N), bool)
    held[np.arange(polls.size), polls] = True
    hs, hn = held[:, :Ns], held[:, Ns:]
    t0 = time.perf_counter()
    tl = timeline.fit(timeline.design_of(data, ~hs, ~hn), variant, chains_per_date=a.exact_chains, num_warmup=a.exact_warmup, num_samples=a.exact_samples, seed=a.seed)
    t_fit = time.perf_counter() - t0
    try:
        t0 = time.perf_counter()
        lpd, cnt = tl.handle.cv_lpd(hs, hn, True)
        t_cv = time.perf_counter() - t0
    finally:
        tl.close()
    d = np.arange(polls.size)
    exact = lpd[d, polls, 0]
    mcse = np.sqrt(np.maximum(np.expm1(lpd[d, polls, 1] - 2.0 * exact) / np.maximum(cnt, 1), 0.0))       # crossval.of_lpd's (Kfold.against)
    e_psis, e_mm = np.abs(r.pointwise[polls, 0] - exact), np.abs(mm.pointwise[polls, 0] - exact)
    out = [f"### exact leave-one-out of the {polls.size} integrated-form polls above 0.7: one timeline.fit launch of {polls.size} data sets x {a.exact_chains} chains x "
           f"({a.exact_warmup} + {a.exact_samples}): {t_fit:.1f} s, potus_cv_lpd {t_cv * 1e3:.1f} ms",
           f"{'poll':>6s}{'k psis':>8s}{'k mm':>8s}{'exact':>10s}{'mcse':>8s}{'psis':>10s}{'mm':>10s}{'|psis-ex|':>10s}{'|mm-ex|':>10s}{'steps':>6s}"]
    for j, i in enumerate(polls):
        out.append(f"{i:6d}{r.pareto_k[i]:8.3f}{mm.pareto_k[i]:8.3f}{exact[j]:10.3f}{mcse[j]:8.3f}{r.pointwise[i, 0]:10.3f}{mm.pointwise[i, 0]:10.3f}{e_psis[j]:10.3f}{e_mm[j]:10.3f}"
                   f"{int(mm.mm_info[i, 0] + mm.mm_info[i, 1]):6d}")
    moved = mm.mm_info[polls, 0] + mm.mm_info[polls, 1] > 0
    out.append(f"mean |elpd_psis - exact| {e_psis.mean():.3f}, mean |elpd_mm - exact| {e_mm.mean():.3f}; over the {int(moved.sum())} polls with an accepted step: "
               f"{e_psis[moved].mean() if moved.any() else float('nan'):.3f} against {e_mm[moved].mean() if moved.any() else float('nan'):.3f}; "
               f"closer after moment matching: {int((e_mm < e_psis).sum())}, further: {int((e_mm > e_psis).sum())}, unchanged: {int((e_mm == e_psis).sum())}")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--design", choices=("2016", "small"), default="small")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1843)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--host-ref", action="store_true", help="time tests/psis_ref.py on the integrated block of the full model")
    ap.add_argument("--moment-match", action="store_true", help="loo.moment_match on both forms (DESIGN.md section 4q)")
    ap.add_argument("--max-iters", type=int, default=30)
    ap.add_argument("--exact", action="store_true", help="with --moment-match: refit the integrated-form polls above 0.7 and compare")
    ap.add_argument("--exact-chains", type=int, default=4)
    ap.add_argument("--exact-warmup", type=int, default=500)
    ap.add_argument("--exact-samples", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    torch.cuda.init()                                  # torch's GPU runtime first, as bench.py does (--host-ref copies through torch)
    data = synthetic.small("full") if a.design == "small" else dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")["data"]
    lines = [f"# PSIS-LOO: design {a.design}, {a.chains} chains, warm-up {a.warmup}, sampling {a.samples}, seed {a.seed}; both variants on the same polls"]
    loos, mms = {}, {}

    def save():
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text("\n".join(lines) + "\n")
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
        if a.moment_match:
            mm, rep = moment_match_report(fit, r, "integrated", a)
            mm.name = v
            mms[v] = mm
            lines += [""] + rep
            save()
            _, rep = moment_match_report(fit, rp, "plain", a)
            lines += [""] + rep
            save()
            if a.exact:
                lines += [""] + exact_report(data, v, r, mm, a)
                save()
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
    if a.moment_match:
        lines += ["", "## loo_compare after moment matching (integrated form)", loo.format_compare(loo.loo_compare(mms["full"], mms["no_mode_adjustment"]))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
