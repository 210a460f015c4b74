"""PSIS-LOO cross-validation of the poll models on the GPU (Vehtari, Gelman, Gabry 2017), what `fit$loo()` gives a cmdstanr user with a
`log_lik` generated quantity, and `loo_compare` to choose between the two variants fitted to the same polls.

    1. per-poll log-likelihood       potus_log_lik_device (k_loo_loglik: rows rebuilt per draw, no draws x columns block)
    2. PSIS per poll                 potus_loo / potus_loo_device (k_loo_psis: r_eff, generalized-Pareto tail, weights, elpd_loo_i)
    3. comparison                    loo_compare (host: the pointwise differences)
    4. moment matching               moment_match (potus_loo_moment_match: the polls with a high Pareto k)

integrate=True (the default) integrates each poll's own noise coordinate raw_measure_noise_* out of its likelihood (integrated
importance sampling, Vehtari et al. 2016): every poll has a parameter of its own, so leaving it out moves that parameter from posterior
to prior, which plain PSIS-LOO (integrate=False) meets with high Pareto k.  DESIGN.md section 4e states the definitions.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .sampler import _check, _device_block, _dp, _handle_ids, _ip, load_library

POINTWISE = ("elpd_loo", "p_loo", "looic", "pareto_k", "r_eff")
ESTIMATES = ("elpd_loo", "p_loo", "looic")


def poll_vectors(data):
    """(outcomes, trials) of every poll: state polls, then national polls."""
    y = np.concatenate([np.asarray(data["n_democrat_state"]), np.asarray(data["n_democrat_national"])]).astype(np.int64)
    n = np.concatenate([np.asarray(data["n_two_share_state"]), np.asarray(data["n_two_share_national"])]).astype(np.int64)
    return y, n


class Loo:
    """One fit's PSIS-LOO: estimates [3, 2] (elpd_loo, p_loo, looic) x (Estimate, SE), pointwise [N, 5] (POINTWISE), and the Pareto k table."""

    def __init__(self, pointwise, estimates, n_draws, name=None, y=None, n=None, integrate=None):
        self.pointwise = np.asarray(pointwise, dtype=np.float64)
        self.estimates = np.asarray(estimates, dtype=np.float64).reshape(3, 2)
        self.n_draws = int(n_draws)
        self.name, self.integrate = name, integrate
        self.y = None if y is None else np.asarray(y)
        self.n = None if n is None else np.asarray(n)

    @property
    def pareto_k(self):
        return self.pointwise[:, 3]

    @property
    def r_eff(self):
        return self.pointwise[:, 4]

    @property
    def elpd_loo(self):
        return float(self.estimates[0, 0])

    @property
    def se_elpd_loo(self):
        return float(self.estimates[0, 1])

    def k_threshold(self):
        """loo 2.x: k-hat up to min(1 - 1 / log10 S, 0.7) is good."""
        return min(1.0 - 1.0 / np.log10(self.n_draws), 0.7)

    def pareto_k_table(self):
        """{"good": count, "bad": count, "very bad": count}: k <= threshold, threshold < k <= 1, k > 1 (an infinite k-hat is very bad)."""
        k, t = self.pareto_k, self.k_threshold()
        return {"good": int((k <= t).sum()), "bad": int(((k > t) & (k <= 1)).sum()), "very bad": int((k > 1).sum())}

    def __str__(self):
        N = self.pointwise.shape[0]
        form = {None: "", True: " (noise coordinate integrated out)", False: " (plain)"}[self.integrate]
        lines = [f"Computed from {self.n_draws} by {N} log-likelihood matrix{form}", "", f"{'':10s}{'Estimate':>10s}{'SE':>8s}"]
        for i, nm in enumerate(ESTIMATES):
            lines.append(f"{nm:10s}{self.estimates[i, 0]:10.1f}{self.estimates[i, 1]:8.1f}")
        t = self.k_threshold()
        tab = self.pareto_k_table()
        lines += ["", "Pareto k diagnostic values:", f"{'':28s}{'Count':>6s}{'Pct.':>8s}"]
        for rng, lab in ((f"(-Inf, {t:.2f}]", "good"), (f"({t:.2f}, 1]", "bad"), ("(1, Inf)", "very bad")):
            lines.append(f"{rng:>14s}  {'(' + lab + ')':12s}{tab[lab]:6d}{100.0 * tab[lab] / N:7.1f}%")
        return "\n".join(lines)


def loo(handles, integrate=True, r_eff=None, name=None):
    """potus_loo over the pooled post-warm-up draws of the listed handles (one posterior, one GPU or several).  r_eff: [N polls], or None
    (computed per poll as loo::relative_eff)."""
    hs, ids = _handle_ids(handles)
    h0 = hs[0]
    N = h0.n_polls
    pw, est = np.zeros((N, 5)), np.zeros((3, 2))
    re = None if r_eff is None else np.ascontiguousarray(r_eff, dtype=np.float64).reshape(N)
    _check(h0.L, h0.L.potus_loo(ids, len(hs), int(bool(integrate)), None if re is None else _dp(re), _dp(pw), _dp(est)))
    y, n = poll_vectors(h0.data)
    S = h0.post_warmup_saved() * sum(h.opts.chains for h in hs)
    return Loo(pw, est, S, name if name is not None else h0.variant, y, n, bool(integrate))


def _runs_one_workgroup_per_chain(h):
    return h.cus_per_chain == 1 and not h.opts.twin and h.opts.metric == _abi.METRIC_DIAG and h.n_datasets == 1


def moment_match(handles, loo, polls=None, model_handle=None, **opts):
    """loo::loo_moment_match (Paananen et al. 2021) for the polls of `loo` whose Pareto k is above the threshold: potus_loo_moment_match.
    handles: the fit `loo` was computed from (with the same `integrate`).  polls: poll numbers, or None for every poll.  model_handle: a
    handle of one workgroup per chain (cus_per_chain = 1, twin = 0, diagonal metric) with the fit's data, whose model evaluates the log
    density; None takes the first such handle of the fit, or creates (and closes) a one-chain handle of the same data.  opts: max_iters
    (30), split (True), k_threshold (0: min(1 - 1 / log10 S, 0.7)), cov (False; True is refused).  Returns a Loo that loo_compare takes,
    with .k_before (the Pareto k of `loo`), .mm_info [N, 6] (_abi.LOO_MM_INFO), .mm_k_path [N, max_iters + 2], .mm_map (a, b of the listed
    polls when polls is given) and .mm_ms (passes, moments, PSIS, final: milliseconds of the device stages)."""
    from .sampler import Handle
    hs, ids = _handle_ids(handles)
    h0 = hs[0]
    L = h0.L
    o = _abi.PotusLooMmOpts()
    L.potus_default_loo_mm_opts(C.byref(o))
    o.integrate = int(bool(loo.integrate if loo.integrate is not None else True))
    for k, v in opts.items():
        if k not in ("max_iters", "split", "cov", "k_threshold", "integrate"):
            raise TypeError(f"unknown moment-matching option {k!r}")
        setattr(o, k, float(v) if k == "k_threshold" else int(v))
    N = h0.n_polls
    if loo.pointwise.shape != (N, 5):
        raise ValueError(f"the Loo holds {loo.pointwise.shape[0]} polls, the fit {N}")
    own = None
    if model_handle is None:
        model_handle = next((h for h in hs if _runs_one_workgroup_per_chain(h)), None)
    if model_handle is None:
        own = model_handle = Handle(h0.data, h0.variant, chains=1, num_warmup=0, num_samples=0, seed=1, device=int(h0.opts.device),
                                    cus_per_chain=1, twin=0)
    try:
        pw, est = np.array(loo.pointwise, dtype=np.float64, order="C"), np.zeros((3, 2))
        info, kpath = np.zeros((N, 6), np.int32), np.full((N, o.max_iters + 2), np.nan)
        pl = None if polls is None else np.ascontiguousarray(np.asarray(polls).reshape(-1), dtype=np.int32)
        mp = None if pl is None else np.zeros((pl.size, 2, h0.D))
        _check(L, L.potus_loo_moment_match(model_handle.h, ids, len(hs), C.byref(o), None if pl is None else _ip(pl), 0 if pl is None else pl.size,
                                           _dp(pw), _dp(est), _ip(info), _dp(kpath), None if mp is None else _dp(mp)))
        ms = np.zeros(4)
        _check(L, L.potus_loo_mm_timing(_dp(ms)))
    finally:
        if own is not None:
            own.close()
    out = Loo(pw, est, loo.n_draws, loo.name, loo.y, loo.n, loo.integrate)
    out.k_before, out.mm_info, out.mm_k_path, out.mm_map, out.mm_ms = loo.pareto_k.copy(), info, kpath, mp, ms
    return out


def loo_of_block(block, r_eff=None, name=None, y=None, n=None):
    """potus_loo_device on a torch tensor [polls, chains, draws] (float64, contiguous, on a GPU) of log-likelihoods."""
    _device_block(block, "loo_of_block", ("polls", "chains", "draws"))
    L = load_library()
    N, ch, nd = (int(x) for x in block.shape)
    pw, est = np.zeros((N, 5)), np.zeros((3, 2))
    re = None if r_eff is None else np.ascontiguousarray(r_eff, dtype=np.float64).reshape(N)
    _check(L, L.potus_loo_device(int(block.device.index or 0), C.c_void_p(block.data_ptr()), N, ch, nd, None if re is None else _dp(re),
                                 _dp(pw), _dp(est)))
    return Loo(pw, est, ch * nd, name, y, n)


def loo_compare(*loos):
    """loo::loo_compare: rows sorted by elpd_loo (best first), each a dict with name, elpd_diff (against the best) and
    se_diff = sqrt(N) sd(elpd_loo_i - elpd_loo_i of the best) (n - 1 in sd), then elpd_loo, se_elpd_loo, p_loo, se_p_loo, looic, se_looic.
    Refuses fits of different polls (outcomes or trials differ)."""
    if len(loos) == 1 and isinstance(loos[0], (list, tuple)):
        loos = tuple(loos[0])
    if len(loos) < 2:
        raise ValueError("loo_compare needs at least two fits")
    l0 = loos[0]
    N = l0.pointwise.shape[0]
    for lo in loos[1:]:
        same = lo.pointwise.shape[0] == N and (lo.y is None) == (l0.y is None)
        if same and l0.y is not None:
            same = np.array_equal(lo.y, l0.y) and np.array_equal(lo.n, l0.n)
        if not same:
            raise ValueError("loo_compare: the fits were not fitted to the same polls (their outcome or trial vectors differ)")
    order = sorted(range(len(loos)), key=lambda i: -loos[i].elpd_loo)
    best = loos[order[0]].pointwise[:, 0]
    rows = []
    for r, i in enumerate(order):
        lo = loos[i]
        d = lo.pointwise[:, 0] - best
        row = {"name": lo.name if lo.name is not None else f"model{i + 1}", "elpd_diff": float(d.sum()),
               "se_diff": 0.0 if r == 0 else float(np.sqrt(N) * np.std(d, ddof=1))}
        for k, nm in enumerate(ESTIMATES):
            row[nm] = float(lo.estimates[k, 0])
            row["se_" + nm] = float(lo.estimates[k, 1])
        rows.append(row)
    return rows


def format_compare(rows):
    keys = ("elpd_diff", "se_diff", "elpd_loo", "se_elpd_loo", "p_loo", "se_p_loo", "looic", "se_looic")
    w = max(len(r["name"]) for r in rows) + 2
    out = [" " * w + "".join(f"{k:>12s}" for k in keys)]
    for r in rows:
        out.append(f"{r['name']:{w}s}" + "".join(f"{r[k]:12.1f}" for k in keys))
    return "\n".join(out)
