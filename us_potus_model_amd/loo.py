"""PSIS-LOO cross-validation of the poll models on the GPU (Vehtari, Gelman, Gabry 2017), what `fit$loo()` gives a cmdstanr user with a
`log_lik` generated quantity, and `loo_compare` to choose between the two variants fitted to the same polls.

    1. per-poll log-likelihood       potus_log_lik_device (k_loo_loglik: rows rebuilt per draw, no draws x columns block)
    2. PSIS per poll                 potus_loo / potus_loo_device (k_loo_psis: r_eff, generalized-Pareto tail, weights, elpd_loo_i)
    3. comparison                    loo_compare (host: the pointwise differences)
    4. moment matching               moment_match (potus_loo_moment_match: the polls with a high Pareto k)
    5. E_loo                         e_loo, e_loo_shared, influence (potus_e_loo_device, potus_e_loo_shared_device: expectations under the
                                     leave-one-out posteriors and what every poll does to the forecast)

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


E_LOO_TYPES = ("mean", "variance", "sd", "quantile")


class ELoo:
    """loo::E_loo of a block: .value and .pareto_k of the requested type ([polls], quantiles [polls, len(probs)]), and every estimate the
    kernel computed beside it: .mean, .variance, .sd, .quantiles [polls, len(probs)], .khat [polls, 3] (k of the mean, of variance and sd,
    of the quantiles)."""

    def __init__(self, out, khat, type, probs):
        self.type, self.probs = type, probs
        self.mean, self.variance, self.sd, self.quantiles, self.khat = out[:, 0], out[:, 1], out[:, 2], out[:, 3:], khat
        self.value = {"mean": self.mean, "variance": self.variance, "sd": self.sd, "quantile": self.quantiles}[type]
        self.pareto_k = khat[:, {"mean": 0, "variance": 1, "sd": 1, "quantile": 2}[type]]


def e_loo(block_x, block_ratios, type="mean", probs=None, r_eff=None):
    """potus_e_loo_device: loo::E_loo of x under the PSIS weights of the raw log ratios (from a fit: -log_lik), both torch tensors [polls,
    chains, draws] (float64, contiguous, on one GPU), x with its own values per poll.  type: "mean", "variance", "sd" or "quantile" (with
    probs inside (0, 1), at most 16).  r_eff: [polls], or None (computed as loo::relative_eff of -ratios).  The weights are the plain PSIS
    weights, not moment-matched ones.  DESIGN.md section 4r states the definitions."""
    if type not in E_LOO_TYPES:
        raise ValueError(f"type = {type!r}: one of {E_LOO_TYPES}")
    if type == "quantile" and probs is None:
        raise ValueError("type = 'quantile' needs probs")
    _device_block(block_x, "e_loo", ("polls", "chains", "draws"))
    _device_block(block_ratios, "e_loo", ("polls", "chains", "draws"))
    if tuple(block_x.shape) != tuple(block_ratios.shape):
        raise ValueError(f"e_loo: x is {tuple(block_x.shape)}, the log ratios {tuple(block_ratios.shape)}")
    L = load_library()
    N, ch, nd = (int(v) for v in block_x.shape)
    pr = np.zeros(0) if probs is None else np.ascontiguousarray(np.atleast_1d(probs), dtype=np.float64)
    out, kh = np.zeros((N, 3 + pr.size)), np.zeros((N, 3))
    re = None if r_eff is None else np.ascontiguousarray(r_eff, dtype=np.float64).reshape(N)
    _check(L, L.potus_e_loo_device(int(block_x.device.index or 0), C.c_void_p(block_x.data_ptr()), C.c_void_p(block_ratios.data_ptr()), N, ch, nd,
                                   None if re is None else _dp(re), _dp(pr) if pr.size else None, int(pr.size), _dp(out), _dp(kh)))
    return ELoo(out, kh, type, pr)


class ELooShared:
    """E_loo of quantities shared by all polls: .mean, .variance, .sd [polls, columns], .ess [polls] = 1 / sum w^2, .pareto_k ([polls]: the k
    of the ratios; [polls, columns] with diag: the k of every mean; None without ratios) and .ms (potus_e_loo_timing)."""

    def __init__(self, mean, var, ess, khat, ms):
        self.mean, self.variance, self.ess, self.pareto_k, self.ms = mean, var, ess, khat, ms
        self.sd = np.sqrt(np.maximum(var, 0.0))     # (.variance itself is not clamped: see e_loo_shared)


def e_loo_shared(block_x, block_log_weights, block_ratios=None, r_eff=None, diag=False):
    """potus_e_loo_shared_device: mean and variance of every column of block_x [columns, chains, draws] under every poll's normalised log
    weights block_log_weights [polls, chains, draws] (what potus_psis_device writes; plain PSIS weights, not moment-matched ones), as tiled
    products on the fp64 matrix cores.  block_ratios (the raw log ratios, same shape as the weights) and r_eff give the Pareto k.
    The product is centred per column on the column's equal-weight mean c: variance = sum w (x - c)^2 - (sum w (x - c))^2, so its absolute
    error is about eps * (variance + shift^2), shift = the leave-one-out mean minus c.  Where one draw carries nearly all the weight (a high
    k: the estimate is unusable anyway) the true variance is near 0 and the result is rounding noise of that size, possibly slightly negative;
    .variance is returned as computed, .sd clamps at 0.  e_loo (the pointwise form) has the exactly centred second pass."""
    _device_block(block_x, "e_loo_shared", ("columns", "chains", "draws"))
    _device_block(block_log_weights, "e_loo_shared", ("polls", "chains", "draws"))
    if tuple(block_x.shape[1:]) != tuple(block_log_weights.shape[1:]):
        raise ValueError(f"e_loo_shared: the columns hold {tuple(block_x.shape[1:])} chains x draws, the weights {tuple(block_log_weights.shape[1:])}")
    if block_ratios is not None:
        _device_block(block_ratios, "e_loo_shared", ("polls", "chains", "draws"))
        if tuple(block_ratios.shape) != tuple(block_log_weights.shape):
            raise ValueError(f"e_loo_shared: the log ratios are {tuple(block_ratios.shape)}, the weights {tuple(block_log_weights.shape)}")
    elif diag:
        raise ValueError("e_loo_shared: diag needs the raw log ratios")
    L = load_library()
    nc, ch, nd = (int(v) for v in block_x.shape)
    N = int(block_log_weights.shape[0])
    mean, var, ess = np.zeros((N, nc)), np.zeros((N, nc)), np.zeros(N)
    kh = None if block_ratios is None else (np.zeros((N, nc)) if diag else np.zeros(N))
    re = None if r_eff is None else np.ascontiguousarray(r_eff, dtype=np.float64).reshape(N)
    _check(L, L.potus_e_loo_shared_device(int(block_x.device.index or 0), C.c_void_p(block_x.data_ptr()), nc, C.c_void_p(block_log_weights.data_ptr()), N, ch, nd,
                                          None if block_ratios is None else C.c_void_p(block_ratios.data_ptr()), None if re is None else _dp(re),
                                          int(bool(diag)), _dp(mean), _dp(var), _dp(ess), None if kh is None else _dp(kh)))
    ms = np.zeros(4)
    _check(L, L.potus_e_loo_timing(_dp(ms)))
    return ELooShared(mean, var, ess, kh, ms)


def psis_weights(block_ratios, r_eff):
    """potus_psis_device: (normalised log weights as a torch tensor of the block's shape and device, k-hat [polls]) of raw log ratios."""
    import torch
    _device_block(block_ratios, "psis_weights", ("polls", "chains", "draws"))
    L = load_library()
    N, ch, nd = (int(v) for v in block_ratios.shape)
    lw, k = torch.empty_like(block_ratios), np.zeros(N)
    re = np.ascontiguousarray(r_eff, dtype=np.float64).reshape(N)
    _check(L, L.potus_psis_device(int(block_ratios.device.index or 0), C.c_void_p(block_ratios.data_ptr()), N, ch, nd, _dp(re), C.c_void_p(lw.data_ptr()), _dp(k)))
    return lw, k


class Influence:
    """What every poll does to the forecast: .delta [N, 2 S + 3] = the leave-one-out expectation of each column minus its posterior mean,
    .loo_mean, .sd (leave-one-out) [N, 2 S + 3], .post_mean [2 S + 3], .columns (names: score_s, national, win_s, ec_win, ev), .pareto_k [N]
    (potus_loo's), .khat [N, 2 S + 3] (the k of every mean; None without diag), .ess [N], .n_draws, .ms (potus_e_loo_timing of the product).
    With days: .days = (begin, end), .delta_days, .loo_mean_days [N, days, S + 1] and .post_mean_days [days, S + 1] (scores, national)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def k_threshold(self):
        return min(1.0 - 1.0 / np.log10(self.n_draws), 0.7)

    def top(self, column, n=10):
        """The n polls with the largest |delta| of `column` (a name or an index) among those whose Pareto k is at most the threshold:
        a list of (poll, delta, pareto_k)."""
        c = self.columns.index(column) if isinstance(column, str) else int(column)
        ok = np.flatnonzero(self.pareto_k <= self.k_threshold())
        order = ok[np.argsort(-np.abs(self.delta[ok, c]), kind="stable")][:n]
        return [(int(i), float(self.delta[i, c]), float(self.pareto_k[i])) for i in order]


def influence_columns(scores, state_weights, ev, ev_to_win=270):
    """The 2 S + 3 forecast columns of one day from scores [draws, S] (torch): the S state scores, the national vote (normalised
    state_weights . scores), the S indicators score > 0.5, electoral college won (sum ev won >= ev_to_win), electoral votes: [2 S + 3, draws]."""
    import torch
    w = torch.as_tensor(np.asarray(state_weights, dtype=np.float64) / np.sum(state_weights), device=scores.device)
    e = torch.as_tensor(np.asarray(ev, dtype=np.float64), device=scores.device)
    won = (scores > 0.5).to(torch.float64)
    evs = won @ e
    return torch.cat([scores.T, (scores @ w)[None], won.T, (evs >= ev_to_win).to(torch.float64)[None], evs[None]]).contiguous()


POOL_BLOCK_BUDGET = 256 << 20     # bytes of the pooled per-poll blocks (log-likelihoods, ratios, weights, shares) alive at a time


def _pooled_ratio_blocks(hs, integrate, blocks_alive=3, shares=False):
    """The polls of a fit in blocks whose pooled [polls, chains, draws] tensors stay within POOL_BLOCK_BUDGET, as potus_loo blocks them: yields
    (b0, b1, r, pointwise, a1, a2) with r = -log_lik of polls [b0, b1) over the chains of every handle (those of other GPUs brought to the
    first handle's by torch), pointwise = potus_loo_device's rows of the block (k-hat, r_eff), and with shares potus_poll_share_device's blocks.
    A handle with data sets, or with fewer than four post-warm-up draws per chain, is refused by the library before any kernel runs."""
    import torch
    h0 = hs[0]
    N = h0.n_polls
    dev0 = torch.device(f"cuda:{h0.opts.device}")
    if len({id(h) for h in hs}) != len(hs):
        raise ValueError("a handle is listed twice")
    nd = h0.post_warmup_saved()
    if any(h.n_polls != N or h.post_warmup_saved() != nd for h in hs):
        raise ValueError("the handles do not hold the same polls and the same number of post-warm-up draws")
    if nd < 4:
        raise ValueError(f"{nd} post-warm-up draws per chain (at least 4)")
    per_poll = 8 * nd * sum(h.opts.chains for h in hs) * (blocks_alive + (2 if shares else 0))
    nb = max(1, min(N, POOL_BLOCK_BUDGET // max(per_poll, 1)))
    for b0 in range(0, N, nb):
        b1 = min(b0 + nb, N)
        lls, s1, s2 = [], [], []
        for h in hs:
            ll = torch.empty((b1 - b0, h.opts.chains, nd), dtype=torch.float64, device=f"cuda:{h.opts.device}")
            lls.append(h.log_lik_device(b0, b1, ll, integrate=integrate).to(dev0))
            if shares:
                a1, a2 = h.poll_share_device(b0, b1, integrate=integrate)
                s1.append(a1.to(dev0))
                s2.append(a2.to(dev0))
        ll = torch.cat(lls, dim=1).contiguous()
        del lls
        pw = loo_of_block(ll).pointwise
        yield b0, b1, (-ll).contiguous(), pw, (torch.cat(s1, dim=1).contiguous() if shares else None), (torch.cat(s2, dim=1).contiguous() if shares else None)


def influence(handles, ev, day=-1, days=None, ev_to_win=270, integrate=True, diag=True):
    """Which polls move the forecast (potus_e_loo, what = influence): for every poll the leave-one-out expectation of the forecast of one day
    (default: election day) minus its posterior mean, from one fit: log-likelihood -> potus_loo's k-hat and r_eff -> PSIS weights -> the
    product on the matrix cores, on the pooled post-warm-up draws of the handles (one posterior; blocks of other GPUs are brought to the first
    handle's), the polls in blocks whose temporaries stay within 256 MB.  days = (begin, end) adds the score and national columns of every
    day of the range.  The weights are the plain PSIS weights of `loo`, not moment-matched ones: read .pareto_k first.  Handles of one
    workgroup per chain with the diagonal metric; handles with data sets and fewer than four post-warm-up draws are refused by the library."""
    hs, ids = _handle_ids(handles)
    h0 = hs[0]
    L = h0.L
    S, T, N = int(h0.data["S"]), int(h0.data["T"]), h0.n_polls
    t = T - 1 if day in (-1, None) else int(day)
    if not 0 <= t < T:
        raise ValueError(f"influence: day {day} of {T}")
    NC = 2 * S + 3
    evv = np.ascontiguousarray(ev, dtype=np.float64).reshape(S)
    mean, var, post, k, ess = np.zeros((N, NC)), np.zeros((N, NC)), np.zeros(NC), np.zeros(N), np.zeros(N)
    kh = np.zeros((N, NC)) if diag else None
    d0, d1 = (0, 0) if days is None else (int(days[0]), int(days[1]))
    nday = max(d1 - d0, 0)
    dm, dp_ = (np.zeros((N, nday, S + 1)), np.zeros((nday, S + 1))) if nday else (None, None)
    _check(L, L.potus_e_loo(ids, len(hs), int(bool(integrate)), _abi.ELOO_INFLUENCE, _dp(evv), int(ev_to_win), t, d0, d1, int(bool(diag)), _dp(mean), _dp(var),
                            _dp(post), _dp(k), _dp(ess), None if kh is None else _dp(kh), None if dm is None else _dp(dm), None if dp_ is None else _dp(dp_)))
    ms = np.zeros(4)
    _check(L, L.potus_e_loo_timing(_dp(ms)))
    out = Influence(delta=mean - post[None], loo_mean=mean, variance=var, sd=np.sqrt(np.maximum(var, 0.0)), post_mean=post, pareto_k=k, khat=kh, ess=ess,
                    n_draws=h0.post_warmup_saved() * sum(h.opts.chains for h in hs), day=t, ms=ms,
                    columns=[f"score_{s}" for s in range(S)] + ["national"] + [f"win_{s}" for s in range(S)] + ["ec_win", "ev"])
    if nday:
        out.days, out.loo_mean_days, out.post_mean_days, out.delta_days = (d0, d1), dm, dp_, dm - dp_[None]
    return out


class Predict:
    """What the model expected of each poll before it saw it: .mean, .sd of the leave-one-out predictive distribution of the observed share
    y / n, .pareto_k (of the mean of a1), .in_sample_mean (equal weights), .share = y / n, .residual = share - mean, .z = residual / sd."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def by_pollster(self):
        """(mean z, count) per pollster index [P] (state and national polls together; NaN for a pollster without polls)."""
        P = int(max(self.pollster.max(), 0)) + 1
        cnt = np.bincount(self.pollster, minlength=P)
        tot = np.bincount(self.pollster, weights=self.z, minlength=P)
        with np.errstate(invalid="ignore", divide="ignore"):
            return tot / cnt, cnt


def predict(handles, integrate=True):
    """For every poll the leave-one-out predictive mean and sd of its observed share y / n (potus_e_loo, what = predict): k_el_poll_share
    gives a1 = E_z[p] and a2 = E_z[p^2] per draw, the pointwise form their expectations under the poll's PSIS weights; mean = E[a1],
    variance = E[a1] / n + (1 - 1 / n) E[a2] - E[a1]^2.  Pooled as `influence` pools.  Plain PSIS weights, not moment-matched ones."""
    hs, ids = _handle_ids(handles)
    h0 = hs[0]
    y, n = (a.astype(np.float64) for a in poll_vectors(h0.data))
    N = h0.n_polls
    o, k = np.zeros((N, 5)), np.zeros(N)
    _check(h0.L, h0.L.potus_e_loo(ids, len(hs), int(bool(integrate)), _abi.ELOO_PREDICT, None, 0, -1, 0, 0, 0, _dp(o), None, None, _dp(k), None, None, None, None))
    share = y / n
    d = h0.data
    pollster = np.concatenate([np.asarray(d["poll_state"]), np.asarray(d["poll_national"])]).astype(np.int64) - 1
    return Predict(mean=o[:, 0], variance=o[:, 1], sd=o[:, 2], pareto_k=o[:, 3], in_sample_mean=o[:, 4], k_ratios=k, share=share,
                   residual=share - o[:, 0], z=(share - o[:, 0]) / o[:, 2], pollster=pollster, n=n, y=y)


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
