"""Posterior predictive checks of the poll models on the GPU: could the fitted model have produced the polls it was fitted to?

    1. replicated polls              potus_poll_rep_device (k_ppc_rep: rows rebuilt per draw, the prior simulator's exact binomial sampler)
    2. PIT and LOO-PIT per poll      potus_ppc_pit_device (k_ppc_pit: sum_s w [y_rep < y], sum_s w [y_rep = y]; w = 1 / S or the PSIS weights)
    3. groups of polls               potus_ppc_groups_device (k_ppc_groups: bias, dispersion and count per pollster, mode, population, state,
                                     month; realised against replicated, a posterior predictive p-value each)
    4. the whole check on a fit      check (potus_ppc: the stages chained per poll block, pooled over the handles of a fit)

integrate=True (the default) replicates a NEW poll of the same pollster, mode, population, state and day: the poll's noise coordinate is drawn
afresh, which is the replicate that belongs with the integrated log-likelihood and its leave-one-out weights.  integrate=False repeats the same
poll at the draw's own noise coordinate.  DESIGN.md section 4s states the definitions; the randomised PIT, the non-randomised histogram
(Czado, Gneiting, Held 2009) and the coverage are formed here, on the host, from the two sums per poll.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .sampler import _check, _device_block, _dp, _handle_ids, _ip, load_library

STATS = ("bias", "dispersion", "count")
GROUP_OUT = ("T_obs", "T_rep", "gt", "eq", "lt", "p")
BY = ("pollster", "mode", "population", "state", "month", "all")
BEGIN, FINISH = 1, 2


def pit_cdf(lo, eq, u):
    """The non-randomised PIT distribution function at u (Czado et al. 2009, eq. 2, averaged over the polls): per poll 0 up to lo, linear to 1 at
    lo + eq, with F(0) = 0; polls with NaN sums are left out."""
    lo, eq = np.asarray(lo, dtype=np.float64), np.asarray(eq, dtype=np.float64)
    ok = np.isfinite(lo) & np.isfinite(eq)
    lo, hi = lo[ok], np.minimum(lo[ok] + eq[ok], 1.0)
    u = np.atleast_1d(np.asarray(u, dtype=np.float64))[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(u >= hi, 1.0, np.where(u <= lo, 0.0, (u - lo) / (hi - lo)))
    f = np.where(u <= 0.0, 0.0, f)
    return f.mean(axis=1)


def pit_hist(lo, eq, bins=10):
    """The non-randomised PIT histogram: the mass of each of `bins` equal bins of [0, 1] (sums to 1; uniform = 1 / bins each)."""
    return np.diff(pit_cdf(lo, eq, np.linspace(0.0, 1.0, int(bins) + 1)))


def pit_coverage(lo, eq, level=0.95):
    """The share of the polls' PIT mass inside the central interval of `level`."""
    a, b = pit_cdf(lo, eq, [(1.0 - level) / 2.0, (1.0 + level) / 2.0])
    return float(b - a)


class Ppc:
    """One fit's posterior predictive check.  Per poll (state polls, then national polls): .pit_lo, .pit_eq (posterior), .loo_pit_lo, .loo_pit_eq
    (leave-one-out), .pareto_k (potus_loo's); NaN for a poll with n = 0.  .groups[name]: a dict of arrays per label of the grouping: labels, n_polls,
    T_obs, T_rep [G, 3] (bias, dispersion, count), gt, eq, lt [G, 3] (draws with T_rep >, =, < T_obs), p_bias, p_dispersion, p_count.  .ms:
    potus_ppc_timing (log-likelihood and PSIS, shares and replicate, PIT, groups)."""

    def __init__(self, pit, pareto_k, groups, n_draws, integrate, rep, ms, y, n):
        self.pit_lo, self.pit_eq, self.loo_pit_lo, self.loo_pit_eq = (np.ascontiguousarray(pit[:, k]) for k in range(4))
        self.pareto_k, self.groups, self.n_draws, self.integrate, self.rep, self.ms, self.y, self.n = pareto_k, groups, n_draws, integrate, rep, ms, y, n

    def _sums(self, loo):
        return (self.loo_pit_lo, self.loo_pit_eq) if loo else (self.pit_lo, self.pit_eq)

    def pit(self, loo=True, seed=0):
        """The randomised PIT lo + v eq, v ~ U(0, 1) from numpy's default generator with `seed`: uniform when the model fits."""
        lo, eq = self._sums(loo)
        return lo + np.random.default_rng(seed).random(lo.shape) * eq

    def pit_hist(self, bins=10, loo=True):
        return pit_hist(*self._sums(loo), bins=bins)

    def coverage(self, level=0.95, loo=True):
        return pit_coverage(*self._sums(loo), level=level)

    def flag(self, alpha=0.01, min_polls=5):
        """The (grouping, label, statistic, p, n_polls) of every group of at least min_polls polls whose p-value is below alpha or above 1 - alpha."""
        out = []
        for name, g in self.groups.items():
            for k, st in enumerate(STATS):
                p = g["p_" + st]
                for j in np.flatnonzero((g["n_polls"] >= min_polls) & ((p < alpha) | (p > 1.0 - alpha))):
                    out.append((name, g["labels"][j], st, float(p[j]), int(g["n_polls"][j])))
        return out


def groupings(data, variant="full", by=BY):
    """The groupings of the polls (state polls, then national polls) from the data list: {name: (labels [N] int32, label names)}.  state: national
    polls get the label "S"; month: day // 30; the no-mode variant has no mode and no population."""
    cat = lambda a, b: np.concatenate([np.asarray(data[a]), np.asarray(data[b])]).astype(np.int64)
    N = int(data["N_state_polls"]) + int(data["N_national_polls"])
    full = variant in ("full", 0)
    out = {}
    for name in by:
        if name == "pollster":
            out[name] = (cat("poll_state", "poll_national") - 1, [str(k + 1) for k in range(int(data["P"]))])
        elif name in ("mode", "population"):
            if not full:
                continue
            key, cnt = ("poll_mode", "M") if name == "mode" else ("poll_pop", "Pop")
            out[name] = (cat(key + "_state", key + "_national") - 1, [str(k + 1) for k in range(int(data[cnt]))])
        elif name == "state":
            S = int(data["S"])
            lab = np.concatenate([np.asarray(data["state"]).astype(np.int64) - 1, np.full(int(data["N_national_polls"]), S)])
            out[name] = (lab, [str(k + 1) for k in range(S)] + ["S"])
        elif name == "month":
            lab = cat("day_state", "day_national") // 30
            out[name] = (lab, [str(k) for k in range(int(lab.max(initial=0)) + 1)])
        elif name == "all":
            out[name] = (np.zeros(N, np.int64), ["all"])
        else:
            raise ValueError(f"by = {name!r}: one of {BY}")
    return {k: (np.ascontiguousarray(v[0], dtype=np.int32), v[1]) for k, v in out.items()}


def _group_table(out, count, names):
    out = np.asarray(out).reshape(len(names), 3, 6)
    t = dict(labels=list(names), n_polls=np.asarray(count, dtype=np.int64), T_obs=out[:, :, 0], T_rep=out[:, :, 1], gt=out[:, :, 2].astype(np.int64),
             eq=out[:, :, 3].astype(np.int64), lt=out[:, :, 4].astype(np.int64))
    for k, st in enumerate(STATS):
        t["p_" + st] = out[:, k, 5]
    return t


def check(handles, by=BY, integrate=True, rep=0, groups=None):
    """potus_ppc over the pooled post-warm-up draws of the listed handles (one posterior, one GPU or several).  by: the groupings built from the
    data list (`groupings`); groups: further ones, {name: (labels [N], label names)} with label -1 for a poll in no group.  Plain PSIS weights,
    not moment-matched ones: read .pareto_k.  Handles with data sets, or with fewer than four post-warm-up draws per chain, are refused by the library."""
    from .loo import poll_vectors
    hs, ids = _handle_ids(handles)
    h0 = hs[0]
    L, N = h0.L, h0.n_polls
    gs = groupings(h0.data, h0.variant, by)
    for k, (lab, names) in (groups or {}).items():
        gs[k] = (np.ascontiguousarray(np.asarray(lab).reshape(N), dtype=np.int32), list(names))
    ng = np.array([len(v[1]) for v in gs.values()], dtype=np.int32)
    lab = np.ascontiguousarray(np.stack([v[0] for v in gs.values()]), dtype=np.int32) if gs else np.zeros((0, N), np.int32)
    tot = int(ng.sum())
    pit, k = np.zeros((N, 4)), np.zeros(N)
    gout, cnt = np.zeros((max(tot, 1), 3, 6)), np.zeros(max(tot, 1), np.int64)
    _check(L, L.potus_ppc(ids, len(hs), int(bool(integrate)), int(rep), _ip(lab) if gs else None, len(gs), _ip(ng) if gs else None, _dp(pit), _dp(k),
                          _dp(gout) if gs else None, cnt.ctypes.data_as(C.POINTER(C.c_longlong)) if gs else None))
    ms = np.zeros(4)
    _check(L, L.potus_ppc_timing(_dp(ms)))
    tabs, o = {}, 0
    for (name, (_, names)), g in zip(gs.items(), ng):
        tabs[name] = _group_table(gout[o:o + g], cnt[o:o + g], names)
        o += int(g)
    y, n = poll_vectors(h0.data)
    return Ppc(pit, k, tabs, h0.post_warmup_saved() * sum(h.opts.chains for h in hs), bool(integrate), int(rep), ms, y, n)


def pit_of_block(block_yrep, y, block_log_weights=None):
    """potus_ppc_pit_device: (lo, eq) [polls] of a torch tensor of replicates [polls, chains, draws] (float64, contiguous, on a GPU) against the
    outcomes y [polls]; block_log_weights: normalised log weights of the same shape (psis_weights), or None for equal weights."""
    _device_block(block_yrep, "pit_of_block", ("polls", "chains", "draws"))
    if block_log_weights is not None:
        _device_block(block_log_weights, "pit_of_block", ("polls", "chains", "draws"))
        if tuple(block_log_weights.shape) != tuple(block_yrep.shape):
            raise ValueError(f"pit_of_block: the replicates are {tuple(block_yrep.shape)}, the weights {tuple(block_log_weights.shape)}")
    L = load_library()
    N, ch, nd = (int(v) for v in block_yrep.shape)
    yy = np.ascontiguousarray(y, dtype=np.float64).reshape(N)
    out = np.zeros((N, 2))
    _check(L, L.potus_ppc_pit_device(int(block_yrep.device.index or 0), C.c_void_p(block_yrep.data_ptr()), _dp(yy),
                                     None if block_log_weights is None else C.c_void_p(block_log_weights.data_ptr()), N, ch, nd, _dp(out)))
    return out[:, 0].copy(), out[:, 1].copy()


def groups_of_block(block_yrep, block_a1, block_a2, y, n, labels, n_groups, acc=None, flags=BEGIN | FINISH, n_in_group=None):
    """potus_ppc_groups_device on three torch tensors [polls, chains, draws]: the polls of the block join the sums of their groups (labels [polls],
    -1: in no group).  acc: a torch tensor [n_groups, 3, 2, chains, draws] that carries the sums from block to block (flags BEGIN on the first,
    FINISH on the last); None: one block.  Returns (table [n_groups, 3, 6] (GROUP_OUT) or None before FINISH, n_in_group [n_groups])."""
    for b in (block_yrep, block_a1, block_a2):
        _device_block(b, "groups_of_block", ("polls", "chains", "draws"))
        if tuple(b.shape) != tuple(block_yrep.shape):
            raise ValueError("groups_of_block: the three blocks differ in shape")
    if acc is not None:
        _device_block(acc, "groups_of_block")
        if tuple(acc.shape) != (int(n_groups), 3, 2) + tuple(block_yrep.shape[1:]):
            raise ValueError(f"groups_of_block: acc is {tuple(acc.shape)}")
    L = load_library()
    N, ch, nd = (int(v) for v in block_yrep.shape)
    yy, nn = (np.ascontiguousarray(a, dtype=np.float64).reshape(N) for a in (y, n))
    lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(N)
    cnt = np.zeros(int(n_groups), np.int64) if n_in_group is None else n_in_group
    out = np.zeros((int(n_groups), 3, 6)) if flags & FINISH else None
    _check(L, L.potus_ppc_groups_device(int(block_yrep.device.index or 0), C.c_void_p(block_yrep.data_ptr()), C.c_void_p(block_a1.data_ptr()),
                                        C.c_void_p(block_a2.data_ptr()), _dp(yy), _dp(nn), _ip(lab), int(n_groups), N, ch, nd,
                                        None if acc is None else C.c_void_p(acc.data_ptr()), int(flags), None if out is None else _dp(out),
                                        cnt.ctypes.data_as(C.POINTER(C.c_longlong))))
    return out, cnt
