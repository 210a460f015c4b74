"""Simulation-based calibration (Talts et al. 2018) of the sampler, adaptation and model code, on the GPU.

    1. theta~ ~ prior                     potus_simulate_prior (one workgroup per simulation)
    2. y~ ~ likelihood(theta~)            (same kernel: exact binomial draws)
    3. fit the model to y~                many data sets in one handle (potus_set_datasets): the replicates are chains of one launch
    4. rank of theta~ among the draws     potus_sbc_ranks (counts on the device, no draws x columns block)

Over many replicates the ranks are uniform on 0..L if and only if the whole chain of computation is right.  Sampler options that the
many-data-set kernels do not run (a cluster per chain, two workgroups per chain, the dense or pooled metric) are calibrated one handle
per replicate, one after another.
"""
from __future__ import annotations

import time

import numpy as np
from scipy import stats

from . import _abi
from .sampler import Handle, PotusError, device_diagnostics_of_block

# options a many-data-set handle runs itself; anything else (or a value other than these) means one handle per replicate
_BATCHED = {"cus_per_chain": 1, "twin": 0, "metric": _abi.METRIC_DIAG, "pooled_metric": 0}
_MEM_CAP = 48 << 30            # bytes of draws + chain state one handle may hold


def default_columns(data, variant="full"):
    """About fifteen named columns that together touch every block of the model (CmdStan names)."""
    S, T = int(data["S"]), int(data["T"])
    cols = [f"mu_b.{s}.{T}" for s in (1, max(1, S // 2), S)] + ["mu_b.1.1", f"national_mu_b_average.{T}", "national_mu_b_average.1",
                                                                  "polling_bias.1", f"polling_bias.{S}", "mu_c.1", f"mu_c.{int(data['P'])}"]
    if _abi.VARIANTS.get(variant, variant) == _abi.VARIANT_FULL:
        cols += ["mu_m.1", "mu_pop.1", "mu_e_bias", "rho_e_bias", f"e_bias.{T}"]
    cols += [f"predicted_score.{T}.1"]
    return cols


def column_index(data, variant, name):
    """Output-row column of a CmdStan name such as "mu_b.3.254" (1-based indices, matrices column-major)."""
    if isinstance(name, (int, np.integer)):
        return int(name)
    layout, _ = _abi.column_layout(data, variant)
    base, *idx = name.split(".")
    a, b, dims = layout[base]
    if len(idx) != len(dims) or not all(1 <= int(i) <= d for i, d in zip(idx, dims)):
        raise KeyError(name)
    off, stride = 0, 1
    for i, d in zip(idx, dims):
        off += (int(i) - 1) * stride
        stride *= d
    return a + off


def plan_batches(n_sims, chains_per_sim, max_chains):
    """[(first simulation, simulations)] of handles holding at most max_chains chains each (at least one simulation per handle)."""
    per = max(1, int(max_chains) // int(chains_per_sim))
    return [(s, min(per, n_sims - s)) for s in range(0, int(n_sims), per)]


def chains_cap(data, variant, num_warmup, num_samples, save_warmup=0, mem_cap=_MEM_CAP):
    """Chains one handle may hold under mem_cap bytes: the saved draws plus the chain state (about 80 vectors of D)."""
    D = _abi.num_params(data, variant)
    per_chain = ((num_samples + (num_warmup if save_warmup else 0)) * (_abi.N_SAMPLER_COLS + D) + 80 * (D + 8)) * 8
    return int(max(1, min(1024, mem_cap // per_chain)))


def break_ties(less, equal, seed=0):
    """Rank = less + U{0 .. equal}, from a seeded numpy generator."""
    rng = np.random.default_rng(seed)
    less, equal = np.asarray(less, dtype=np.int64), np.asarray(equal, dtype=np.int64)
    return less + np.floor(rng.random(less.shape) * (equal + 1)).astype(np.int64)


def uniformity(ranks, L, bins=20):
    """Chi-square p-value per column that ranks [n, ncols] (values 0..L) are uniform; bins split the L + 1 values as evenly as they can
    (expected counts follow the number of values in each bin)."""
    obs, edges = histograms(ranks, L, bins)
    expected = obs.sum(axis=1, keepdims=True) * np.diff(edges) / (L + 1)
    return stats.chi2.sf(((obs - expected) ** 2 / expected).sum(axis=1), obs.shape[1] - 1)


def histograms(ranks, L, bins=20):
    """(counts [ncols, bins], edges): bin b holds the rank values [edges[b], edges[b + 1])."""
    ranks = np.atleast_2d(np.asarray(ranks))
    bins = int(min(bins, L + 1))
    edges = np.floor(np.arange(bins + 1) * (L + 1) / bins).astype(np.int64)
    counts = np.stack([np.bincount(np.searchsorted(edges, ranks[:, k], side="right") - 1, minlength=bins)[:bins] for k in range(ranks.shape[1])])
    return counts, edges


def _replicate_stats(h, first, reps, chains_per_sim):
    """Per replicate of handle h: max split R-hat over lp__ and the unconstrained coordinates, post-warm-up divergences, failed flag."""
    import torch
    status, _ = h.chain_status()
    n_saved = h.draws_saved()
    ptr, _ = h.draws_device_ptr()
    row = _abi.N_SAMPLER_COLS + h.D
    n_max = h.opts.num_samples + (h.opts.num_warmup if h.opts.save_warmup else 0)

    class _Dev:
        def __init__(s_, p, shape):
            s_.__cuda_array_interface__ = {"shape": shape, "typestr": "<f8", "data": (p, False), "version": 2}
    draws = torch.as_tensor(_Dev(ptr, (h.opts.chains, n_max, row)), device=f"cuda:{h.opts.device}")
    rhat, div, failed = np.full(reps, np.nan), np.zeros(reps, np.int64), np.zeros(reps, bool)
    cols = [0] + list(range(_abi.N_SAMPLER_COLS, row))
    for r in range(reps):
        c0, c1 = r * chains_per_sim, (r + 1) * chains_per_sim
        failed[r] = any(status[c0:c1])
        if failed[r] or n_saved - first < 4:
            continue
        blk = draws[c0:c1, first:n_saved]
        div[r] = int(blk[:, :, 5].sum().item())
        rh, _ = device_diagnostics_of_block(blk[:, :, cols].permute(1, 0, 2).contiguous())
        rhat[r] = float(np.nanmax(rh))
    return rhat, div, failed


def run(data, variant="full", n_sims=100, chains_per_sim=2, num_warmup=1000, num_samples=1000, thin=10, seed=1843, columns=None,
        sim_data=None, tie_seed=0, mem_cap=_MEM_CAP, **opts):
    """SBC of the posterior of `data`'s design.  Simulates from `sim_data` (default: `data`; a different prior there is the negative control).

    Returns dict(ranks [n_sims, ncols] (ties broken at random), L, columns (names), less, equal, rhat, divergent, failed [n_sims],
    wall_s, leapfrogs, batched (True: replicates as chains of one launch))."""
    import torch
    if not torch.cuda.is_available():
        raise PotusError("sbc.run: torch sees no GPU (the per-replicate R-hat is taken by potus_diagnostics_device on torch tensors)")
    torch.cuda.init()          # before the library's first launch in this process, as bench.py does
    columns = list(default_columns(data, variant) if columns is None else columns)
    idx = np.array([column_index(data, variant, c) for c in columns])
    a, e = int(idx.min()), int(idx.max()) + 1
    t0 = time.perf_counter()
    sim = Handle(data if sim_data is None else sim_data, variant, chains=1, num_warmup=0, num_samples=0, device=opts.get("device", 0))
    q, ys, yn = sim.simulate_prior(seed, n_sims)
    truth = sim.constrain(q, a, e)
    sim.close()
    save_warmup = int(opts.get("save_warmup", 0))
    first = num_warmup if save_warmup else 0
    batched = all(opts.get(k, v) == v for k, v in _BATCHED.items())
    less, equal = np.zeros((n_sims, e - a), np.int64), np.zeros((n_sims, e - a), np.int64)
    rhat, div, failed = np.full(n_sims, np.nan), np.zeros(n_sims, np.int64), np.zeros(n_sims, bool)
    L, leapfrogs = None, 0
    fit_opts = dict(num_warmup=num_warmup, num_samples=num_samples, seed=seed, **opts)
    if batched:
        fit_opts.update(_BATCHED)
        plan = plan_batches(n_sims, chains_per_sim, chains_cap(data, variant, num_warmup, num_samples, save_warmup, mem_cap))
    else:
        plan = [(s, 1) for s in range(n_sims)]
    for s0, ns in plan:
        if batched:
            h = Handle(data, variant, chains=ns * chains_per_sim, chain_id_offset=s0 * chains_per_sim, **fit_opts)   # (own Philox streams)
            h.set_datasets(ys[s0:s0 + ns], yn[s0:s0 + ns])
        else:
            d1 = dict(data, n_democrat_state=ys[s0], n_democrat_national=yn[s0])
            h = Handle(d1, variant, chains=chains_per_sim, chain_id_offset=s0 * chains_per_sim, **fit_opts)
        try:
            h.init()
            h.run(num_warmup + num_samples)
        except Exception:
            if batched:
                raise
            failed[s0] = True                      # a plain handle fails as a whole (step-size search, initialisation)
            h.close()
            continue
        ls, eq, Lh = h.sbc_ranks(truth[s0:s0 + ns], a, e, thin)
        L = Lh if L is None else L
        less[s0:s0 + ns], equal[s0:s0 + ns] = ls, eq
        rhat[s0:s0 + ns], div[s0:s0 + ns], failed[s0:s0 + ns] = _replicate_stats(h, first, ns, chains_per_sim)
        leapfrogs += h.total_leapfrogs()
        h.close()
    sel = idx - a
    less, equal = less[:, sel], equal[:, sel]
    ranks = break_ties(less, equal, tie_seed)
    return dict(ranks=ranks, L=int(L or 0), columns=columns, less=less, equal=equal, rhat=rhat, divergent=div, failed=failed,
                wall_s=time.perf_counter() - t0, leapfrogs=leapfrogs, batched=batched)
