"""The posterior summary table, on the device: what `fit$summary()` / `print(stanfit)` / `rstan::monitor` show, for any column of the output row.

The reference's scripts extract a parameter and tabulate it at once (final_2016.R:556-705):

    mu_b_T    <- mean_low_high(extract(out, "mu_b")[[1]][, , 254], ...)     ->  monitor(hs, ["mu_b"]).mean_low_high("mu_b")[:, -1]
    mu_c      mean +- 1.96 sd (final_2016.R:568-582)                           ->  monitor(hs, ["mu_c"]).mean_low_high("mu_c")
    e_bias    apply(e_bias, 2, mean) (final_2016.R:705)                        ->  monitor(hs, ["e_bias"]).par("e_bias")[..., 0]

potus_monitor (csrc/potus_monitor.hpp) forms every row on the GPU that holds the draws: mean, sd, mad, mcse_mean, rhat, ess_bulk, ess_tail,
ess_mean and R's type-7 quantiles; diagnostics.monitor_row is its numpy restatement.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .diagnostics import MONITOR_STATS
from .sampler import _check, _device_block, _dp, _handle_ids, load_library

N_STATS = len(MONITOR_STATS)
MAX_PROBS = 16
DEFAULT_PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)


def _probs(probs):
    p = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, dtype=np.float64))) if probs is not None and len(probs) else np.zeros(0)
    if p.ndim != 1 or p.size > MAX_PROBS:
        raise ValueError(f"monitor: at most {MAX_PROBS} probabilities ({p.size} given)")
    if not (np.isfinite(p).all() and (p >= 0).all() and (p <= 1).all()):
        raise ValueError("monitor: probabilities must lie in [0, 1]")
    return p


def _prob_label(p):
    return f"{100 * p:.10g}%"


class Monitor:
    """table [columns, 8 + len(probs)], names [columns] (potus_column_name), blocks {parameter: (first row, end row, dims)}."""

    def __init__(self, table, names, probs, blocks=None, n_chains=None, n_draws=None):
        self.table = np.asarray(table, dtype=np.float64)
        self.names = list(names)
        self.probs = tuple(float(p) for p in probs)
        self.stats = tuple(MONITOR_STATS) + tuple(_prob_label(p) for p in self.probs)
        self.blocks = dict(blocks or {})
        self.n_chains, self.n_draws = n_chains, n_draws
        if self.table.shape != (len(self.names), len(self.stats)):
            raise ValueError(f"table has shape {self.table.shape}, ({len(self.names)}, {len(self.stats)}) expected")

    def __len__(self):
        return len(self.names)

    def column(self, stat):
        """One statistic of every row: a name of `stats` ("mean", "rhat", "97.5%", ...)."""
        return self.table[:, self.stats.index(stat)]

    def par(self, name):
        """The rows of one parameter in its own shape: [*dims, 8 + len(probs)] (matrices column-major in the row, as CmdStan flattens them)."""
        if name not in self.blocks:
            raise KeyError(f"{name!r} is not in this table (it holds {sorted(self.blocks)})")
        a, b, dims = self.blocks[name]
        t = self.table[a:b]
        if not dims:
            return t[0]
        return t.reshape(tuple(reversed(dims)) + (t.shape[1],)).transpose(tuple(range(len(dims) - 1, -1, -1)) + (len(dims),))

    def mean_low_high(self, name, z=1.96):
        """final_2016.R:578-582: (mean, mean - z sd, mean + z sd) of a parameter, [*dims, 3]."""
        t = np.atleast_2d(self.par(name))
        m, s = t[..., 0], t[..., 1]
        out = np.stack([m, m - z * s, m + z * s], axis=-1)
        return out if self.blocks[name][2] else out[0]

    def __str__(self):
        head = f"Inference for {len(self.names)} columns"
        if self.n_chains and self.n_draws:
            head += f": {self.n_chains} chains, each with {self.n_draws} post-warmup draws; total post-warmup draws={self.n_chains * self.n_draws}"
        w = max([len(n) for n in self.names] + [4])
        cols = ("mean", "se_mean", "sd") + tuple(_prob_label(p) for p in self.probs) + ("n_eff", "Rhat", "tail_eff")
        idx = [0, 3, 1] + list(range(N_STATS, N_STATS + len(self.probs))) + [5, 4, 6]
        lines = [head + ".", "", " " * w + "".join(f"{c:>11s}" for c in cols)]
        for n, row in zip(self.names, self.table):
            cells = []
            for c, i in zip(cols, idx):
                v = row[i]
                whole = c in ("n_eff", "tail_eff") or (c != "se_mean" and 1e5 <= abs(v) < 1e10)      # lp__ of the large designs: no exponent
                cells.append(f"{v:11.0f}" if whole and np.isfinite(v) else f"{v:11.3f}" if c == "Rhat" else f"{v:11.4g}")
            lines.append(f"{n:<{w}s}" + "".join(cells))
        lines += ["", "n_eff is the bulk effective sample size, tail_eff the tail one, Rhat the rank-normalised split R-hat (Vehtari et al. 2021);",
                  "se_mean = sd / sqrt(ess_mean)."]
        return "\n".join(lines)


def _column_names(h, cols):
    buf = C.create_string_buffer(96)
    names = []
    for k in cols:
        _check(h.L, h.L.potus_column_name(C.byref(h._d), int(k), buf, 96))
        names.append(buf.value.decode())
    return names


def _ranges(h, pars, cols):
    """[(name or None, begin, end, dims)] of the column ranges asked for: parameter names through the layout, sampler columns by name."""
    if pars is not None and cols is not None:
        raise ValueError("monitor: give pars or cols, not both")
    if cols is not None:
        a, b = int(cols[0]), int(cols[1])
        if not (0 <= a < b <= h.n_cols):
            raise ValueError(f"monitor: columns [{a}, {b}) of {h.n_cols}")
        return [(None, a, b, None)]
    if pars is None:
        return [(None, 0, h.n_cols, None)]
    out = []
    for name in ([pars] if isinstance(pars, str) else list(pars)):
        if name in _abi.SAMPLER_COLS:
            k = _abi.SAMPLER_COLS.index(name)
            out.append((name, k, k + 1, ()))
        elif name in h.layout:
            a, b, dims = h.layout[name]
            out.append((name, a, b, dims))
        else:
            raise KeyError(f"unknown parameter {name!r}")
    return out


def monitor(handles, pars=None, cols=None, probs=DEFAULT_PROBS):
    """potus_monitor over the pooled post-warm-up draws of the listed handles (one posterior, one GPU or several).  pars: parameter names of
    Handle.layout or sampler columns ("mu_c", "polling_bias", "lp__", ...); cols: a (begin, end) column range instead; neither: the whole row."""
    hs, ids = _handle_ids(handles)
    h0 = hs[0]
    p = _probs(probs)
    parts, names, blocks, row = [], [], {}, 0
    for name, a, b, dims in _ranges(h0, pars, cols):
        t = np.zeros((b - a, N_STATS + p.size))
        _check(h0.L, h0.L.potus_monitor(ids, len(hs), a, b, _dp(p) if p.size else None, int(p.size), _dp(t)))
        parts.append(t)
        names += _column_names(h0, range(a, b))
        if name is not None:
            blocks[name] = (row, row + b - a, dims)
        row += b - a
    if pars is None:                                               # a plain range: every parameter that lies wholly inside it can be asked for by name
        a0 = 0 if cols is None else int(cols[0])
        for name, (a, b, dims) in h0.layout.items():
            if a >= a0 and b <= a0 + row:
                blocks[name] = (a - a0, b - a0, dims)
    return Monitor(np.concatenate(parts, axis=0), names, p, blocks, sum(h.opts.chains for h in hs), h0.post_warmup_saved())


def monitor_of_block(block, probs=DEFAULT_PROBS, names=None, n_draws=None, n_chains=None, n_cols=None, device=0):
    """potus_monitor_device on a block [draws, chains, columns] that sits on a GPU: a torch tensor (float64, contiguous), or a device pointer
    (an int / ctypes.c_void_p) with n_draws, n_chains, n_cols and the device given.  Every row of the block counts as a draw."""
    p = _probs(probs)
    L = load_library()
    if isinstance(block, (int, C.c_void_p)):
        if n_draws is None or n_chains is None or n_cols is None:
            raise TypeError("monitor_of_block: a device pointer needs n_draws, n_chains and n_cols")
        ptr, nd, nc, ncol, dev = (block if isinstance(block, C.c_void_p) else C.c_void_p(block)), int(n_draws), int(n_chains), int(n_cols), int(device)
    else:
        _device_block(block, "monitor_of_block", ("draws", "chains", "columns"))
        nd, nc, ncol = (int(x) for x in block.shape)
        ptr, dev = C.c_void_p(block.data_ptr()), int(block.device.index or 0)
    t = np.zeros((ncol, N_STATS + p.size))
    _check(L, L.potus_monitor_device(dev, ptr, nd, nc, ncol, _dp(p) if p.size else None, int(p.size), _dp(t)))
    return Monitor(t, names if names is not None else [f"V{k + 1}" for k in range(ncol)], p, None, nc, nd)
