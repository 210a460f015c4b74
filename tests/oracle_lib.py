"""ctypes binding of oracle/libpotus_oracle.so (the CPU checker; tests + bench cpu_baseline only)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from us_potus_model_amd import _abi

ROOT = Path(__file__).resolve().parent.parent
_LIB = None


class OracleOpts(C.Structure):
    _fields_ = [("num_warmup", C.c_int32), ("num_samples", C.c_int32), ("max_depth", C.c_int32),
                ("init_buffer", C.c_int32), ("term_buffer", C.c_int32), ("window", C.c_int32),
                ("delta", C.c_double), ("gamma", C.c_double), ("kappa", C.c_double), ("t0", C.c_double),
                ("stepsize", C.c_double), ("init_radius", C.c_double), ("seed", C.c_uint64),
                ("fast_grad", C.c_int32), ("save_warmup", C.c_int32), ("dense_metric", C.c_int32), ("pooled", C.c_int32)]


def build():
    so = ROOT / "oracle" / "libpotus_oracle.so"
    src = ROOT / "oracle" / "potus_oracle.c"
    if not so.exists() or so.stat().st_mtime < src.stat().st_mtime:
        subprocess.run(["make", "-C", str(ROOT / "oracle")], check=True, capture_output=True)
    return so


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(str(build()))
        dp = C.POINTER(C.c_double)
        L.oracle_model_create.restype = C.c_void_p
        L.oracle_model_create.argtypes = [C.POINTER(_abi.PotusData), C.c_char_p, C.c_int]
        L.oracle_model_free.argtypes = [C.c_void_p]
        L.oracle_num_params.argtypes = [C.c_void_p]
        L.oracle_num_columns.argtypes = [C.c_void_p]
        L.oracle_cholesky_factors.argtypes = [C.c_void_p, dp, dp, dp]
        for f in (L.oracle_log_prob_grad, L.oracle_log_prob_grad_fast):
            f.restype = C.c_double
            f.argtypes = [C.c_void_p, dp, dp]
        L.oracle_write_array.argtypes = [C.c_void_p, dp, dp]
        L.oracle_default_opts.argtypes = [C.POINTER(OracleOpts)]
        L.oracle_sample_chain.argtypes = [C.c_void_p, C.POINTER(OracleOpts), C.c_int, dp, dp, dp,
                                          C.POINTER(C.c_longlong)]
        L.oracle_sample_chain_metric.argtypes = [C.c_void_p, C.POINTER(OracleOpts), C.c_int, dp, dp, dp,
                                                 C.POINTER(C.c_longlong), dp]
        L.oracle_window_ends.argtypes = [C.POINTER(OracleOpts), C.POINTER(C.c_int), C.c_int]
        L.oracle_sample_chain_timed.argtypes = [C.c_void_p, C.POINTER(OracleOpts), C.c_int, dp, dp, dp, C.c_double]
        L.oracle_transitions_from.argtypes = [C.c_void_p, C.POINTER(OracleOpts), C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp]
        L.oracle_init_stepsize_from.restype = C.c_double
        L.oracle_init_stepsize_from.argtypes = [C.c_void_p, C.POINTER(OracleOpts), C.c_int, C.c_uint32, dp, C.c_double, dp, dp]
        L.oracle_time_leapfrogs_dense.restype = C.c_double
        L.oracle_time_leapfrogs_dense.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
        L.oracle_philox.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.oracle_rng_uniform.restype = C.c_double
        L.oracle_rng_uniform.argtypes = [C.c_uint64] + [C.c_uint32] * 5
        L.oracle_rng_normal_pair.argtypes = [C.c_uint64] + [C.c_uint32] * 5 + [dp, dp]
        L.oracle_time_leapfrogs.restype = C.c_double
        L.oracle_time_leapfrogs.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_uint64]
        _LIB = L
    return _LIB


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class OracleModel:
    def __init__(self, data: dict, variant="full"):
        self.L = lib()
        self._d, self._keep = _abi.make_data(data, variant)
        err = C.create_string_buffer(256)
        self.h = self.L.oracle_model_create(C.byref(self._d), err, 256)
        if not self.h:
            raise ValueError(err.value.decode())
        self.D = self.L.oracle_num_params(self.h)
        self.n_cols = self.L.oracle_num_columns(self.h)
        self.S = int(data["S"])

    def __del__(self):
        if getattr(self, "h", None):
            self.L.oracle_model_free(self.h)
            self.h = None

    def cholesky(self):
        S = self.S
        out = [np.zeros(S * S) for _ in range(3)]
        self.L.oracle_cholesky_factors(self.h, *[_dp(o) for o in out])
        return [o.reshape(S, S).T.copy() for o in out]  # L_B, L_T, L_W as row-major numpy

    def log_prob_grad(self, q, fast=False):
        q = np.ascontiguousarray(q, dtype=np.float64)
        g = np.zeros(self.D)
        f = self.L.oracle_log_prob_grad_fast if fast else self.L.oracle_log_prob_grad
        lp = f(self.h, _dp(q), _dp(g))
        return lp, g

    def write_array(self, q):
        q = np.ascontiguousarray(q, dtype=np.float64)
        out = np.zeros(self.n_cols - _abi.N_SAMPLER_COLS)
        self.L.oracle_write_array(self.h, _dp(q), _dp(out))
        return out

    def default_opts(self, **kw):
        o = OracleOpts()
        self.L.oracle_default_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def sample_chain(self, chain_id, opts, q0=None):
        n_saved = opts.num_samples + (opts.num_warmup if opts.save_warmup else 0)
        draws = np.zeros((n_saved, _abi.N_SAMPLER_COLS + self.D))
        adapt = np.zeros(1 + self.D)
        nl = C.c_longlong(0)
        q0p = _dp(np.ascontiguousarray(q0, dtype=np.float64)) if q0 is not None else None
        rc = self.L.oracle_sample_chain(self.h, C.byref(opts), chain_id, q0p, _dp(draws), _dp(adapt), C.byref(nl))
        if rc:
            raise RuntimeError(f"oracle_sample_chain failed rc={rc}")
        return draws, adapt, nl.value

    def window_ends(self, opts):
        """The warm-up iterations (0-based) after which sample_chain updates the metric under opts."""
        ends = (C.c_int * 64)()
        n = self.L.oracle_window_ends(C.byref(opts), ends, 64)
        assert n <= 64
        return list(ends[:n])

    def sample_chain_timed(self, chain_id, opts, budget_s=0.0):
        """sample_chain + (warm-up seconds, sampling seconds, warm-up leapfrogs, sampling leapfrogs, iterations done):
        bench.py's cpu_baseline; budget_s > 0 cuts the run at the first iteration boundary after that many seconds."""
        n_saved = opts.num_samples + (opts.num_warmup if opts.save_warmup else 0)
        draws = np.zeros((n_saved, _abi.N_SAMPLER_COLS + self.D))
        adapt = np.zeros(1 + self.D)
        timing = np.zeros(5)
        rc = self.L.oracle_sample_chain_timed(self.h, C.byref(opts), chain_id, _dp(draws), _dp(adapt), _dp(timing), float(budget_s))
        if rc:
            raise RuntimeError(f"oracle_sample_chain_timed failed rc={rc}")
        return draws, adapt, timing

    def sample_chain_metric(self, chain_id, opts, q0=None):
        """sample_chain + the adapted inverse metric as a D x D matrix (diag(minv) for the diagonal metric)."""
        n_saved = opts.num_samples + (opts.num_warmup if opts.save_warmup else 0)
        draws = np.zeros((n_saved, _abi.N_SAMPLER_COLS + self.D))
        adapt = np.zeros(1 + self.D)
        metric = np.zeros((self.D, self.D))
        nl = C.c_longlong(0)
        q0p = _dp(np.ascontiguousarray(q0, dtype=np.float64)) if q0 is not None else None
        rc = self.L.oracle_sample_chain_metric(self.h, C.byref(opts), chain_id, q0p, _dp(draws), _dp(adapt), C.byref(nl), _dp(metric))
        if rc:
            raise RuntimeError(f"oracle_sample_chain_metric failed rc={rc}")
        return draws, adapt, nl.value, metric

    def transitions_from(self, chain_id, opts, iter0, qs, eps, minv, chol=None):
        """Single transitions from given states: row t starts at qs[t] with step size eps[t] and RNG iteration iter0 + t under the
        metric handed in (dense: minv [D, D] and its lower Cholesky factor chol; diagonal: minv [D]).  Returns rows [n, 7 + D]."""
        qs = np.ascontiguousarray(np.atleast_2d(qs), dtype=np.float64)
        eps = np.ascontiguousarray(np.atleast_1d(eps), dtype=np.float64)
        minv = np.ascontiguousarray(minv, dtype=np.float64)
        n = qs.shape[0]
        rows = np.zeros((n, _abi.N_SAMPLER_COLS + self.D))
        cp = _dp(np.ascontiguousarray(chol, dtype=np.float64)) if chol is not None else None
        rc = self.L.oracle_transitions_from(self.h, C.byref(opts), chain_id, int(iter0), n, _dp(qs), _dp(eps), _dp(minv), cp, _dp(rows))
        if rc:
            raise RuntimeError(f"oracle_transitions_from failed rc={rc}")
        return rows

    def init_stepsize_from(self, chain_id, opts, iteration, q, eps0, minv, chol=None):
        """base_hmc::init_stepsize at q from eps0 under the given metric, momentum draws of RNG iteration `iteration`."""
        q = np.ascontiguousarray(q, dtype=np.float64)
        minv = np.ascontiguousarray(minv, dtype=np.float64)
        cp = _dp(np.ascontiguousarray(chol, dtype=np.float64)) if chol is not None else None
        return self.L.oracle_init_stepsize_from(self.h, C.byref(opts), chain_id, int(iteration) & 0xFFFFFFFF, _dp(q), float(eps0), _dp(minv), cp)

    def time_leapfrogs_dense(self, n, eps=0.01, seed=1):
        """(seconds, OpenMP threads, bytes of the matrix) of n leapfrogs of one chain under a dense D x D inverse metric."""
        nt, nb = C.c_int(0), C.c_longlong(0)
        secs = self.L.oracle_time_leapfrogs_dense(self.h, int(n), float(eps), int(seed), C.byref(nt), C.byref(nb))
        return secs, nt.value, nb.value

    def time_leapfrogs(self, n, eps=0.01, fast=False, seed=1):
        return self.L.oracle_time_leapfrogs(self.h, n, eps, int(fast), seed)
