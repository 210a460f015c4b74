"""The dense-metric kernels at the edges of their tiles and panels (csrc/potus_dense.hpp, csrc/potus_dense_pool.hpp), through the four probes of
include/potus_hmc_debug.h on the inputs of tests/dense_edge_cases.py (tests/test_dense_edges_host.py holds those inputs and their references
to numpy, and shows that every window-end case is conditioned well enough for its forward comparison to mean something).  Both storages
everywhere: POTUS_PROBE_F32 = 1 runs the probes with metric_storage = f32 on caller data.

  A  per-chain product   k_dn_symv<NRHS, F32> + k_dn_symv_finish     M x in np.longdouble (float64 beyond D = 1024)   the tolerances of
  B  pooled product      k_dn_pool_mm<NT, F32> + k_dn_pool_finish    the same, one matrix for every chain             tests/test_gpu_dense.py
  C  window end          k_dn_center, k_dn_cov, dense_cholesky_launch (k_dn_potrf, k_dn_trsm, k_dn_syrk, k_dn_syrk_wide), k_dn_trsv_*
  D  pooled window end   k_dn_pool_center, k_dn_pool_cov, k_dn_pool_scale, the factor in its own buffer

Legs C and D: the covariance against covar_adaptation::learn_covariance in np.longdouble; the backward-stable residuals L L' against the
device's own matrix and L' p against u at the tolerances of tests/test_gpu_dense.py; L against numpy's Cholesky factor of the device's matrix
and p against scipy's triangular solve under 8 D eps kappa_2 times the scale of the result (tests/test_gpu_laplace.py, check_draws), kappa_2
from eigvalsh of the device's matrix and that bound itself at most 1e-6.  Every probe call of legs A and B is made twice and must repeat
its bytes; every leg prints its worst deviation before it asserts.

Measured on an MI355X (largest over the cases of a leg): A and B 1e-4 of the tolerance, the fused dot 7e-16 relative; C and D the covariance 8e-16 of
max |M| (fp32 storage: 5.2e-8, the rounding), L L' - M 1.6e-15, |L' p - u| / |u| 1.7e-14, L 1e-13 and p 7e-12 against 8 D eps kappa_2 of 1e-9 to 6.3e-8.
The 196 cases take 17 s together, none more than 2.3 s (D = 16 384: a 2 GB matrix built, rounded, uploaded and multiplied)."""
import ctypes as C

import numpy as np
import pytest
from scipy.linalg import solve_triangular

import dense_edge_cases as cases
from us_potus_model_amd import sampler

pytestmark = pytest.mark.gpu
DP = C.POINTER(C.c_double)
STORAGE = ("fp64", "fp32")


def _lib():
    L = sampler.load_library()
    L.potus_dense_matvec_probe.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, DP, C.POINTER(C.c_longlong)]
    L.potus_dense_factor_probe.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, DP]
    L.potus_dense_pool_matvec_probe.argtypes = L.potus_dense_matvec_probe.argtypes
    L.potus_dense_pool_factor_probe.argtypes = L.potus_dense_factor_probe.argtypes
    return L


def _product(M, x, pooled, times=2):
    """the probe on the matrix M ([chains, D, D], pooled: [D, D]) and x [chains, nrhs, D], `times` times: -> (y, dot, bytes of matrix per pass)"""
    L = _lib()
    chains, nrhs, D = x.shape
    M, x = np.ascontiguousarray(M), np.ascontiguousarray(x)
    fn = L.potus_dense_pool_matvec_probe if pooled else L.potus_dense_matvec_probe
    out = []
    for _ in range(times):
        y, dot, ms, nb = np.full((chains, nrhs, D), np.nan), np.full(chains, np.nan), C.c_double(), C.c_longlong()
        assert fn(0, chains, D, nrhs, M.ctypes.data, x.ctypes.data, y.ctypes.data, dot.ctypes.data, 1, C.byref(ms), C.byref(nb)) == 0
        out.append((y, dot, nb.value))
    for y, dot, _ in out[1:]:
        assert y.tobytes() == out[0][0].tobytes() and dot.tobytes() == out[0][1].tobytes()          # reproducible bit for bit
    return out[0]


def _product_against(y, dot, x, yref, dotref, who):
    """the assertions of test_dense_matvec_against_numpy / test_pooled_product_against_numpy; -> the deviation in units of the tolerance"""
    D = x.shape[2]
    tol = 1e-12 * float(np.abs(yref).max()) * np.sqrt(D)
    err = float(np.abs(y - yref).max())
    dref = np.asarray(dotref, dtype=np.float64)
    print(f"{who}: |y - M x|max {err:.2e} <= {tol:.2e}; fused dot {np.abs(dot / dref - 1).max():.1e} relative")
    assert np.isfinite(y).all() and err <= tol, who
    assert np.allclose(dot, dref, rtol=1e-11), who
    return err / tol


# ---------------------------------------------------------------------------------------------------- A. per-chain product
@pytest.mark.parametrize("f32", [0, 1], ids=STORAGE)
@pytest.mark.parametrize("D", cases.SYMV_D)
def test_per_chain_product_at_the_tile_edges(D, f32, monkeypatch):
    """nrhs = 1, 2, 3 (k_dn_symv<1>, <2>, <2> + <1>) with two or three chains.  The lower triangle handed in is NaN: the kernel selects what counts,
    so one element read from the wrong side of the diagonal or from beyond the right edge -- past column LD a row runs into the next row's leading
    doubles, with fp32 storage a row's floats do so from column D on -- shows in the result.  (It did: the fp64 pass multiplied those by a zero of x
    and returned NaN at every D > 1 whose LD is no multiple of 512, until its last tile was masked like the fp32 pass's.)  fp32: the product is the
    rounded matrix's, and it is NOT the unrounded matrix's."""
    monkeypatch.setenv("POTUS_PROBE_F32", str(f32))
    for nrhs in cases.SYMV_NRHS:
        chains = cases.symv_chains(D, nrhs)
        M = cases.symv_matrices(chains, D)
        x, yref, dotref = cases.symv_case(D, nrhs, f32)
        y, dot, _ = _product(cases.poisoned(M), x, False)
        who = f"D = {D}, {chains} chains, nrhs = {nrhs}, {STORAGE[f32]}"
        _product_against(y, dot, x, yref, dotref, who)
        if f32 and D > 1:
            y64 = cases.symv_case(D, nrhs, 0)[1]
            assert np.abs(y - y64).max() > 100 * 1e-12 * float(np.abs(y64).max()) * np.sqrt(D), who     # (the host file: the two references are that far apart)


@pytest.mark.parametrize("f32", [0, 1], ids=STORAGE)
@pytest.mark.parametrize("D", cases.SYMV_BIG_D)
def test_per_chain_product_where_the_row_block_changes(D, f32, monkeypatch):
    """dense_launch_shape: 128 rows per workgroup below D = 8192, 256 from there (8193: a last block of one row), 512 from 16 384.  One chain, two
    right-hand sides; the pass reads as many bytes as a triangle cut into blocks of that size has."""
    monkeypatch.setenv("POTUS_PROBE_F32", str(f32))
    M = cases.big_symv_matrix(D)
    x = cases.symv_rhs(cases.SYMV_BIG_CHAINS, cases.SYMV_BIG_NRHS, D)
    yref, dotref = cases.symv_reference(cases.round32(M) if f32 else M, x, cases.ref_dtype(D))
    y, dot, nbytes = _product(cases.poisoned(M), x, False)
    rb = cases.DN_RB_MAX if D >= cases.RB_MAX_FROM else cases.DN_RB_BIG if D >= cases.RB_BIG_FROM else cases.DN_RB
    LD = (D + 7) // 8 * 8
    tile_end = min(LD, -(-D // cases.DN_CT) * cases.DN_CT)
    want = sum(min(rb, D - r0) * (tile_end - r0 // cases.DN_CT * cases.DN_CT) for r0 in range(0, D, rb)) * (4 if f32 else 8)
    assert nbytes == want, (nbytes, want, rb)
    _product_against(y, dot, x, yref, dotref, f"D = {D}, rb = {rb}, {STORAGE[f32]}")


# ---------------------------------------------------------------------------------------------------- B. pooled product
def _pooled_combos(D, f32, label=""):
    M = cases.pool_matrix(D)
    LD = (D + 7) // 8 * 8
    got = {}
    for chains, nrhs in cases.POOL_RHS:
        x, yref, dotref = cases.pool_case(D, chains, nrhs, f32)
        y, dot, nbytes = _product(M, x, True)
        assert nbytes == (4 if f32 else 8) * D * LD * -(-chains * nrhs // cases.DNP_RMAX)     # the whole matrix once per launch of up to 48 right-hand sides
        _product_against(y, dot, x, yref, dotref, f"pooled{label} D = {D}, {chains} chains x {nrhs} = {chains * nrhs} right-hand sides, {STORAGE[f32]}")
        got[chains, nrhs] = (x, y, dot)
    return M, got


@pytest.mark.parametrize("f32", [0, 1], ids=STORAGE)
@pytest.mark.parametrize("D", cases.POOL_D)
def test_pooled_product_at_the_tile_edges(D, f32, monkeypatch):
    """R = 16, 17, 32, 33, 48 right-hand sides: one, two and three operand tiles, full and with one column in the last; 51 and 50: a second launch of three
    and of two columns.  D around one operand tile of columns, one batch of rows, one panel (256 columns, 512 with fp32 storage), and 1025.  At R = 17
    chains 0 and 16 alone (fifteen idle companions, the compacted list) get the bytes they get in company."""
    monkeypatch.setenv("POTUS_PROBE_F32", str(f32))
    M, got = _pooled_combos(D, f32)
    chains, nrhs = cases.POOL_IDLE
    x, y, dot = got[chains, nrhs]
    monkeypatch.setenv("POTUS_PROBE_ACTIVE", f"0,{chains - 1}")
    y2, dot2, _ = _product(M, x, True, times=1)
    for c in (0, chains - 1):
        assert y2[c].tobytes() == y[c].tobytes() and dot2[c] == dot[c], c


@pytest.mark.parametrize("f32", [0, 1], ids=STORAGE)
@pytest.mark.parametrize("split", cases.POOL_SPLITS)
@pytest.mark.parametrize("D", cases.POOL_SPLIT_D)
def test_pooled_product_with_the_row_split_stated(D, split, f32, monkeypatch):
    """POTUS_POOL_SPLIT = 8: batches of 32 rows, so D = 33 has two splits and D = 257 five, the last of one row each.  3 and 1: other row counts per
    split and none at all.  The numbers agree with numpy at the same tolerance whatever the split (their bytes may depend on it)."""
    monkeypatch.setenv("POTUS_PROBE_F32", str(f32))
    monkeypatch.setenv("POTUS_POOL_SPLIT", str(split))
    _pooled_combos(D, f32, f" (split {split})")


# ---------------------------------------------------------------------------------------------------- C, D. window end
def _window_end(chains, n, D, pooled):
    L = _lib()
    draws, u = cases.window_draws(chains, n, D)
    nm = 1 if pooled else chains
    Mi, Lc, p, ms = np.full((nm, D, D), np.nan), np.full((nm, D, D), np.nan), np.full((chains, D), np.nan), (C.c_double * 3)()
    fn = L.potus_dense_pool_factor_probe if pooled else L.potus_dense_factor_probe
    d, uu = np.ascontiguousarray(draws), np.ascontiguousarray(u)
    assert fn(0, chains, D, n, d.ctypes.data, uu.ctypes.data, Mi.ctypes.data, Lc.ctypes.data, p.ctypes.data, ms) == 0
    return u, Mi, Lc, p


def _check_window_end(chains, n, D, pooled, f32):
    u, Mi, Lc, p = _window_end(chains, n, D, pooled)
    ref = cases.window_reference(chains, n, D, pooled)
    ref = ref[None] if pooled else ref
    worst = dict(cov=0.0, llt=0.0, solve=0.0, L=0.0, p=0.0, bound=0.0)
    for m in range(Mi.shape[0]):
        M, R = Mi[m], ref[m]
        who = (D, n, m, STORAGE[f32])
        scale = np.abs(R).max()
        worst["cov"] = max(worst["cov"], np.abs(M - R).max() / scale)
        # the matrix (per chain, fp64: the upper triangle of the buffer the factorisation has just run in; fp32: the floats in the rows' free halves)
        assert np.isfinite(M).all() and np.array_equal(M, M.T), who                                # exactly symmetric
        if f32:
            assert np.array_equal(M, cases.round32(M)), who                                        # every element an fp32 number
            assert np.allclose(M, R, rtol=1e-7, atol=1e-7 * scale), who
        else:
            assert np.allclose(M, R, rtol=1e-10, atol=1e-12 * scale), who
        # the factor: nothing above the diagonal, L L' is the device's own matrix
        Lg = Lc[m]
        assert np.isfinite(Lg).all() and not np.triu(Lg, 1).any() and (np.diag(Lg) > 0).all(), who
        worst["llt"] = max(worst["llt"], np.abs(Lg @ Lg.T - M).max() / scale)
        assert np.allclose(Lg @ Lg.T, M, rtol=1e-10, atol=1e-12 * scale), who
        # ... and numpy's factor of that matrix, under the bound that carries its conditioning
        bound, ev = cases.forward_bound(M)
        assert bound <= cases.FORWARD_BOUND, (who, bound)
        Lref = np.linalg.cholesky(M)
        worst["bound"] = max(worst["bound"], bound)
        worst["L"] = max(worst["L"], np.abs(Lg - Lref).max() / np.abs(Lref).max())
        assert np.abs(Lg - Lref).max() <= bound * np.abs(Lref).max(), who
        for c in (range(chains) if pooled else [m]):
            assert np.isfinite(p[c]).all(), who
            res = np.linalg.norm(Lg.T @ p[c] - u[c]) / np.linalg.norm(u[c])
            worst["solve"] = max(worst["solve"], res)
            assert res < 1e-9, (who, c, res)                                                       # (the bound of potus_dense_check)
            pdev = solve_triangular(Lg.T, u[c], lower=False)
            assert np.allclose(p[c], pdev, rtol=1e-8, atol=1e-9 * np.abs(pdev).max()), (who, c)
            pref = solve_triangular(Lref.T, u[c], lower=False)
            worst["p"] = max(worst["p"], np.abs(p[c] - pref).max() / np.abs(pref).max())
            assert np.abs(p[c] - pref).max() <= bound * np.abs(pref).max(), (who, c)
    print(f"{'pooled ' if pooled else ''}D = {D}, {chains} x {n} draws, {STORAGE[f32]}: |M - ref| {worst['cov']:.1e}, |L L' - M| {worst['llt']:.1e} (of max |M|), "
          f"|L' p - u| / |u| {worst['solve']:.1e}, |L - chol(M)| {worst['L']:.1e}, |p - solve| {worst['p']:.1e} <= 8 D eps kappa_2 = {worst['bound']:.1e}")


@pytest.mark.parametrize("f32", [0, 1], ids=STORAGE)
@pytest.mark.parametrize("D,n", cases.window_cases())
def test_window_end_at_the_block_and_panel_edges(D, n, f32, monkeypatch):
    """Two chains with different draws.  D: below one block of 64, one block, a panel of four, a second panel of one block (and a row), 127 / 128 / 129
    rows behind the first panel (one wide tile, one exactly, two), two panels, a fourth panel of one row.  n at D = 65 and 257: the legal minimum 2, 3,
    and the 64 draws k_dn_cov reads at a time with their neighbours.  fp32: the fp32 branch of k_dn_cov on caller data -- the matrix that comes back
    is read from the floats in the rows' free halves AFTER the factorisation has run beside them."""
    monkeypatch.setenv("POTUS_PROBE_F32", str(f32))
    _check_window_end(cases.WINDOW_CHAINS, n, D, False, f32)


@pytest.mark.parametrize("f32", [0, 1], ids=STORAGE)
@pytest.mark.parametrize("D,n", cases.pool_window_cases())
def test_pooled_window_end_at_the_block_and_panel_edges(D, n, f32, monkeypatch):
    """Three chains, ONE matrix of their pooled draws and ONE factor in its own buffer, every chain's solve out of it."""
    monkeypatch.setenv("POTUS_PROBE_F32", str(f32))
    _check_window_end(cases.POOL_WINDOW_CHAINS, n, D, True, f32)
