"""The machinery of tests/test_gpu_dense_edges.py without a GPU (tests/dense_edge_cases.py): the constants the case lists are derived from
against the text of csrc/potus_dense.hpp, csrc/potus_dense_pool.hpp and dense_launch_shape; every edge in its list; the np.longdouble
references against float64 numpy; the fp32 rounding helper; and, for every window-end case, that the conditioning-scaled bound of the
forward comparisons cannot hide a failure: 8 D eps kappa_2 of the reference matrix (and of its fp32 rounding) is at most 1e-6 and numpy
factors it."""
import re
import struct

import numpy as np
import pytest

import dense_edge_cases as cases
from conftest import ROOT

CSRC = ROOT / "us_potus_model_amd" / "csrc"


def _define(text, name):
    m = re.search(rf"^#define {name}\s+(\S+)", text, re.M)
    assert m, name
    return m.group(1)


def test_the_constants_are_the_headers():
    dense, pool, hip = (CSRC / "potus_dense.hpp").read_text(), (CSRC / "potus_dense_pool.hpp").read_text(), (CSRC / "potus_hmc.hip").read_text()
    for name in ("DN_NB", "DN_PANEL", "DN_WT", "DN_RB", "DN_RB_BIG", "DN_RB_MAX", "DN_CT"):
        assert int(_define(dense, name)) == getattr(cases, name), name
    for name in ("DNP_COLS", "DNP_KB", "DNP_RMAX"):
        assert int(_define(pool, name)) == getattr(cases, name), name
    assert _define(dense, "DN_FIN") == "256" and _define(dense, "DN_THREADS") == "512"
    # fp32 storage: four operand tiles of 128 columns; two or three operand tiles of right-hand sides: batches of 16 rows
    assert "#define DNP_CT(F32) ((F32) ? 4 : 2)" in pool and "#define DNP_COLS_OF(F32) (128 * DNP_CT(F32))" in pool
    assert cases.DNP_COLS == 128 * 2 and cases.DNP_COLS_F32 == 128 * 4
    assert f"#define DNP_KB_OF(NT, F32) ((NT) >= 2 ? {cases.DNP_KB_TILES} : DNP_KB)" in pool
    # the row-block size by D, the draws k_dn_cov reads at a time, the panels of the factorisation
    assert "P.rb = P.D >= 32 * DN_RB_MAX ? DN_RB_MAX : P.D >= 32 * DN_RB_BIG ? DN_RB_BIG : DN_RB;" in hip
    assert (cases.RB_BIG_FROM, cases.RB_MAX_FROM) == (8192, 16384)
    assert dense.count("for (int k0 = 0; k0 < n; k0 += DN_NB) {") == 1 and pool.count("for (int k0 = 0; k0 < n; k0 += DN_NB) {") == 1
    assert "for (int pb = 0; pb < nb; pb += DN_PANEL) {" in hip and "const int nt = (behind + DN_WT - 1) / DN_WT;" in hip
    assert cases.PANEL == 256


def test_every_edge_is_in_its_list():
    NB, PANEL, WT, RB, CT = cases.DN_NB, cases.PANEL, cases.DN_WT, cases.DN_RB, cases.DN_CT
    # per-chain product: below one block, every multiple of the row block up to one column tile with its neighbours, a last tile of 1 .. 5 columns
    want = {1, 2, 7, 8, 9} | {k * RB + d for k in (1, 2, 3, 4) for d in (-1, 0, 1)} | {CT + d for d in (1, 2, 3, 5)}
    assert want <= set(cases.SYMV_D)
    assert {cases.RB_BIG_FROM + d for d in (-1, 0, 1)} | {cases.RB_MAX_FROM - 1, cases.RB_MAX_FROM} == set(cases.SYMV_BIG_D)
    assert {cases.symv_chains(D, r) for D in cases.SYMV_D for r in cases.SYMV_NRHS} == {2, 3}
    for D in cases.SYMV_D:                                   # every size meets both chain counts
        assert {cases.symv_chains(D, r) for r in cases.SYMV_NRHS} == {2, 3}
    # pooled product: a 16-column operand tile, a batch of 32 rows, a panel of 256 (fp32: 512) columns, each with its neighbours; right-hand sides at
    # the edges of the operand tiles and beyond one launch
    want = {1, 1025} | {e + d for e in (16, cases.DNP_KB, cases.DNP_COLS, cases.DNP_COLS_F32) for d in (-1, 0, 1)}
    assert want <= set(cases.POOL_D)
    R = [c * r for c, r in cases.POOL_RHS]
    assert R == [16, 17, 32, 33, 48, 51, 50] and {-(-v // 16) for v in R if v <= cases.DNP_RMAX} == {1, 2, 3} and cases.POOL_IDLE in cases.POOL_RHS
    for D in cases.POOL_SPLIT_D:                             # eight splits asked for: batches of DNP_KB rows, the last split one row
        rows = -(-(-(-D // 8)) // cases.DNP_KB) * cases.DNP_KB
        assert D % rows == 1
    # window end
    want = {1, 2} | {NB + d for d in (-1, 0, 1)} | {2 * NB} | {PANEL + d for d in (-1, 0, 1)} | {PANEL + NB + d for d in (-1, 0, 1)}
    want |= {PANEL + WT + d for d in (-1, 0, 1)} | {2 * PANEL + d for d in (-1, 0, 1)} | {3 * PANEL + 1}
    assert want <= set(cases.WINDOW_D)
    assert [D - PANEL for D in (383, 384, 385)] == [WT - 1, WT, WT + 1]
    assert {2, 3} | {NB + d for d in (-1, 0, 1)} | {2 * NB, 2 * NB + 1} == set(cases.WINDOW_N)
    per_chain = cases.window_cases()
    assert {(D, n) for D in cases.WINDOW_N_D for n in cases.WINDOW_N} <= set(per_chain) and len(per_chain) == len(set(per_chain)) == 33
    assert {1, 2, NB - 1, NB, NB + 1, PANEL - 1, PANEL, PANEL + 1, PANEL + NB, PANEL + NB + 1, PANEL + WT - 1, PANEL + WT, PANEL + WT + 1,
            2 * PANEL, 2 * PANEL + 1, 3 * PANEL + 1} <= set(cases.POOL_WINDOW_D)
    assert [cases.POOL_WINDOW_CHAINS * n for _, n in cases.POOL_WINDOW_N] == [6, 63, 66, 129]


def test_the_finishing_kernel_starts_at_the_rows_own_tile_for_every_block_size():
    """k_dn_symv_finish adds the row sums of row i from tile ((i / rb) * rb) / DN_CT on.  Every block size divides the tile, so that is i / DN_CT
    whichever of them the launch took -- which is why a finish that used another of the three block sizes there would give the same bytes."""
    i = np.arange(3 * cases.RB_MAX_FROM)
    for rb in (cases.DN_RB, cases.DN_RB_BIG, cases.DN_RB_MAX):
        assert cases.DN_CT % rb == 0 and np.array_equal((i // rb * rb) // cases.DN_CT, i // cases.DN_CT)


def test_the_fp32_rounding_helper():
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.standard_normal(2000) * 10.0 ** rng.integers(-6, 6, 2000), [0.0, -0.0, 1.0, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -23, 1.0 + 3 * 2.0 ** -24]])
    r = cases.round32(a)
    assert r.dtype == np.float64 and np.array_equal(cases.round32(r), r)
    assert np.array_equal(r, [struct.unpack("f", struct.pack("f", v))[0] for v in a])            # C's (float) conversion
    assert np.all(np.abs(r - a) <= 2.0 ** -24 * np.abs(a))
    assert r[-3] == 1.0 and r[-2] == 1.0 + 2.0 ** -23 and r[-1] == 1.0 + 2.0 ** -22             # ties go to the even neighbour
    M = cases.symv_matrices(2, 129)
    assert not np.array_equal(cases.round32(M), M) and np.array_equal(cases.round32(M), np.transpose(cases.round32(M), (0, 2, 1)))


def test_the_poisoned_matrix_keeps_the_upper_triangle_and_the_diagonal():
    M = cases.symv_matrices(3, 9)
    P = cases.poisoned(M)
    iu, il = np.triu_indices(9), np.tril_indices(9, -1)
    assert np.array_equal(P[:, iu[0], iu[1]], M[:, iu[0], iu[1]]) and np.isnan(P[:, il[0], il[1]]).all() and M.flags.writeable is False


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("D", cases.SYMV_D)
def test_product_references_against_float64(D, f32):
    for nrhs in cases.SYMV_NRHS:
        chains = cases.symv_chains(D, nrhs)
        M = cases.symv_matrices(chains, D)
        x, y, dot = cases.symv_case(D, nrhs, f32)
        assert y.dtype == np.longdouble and y.shape == (chains, nrhs, D) and not y.flags.writeable
        Mu = cases.round32(M) if f32 else M
        assert np.array_equal(Mu, np.transpose(Mu, (0, 2, 1))) and np.linalg.eigvalsh(M).min() >= 1.0 - 1e-12
        y64 = np.einsum("cij,crj->cri", Mu, x)
        assert np.abs(y64 - y).max() <= 4 * D * cases.EPS * np.abs(y64).max()
        assert np.allclose(np.einsum("ci,ci->c", x[:, 0], y64[:, 0]), np.asarray(dot, dtype=np.float64), rtol=1e-13, atol=0)
        if f32 and D > 1:                                    # the rounded matrix gives another product, far outside the tolerance of the GPU test
            y_unrounded = cases.symv_case(D, nrhs, 0)[1]
            assert np.abs(y_unrounded - y).max() > 100 * 1e-12 * float(np.abs(y).max()) * np.sqrt(D)


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("D", cases.POOL_D)
def test_pooled_product_references_against_float64(D, f32):
    M = cases.pool_matrix(D)
    Mu = cases.round32(M) if f32 else M
    for chains, nrhs in cases.POOL_RHS:
        x, y, dot = cases.pool_case(D, chains, nrhs, f32)
        assert y.dtype == cases.ref_dtype(D) and y.shape == (chains, nrhs, D)
        y64 = np.einsum("ij,crj->cri", Mu, x)
        assert np.abs(y64 - y).max() <= 4 * D * cases.EPS * np.abs(y64).max()
        assert np.allclose(np.einsum("ci,ci->c", x[:, 0], y64[:, 0]), np.asarray(dot, dtype=np.float64), rtol=1e-13, atol=0)


def _condition(M, who):
    """numpy factors it, and 8 D eps kappa_2 is small enough that the forward comparisons of the GPU test mean something"""
    np.linalg.cholesky(M)
    bound, ev = cases.forward_bound(M)
    assert ev[0] > 0 and bound <= cases.FORWARD_BOUND, (who, bound, ev[0], ev[-1])
    return bound


@pytest.mark.parametrize("D,n", cases.window_cases())
def test_window_cases_are_well_conditioned_and_their_reference_is_numpys(D, n):
    draws, u = cases.window_draws(cases.WINDOW_CHAINS, n, D)
    ref = cases.window_reference(cases.WINDOW_CHAINS, n, D, False)
    assert draws.shape == (cases.WINDOW_CHAINS, n, D) and not np.array_equal(draws[0], draws[1]) and not draws.flags.writeable
    worst = 0.0
    for c in range(cases.WINDOW_CHAINS):
        np64 = (n / (n + 5.0)) * np.cov(draws[c].T).reshape(D, D) + 1e-3 * (5.0 / (n + 5.0)) * np.eye(D)
        assert np.allclose(ref[c], np64, rtol=1e-11, atol=1e-13 * np.abs(np64).max()) and np.array_equal(ref[c], ref[c].T)
        if n - 1 < D:                                        # rank-deficient covariance: the regulariser is the smallest eigenvalue
            assert np.isclose(np.linalg.eigvalsh(ref[c])[0], 1e-3 * 5.0 / (n + 5.0), rtol=1e-6)
        worst = max(worst, _condition(ref[c], (D, n, c, "fp64")), _condition(cases.round32(ref[c]), (D, n, c, "fp32")))
    print(f"D = {D}, n = {n}: 8 D eps kappa_2 <= {worst:.2e}")


@pytest.mark.parametrize("D,n", cases.pool_window_cases())
def test_pooled_window_cases_are_well_conditioned_and_their_reference_is_numpys(D, n):
    chains = cases.POOL_WINDOW_CHAINS
    draws, u = cases.window_draws(chains, n, D)
    ref = cases.window_reference(chains, n, D, True)
    N = chains * n
    np64 = (N / (N + 5.0)) * np.cov(draws.reshape(N, D).T).reshape(D, D) + 1e-3 * (5.0 / (N + 5.0)) * np.eye(D)
    assert np.allclose(ref, np64, rtol=1e-11, atol=1e-13 * np.abs(np64).max()) and np.array_equal(ref, ref.T)
    worst = max(_condition(ref, (D, n, "fp64")), _condition(cases.round32(ref), (D, n, "fp32")))
    print(f"D = {D}, {chains} x {n} draws: 8 D eps kappa_2 <= {worst:.2e}")
