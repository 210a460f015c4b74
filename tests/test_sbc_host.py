"""CPU tests of the simulation-based-calibration layer (us_potus_model_amd/sbc.py) and of the new entry points' error paths."""
import ctypes as C

import numpy as np
import pytest

from us_potus_model_amd import _abi, sampler, sbc


def test_uniformity_accepts_uniform_and_rejects_u_shaped_and_shifted_ranks():
    rng = np.random.default_rng(11)
    L, n = 99, 1000
    uniform = rng.integers(0, L + 1, (n, 3))
    assert (sbc.uniformity(uniform, L) > 0.01).all()
    u_shaped = np.where(rng.random((n, 1)) < 0.5, rng.integers(0, 15, (n, 1)), rng.integers(L - 14, L + 1, (n, 1)))
    shifted = np.minimum(L, rng.integers(0, L + 1, (n, 1)) + 30)
    assert sbc.uniformity(u_shaped, L)[0] < 1e-6
    assert sbc.uniformity(shifted, L)[0] < 1e-6


def test_uniformity_bins_with_unequal_widths():
    # L + 1 = 7 values over 3 bins: widths 2, 2, 3 -- exactly proportional counts are a perfect fit
    ranks = np.repeat(np.arange(7), 10)[:, None]
    counts, edges = sbc.histograms(ranks, 6, 3)
    assert list(np.diff(edges)) == [2, 2, 3] and list(counts[0]) == [20, 20, 30]
    assert sbc.uniformity(ranks, 6, 3)[0] == pytest.approx(1.0)


def test_tie_breaking_stays_within_less_and_less_plus_equal():
    rng = np.random.default_rng(3)
    less = rng.integers(0, 50, (400, 5))
    equal = rng.integers(0, 4, (400, 5))
    r = sbc.break_ties(less, equal, seed=5)
    assert ((r >= less) & (r <= less + equal)).all()
    assert (r[equal == 0] == less[equal == 0]).all()
    assert np.array_equal(r, sbc.break_ties(less, equal, seed=5))
    # every value of the tie range is reached
    r = sbc.break_ties(np.zeros(4000, int), np.full(4000, 3), seed=1)
    assert set(np.unique(r)) == {0, 1, 2, 3}


@pytest.mark.parametrize("n_sims,chains_per_sim,max_chains", [(256, 2, 512), (300, 2, 128), (7, 3, 5), (5, 4, 1), (1, 1, 1024)])
def test_batching_plan_covers_every_sim_and_chain_once(n_sims, chains_per_sim, max_chains):
    plan = sbc.plan_batches(n_sims, chains_per_sim, max_chains)
    seen = []
    for s0, ns in plan:
        assert ns >= 1 and (ns * chains_per_sim <= max_chains or ns == 1)
        seen += [(s0 + i, c) for i in range(ns) for c in range(chains_per_sim)]
    assert sorted(seen) == [(s, c) for s in range(n_sims) for c in range(chains_per_sim)]


def test_chains_cap_follows_the_memory_cap(cases):
    data, variant = cases["2016"]
    D = _abi.num_params(data, variant)
    n = sbc.chains_cap(data, variant, 1000, 1000, mem_cap=1 << 30)
    assert n == max(1, (1 << 30) // ((1000 * (7 + D) + 80 * (D + 8)) * 8))
    assert sbc.chains_cap(*cases["small_full"], 1000, 1000) == 1024


def test_column_names_resolve_to_the_layout(cases):
    data, variant = cases["small_full"]
    layout, ncols = _abi.column_layout(data, variant)
    S, T = int(data["S"]), int(data["T"])
    assert sbc.column_index(data, variant, f"mu_b.2.{T}") == layout["mu_b"][0] + 1 + S * (T - 1)
    assert sbc.column_index(data, variant, f"predicted_score.{T}.1") == layout["predicted_score"][0] + T - 1
    assert sbc.column_index(data, variant, "mu_e_bias") == layout["mu_e_bias"][0]
    for c in sbc.default_columns(data, variant):
        assert 7 <= sbc.column_index(data, variant, c) < ncols
    with pytest.raises(KeyError):
        sbc.column_index(data, variant, f"mu_b.{S + 1}.1")
    assert "mu_e_bias" not in sbc.default_columns(*cases["small_nomode"])


def _err(L):
    buf = C.create_string_buffer(256)
    L.potus_last_error(buf, 256)
    return buf.value.decode()


def test_new_entry_points_fail_cleanly_on_a_bad_handle():
    L = sampler.load_library()
    i32 = np.zeros(8, np.int32)
    f64 = np.zeros(8)
    ip = i32.ctypes.data_as(C.POINTER(C.c_int32))
    dp = f64.ctypes.data_as(C.POINTER(C.c_double))
    n = C.c_int()
    for rc in (L.potus_set_datasets(12345, 2, ip, ip), L.potus_simulate_prior(12345, 1, 2, 0, dp, ip, ip),
               L.potus_constrain(12345, dp, 1, 7, 8, dp), L.potus_sbc_ranks(12345, dp, 7, 8, 1, ip, ip, C.byref(n))):
        assert rc == 4 and _err(L) == "bad handle"
    st = C.c_int(0)
    h = C.c_int(-3)
    two = (C.c_int * 3)(7, 8, 1)
    L.potus_R_set_datasets.argtypes = [C.POINTER(C.c_int)] * 5
    L.potus_R_set_datasets(C.byref(h), C.byref(C.c_int(2)), ip, ip, C.byref(st))
    assert st.value == 4 and _err(L) == "bad handle"
    st.value = 0
    L.potus_R_simulate_prior(C.byref(h), C.byref(C.c_double(1843.0)), (C.c_int * 2)(2, 0), dp, ip, ip, C.byref(st))
    assert st.value == 4 and _err(L) == "bad handle"
    st.value = 0
    L.potus_R_simulate_prior(C.byref(h), C.byref(C.c_double(-1.0)), (C.c_int * 2)(2, 0), dp, ip, ip, C.byref(st))
    assert st.value == 1 and "seed" in _err(L)
    st.value = 0
    L.potus_R_sbc_ranks(C.byref(h), dp, two, ip, ip, C.byref(n), C.byref(st))
    assert st.value == 4 and _err(L) == "bad handle"
    st.value = 0
    L.potus_R_constrain(C.byref(h), dp, C.byref(C.c_int(1)), two, dp, C.byref(st))
    assert st.value == 4 and _err(L) == "bad handle"


def test_pooled_entry_points_refuse_a_null_list_and_an_unknown_handle():
    """Every entry point that takes a list of handles: a null list is an argument error (1) and handle 12345 a state error (4) whose message
    names the handle -- decided on the host, before any HIP call (this machine may have no GPU)."""
    L = sampler.load_library()
    f64 = np.zeros(64)
    dp = f64.ctypes.data_as(C.POINTER(C.c_double))
    ip = C.POINTER(C.c_int)
    n, ll = C.c_int(), C.c_longlong()
    L.potus_extract_matrix.argtypes = [ip, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_longlong)]
    calls = {
        "potus_extract_matrix": lambda h, k: L.potus_extract_matrix(h, k, 0, 1, None, 0, C.byref(ll)),
        "potus_posterior_summary_many": lambda h, k: L.potus_posterior_summary_many(h, k, dp, dp, dp, dp),
        "potus_diagnostics": lambda h, k: L.potus_diagnostics(h, k, 0, 1, dp, dp),
        "potus_check_convergence": lambda h, k: L.potus_check_convergence(h, k, 1.01, 400.0, C.byref(n), dp, dp),
        "potus_loo": lambda h, k: L.potus_loo(h, k, 0, None, dp, dp),
        "potus_run_many": lambda h, k: L.potus_run_many(h, k, 5),
    }
    bad = (C.c_int * 1)(12345)
    for name, call in calls.items():
        assert call(None, 1) == 1 and "null" in _err(L), (name, _err(L))
        assert call(bad, 1) == 4 and "bad handle 12345" in _err(L), (name, _err(L))
