"""The exchange fetch (xld, potus_cluster.hpp) issues the loads of a first round back to back, between two scheduling fences, and compares the tags
behind the last load; the re-fetch loop for words that were not there yet is what it was.  Protocol, layout, tags and summation order are unchanged,
so the draws are: the same bytes from every build of the pass and from one cluster or two per chain, and the oracle's chain for the first
transitions.  The shapes are the smallest at which a wrong mask, a wrong offset or a dropped re-fetch shows: a full cluster of sixteen, a cluster
that is not XCD-local (write-through stores: words arrive later, re-fetch rounds happen), and a cluster of four (twelve of the sixteen loads of
a round belong to absent members and go out of range).  A missed word fails the comparison or returns the watchdog error."""
import ctypes as C
import functools
from pathlib import Path

import numpy as np
import pytest

from oracle_lib import OracleModel
from us_potus_model_amd import Handle

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
NW, NS, SEED = 30, 10, 1843
NAMES = ["small_full", "small_nomode"]


@functools.lru_cache(maxsize=None)
def _oracle_chain(name):
    """Chain 1 of the oracle for the run the tests here make (computed once per posterior, never modified); 12 + 4 transitions of the 2016 posterior."""
    from us_potus_model_amd import dataprep, synthetic
    variant = "no_mode_adjustment" if name == "small_nomode" else "full"
    data = dataprep.load_npz(GOLD / "data_2016.npz")["data"] if name == "2016" else synthetic.small(variant)
    m = OracleModel(data, variant)
    o = m.default_opts(num_warmup=12 if name == "2016" else NW, num_samples=4 if name == "2016" else NS, seed=SEED, fast_grad=1, save_warmup=1)
    ref = m.sample_chain(1, o)[0]
    ref.setflags(write=False)
    return ref


def _draws(cases, name, chains, cus, twin, expect_tag=None, nw=NW, ns=NS):
    data, variant = cases[name]
    h = Handle(data, variant, chains=chains, num_warmup=nw, num_samples=ns, seed=SEED, save_warmup=1, cus_per_chain=cus, twin=twin)
    assert h.cus_per_chain == cus and h.clusters_per_chain == 1 + twin
    if expect_tag is not None:
        assert h.L.potus_debug_build_tag(h.h) == expect_tag
    h.init()
    h.run(nw + ns)
    d = h.draws().copy()
    L = h.L
    L.potus_debug_xcd_local.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.potus_debug_xcd_local.restype = C.c_int
    loc = (C.c_int * 64)()
    n = L.potus_debug_xcd_local(h.h, loc)
    h.close()
    assert d.shape[:2] == (chains, nw + ns) and np.isfinite(d).all()
    return d, [int(loc[i]) for i in range(max(n, 0))]


def _follows_the_oracle(d, name, k=6):
    ref = _oracle_chain(name)
    assert np.array_equal(d[0, :k, 3:6], ref[:k, 3:6]), (d[0, :k, :7], ref[:k, :7])   # tree depth, n_leapfrog, divergent
    assert np.allclose(d[0, :k, 0], ref[:k, 0], rtol=1e-7), (d[0, :k, 0], ref[:k, 0])


@pytest.mark.parametrize("name", NAMES)
def test_sixteen_members_twin_one_cluster_and_dynamic_build_give_the_same_bytes(cases, name, monkeypatch):
    twin, _ = _draws(cases, name, 2, 16, 1)
    one, _ = _draws(cases, name, 2, 16, 0)
    monkeypatch.setenv("POTUS_CL_DYNAMIC", "1")
    dyn, _ = _draws(cases, name, 2, 16, 0, expect_tag=4)
    dyn_twin, _ = _draws(cases, name, 2, 16, 1, expect_tag=4)
    monkeypatch.delenv("POTUS_CL_DYNAMIC")
    assert np.array_equal(twin, one), np.argwhere(twin != one)[:5]
    assert np.array_equal(one, dyn), np.argwhere(one != dyn)[:5]
    assert np.array_equal(one, dyn_twin), np.argwhere(one != dyn_twin)[:5]
    _follows_the_oracle(twin, name)


@pytest.mark.parametrize("name", NAMES)
def test_clusters_across_xcds_refetch_and_give_the_same_bytes(cases, name):
    """6 chains: neither 12 nor 6 clusters are a multiple of eight, so no cluster is XCD-local and every exchange word is a write-through store."""
    twin, loc2 = _draws(cases, name, 6, 16, 1)
    one, loc1 = _draws(cases, name, 6, 16, 0)
    assert len(loc2) == 12 and len(loc1) == 6 and not any(loc2) and not any(loc1), (loc2, loc1)
    assert np.array_equal(twin, one), np.argwhere(twin != one)[:5]
    _follows_the_oracle(twin, name)


@pytest.mark.parametrize("name", NAMES)
def test_four_members_leave_twelve_loads_of_a_round_out_of_range(cases, name, monkeypatch):
    twin, _ = _draws(cases, name, 2, 4, 1)
    one, _ = _draws(cases, name, 2, 4, 0)
    monkeypatch.setenv("POTUS_CL_DYNAMIC", "1")
    dyn, _ = _draws(cases, name, 2, 4, 0, expect_tag=4)
    monkeypatch.delenv("POTUS_CL_DYNAMIC")
    assert np.array_equal(twin, one), np.argwhere(twin != one)[:5]
    assert np.array_equal(one, dyn), np.argwhere(one != dyn)[:5]
    _follows_the_oracle(twin, name)


def test_fixed_layout_build_of_sixteen_across_xcds_and_inside_one(cases, monkeypatch):
    """The 2016 posterior takes the fixed-layout build (tag 16), whose rounds the compiler had interleaved with their compares.  12 + 4 transitions: 6 chains (no cluster XCD-local, re-fetch rounds) and 2 chains, twin against one cluster against the dynamic build."""
    kw = dict(nw=12, ns=4)
    far_twin, loc = _draws(cases, "2016", 6, 16, 1, expect_tag=16, **kw)
    far_one, _ = _draws(cases, "2016", 6, 16, 0, expect_tag=16, **kw)
    near_twin, _ = _draws(cases, "2016", 2, 16, 1, expect_tag=16, **kw)
    monkeypatch.setenv("POTUS_CL_DYNAMIC", "1")
    dyn, _ = _draws(cases, "2016", 2, 16, 0, expect_tag=4, **kw)
    monkeypatch.delenv("POTUS_CL_DYNAMIC")
    assert len(loc) == 12 and not any(loc), loc
    assert np.array_equal(far_twin, far_one), np.argwhere(far_twin != far_one)[:5]
    assert np.array_equal(far_twin[:2], near_twin), np.argwhere(far_twin[:2] != near_twin)[:5]   # a chain's stream depends on its number only
    assert np.array_equal(near_twin, dyn), np.argwhere(near_twin != dyn)[:5]
    _follows_the_oracle(far_twin, "2016")
