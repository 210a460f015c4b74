"""The adjoint gather of the cluster pass (phase D of cl_pass_partial, potus_cluster.hpp) at the edges of its chunks and groups.

A member's polls (day order) are cut into eight equal chunks, one per wave: chunk w is [np w / 8, np (w + 1) / 8).  A wave walks its chunk
in groups -- sixteen polls in the dynamic builds (tags 4 / 8; eight before the walk was shortened), in trips of 64; the fixed builds (tags
16 / 17, at most 32 polls per chunk) unroll it as 16 + 8 + 8 at constant lanes.  Behind every poll the running sum is stored: to the poll's
day where the poll is the last of its day, else to a dump column.  What can go wrong sits at the group, chunk and trip boundaries and at
the day ends next to them, so the designs here FORCE the calendar as tests/test_gpu_cluster_builds.py does (its `design`,
`assert_preconditions` and `open_handle` are reused): every design states its partition (days and polls of every member) as a literal, asserts
it on its own arrays, and gets that module's check 2: log density to 1e-11 relative and gradient to 1e-10 of its max-norm against the fp64
oracle at zeros, uniform(-2, 2) and 0.2 x normal.  No transitions: a case is a fraction of a second.

The polls per chunk follow from the literal: a member of 8 c polls has eight chunks of c.  Every design has polls on day T.
tests/test_gather_walk_designs.py checks on the CPU that every design meets its preconditions and that the oracle alone is finite on it."""
import functools

import numpy as np
import pytest

from oracle_lib import OracleModel
from test_gpu_cluster_builds import ALL, FULL, GRAD_RTOL, LP_RTOL, NOMODE, SEED, _blocks, assert_preconditions, design, open_handle
from us_potus_model_amd import Handle

pytestmark = pytest.mark.gpu

WALK = {}


def _uniform(c, days_per_member, K, **kw):
    """K members of `days_per_member` days with 8 c polls each: eight chunks of c polls in every member."""
    per_day, rem = divmod(8 * c, days_per_member)
    assert rem == 0
    n = max(1, per_day // 7)
    return functools.partial(design, T=K * days_per_member, K=K, per_day=(per_day - n, n), **kw)


# dynamic builds (tag 4: S != 51), K = 4: chunks of 1, 7, 8, 9, 15, 16, 17 and 24 polls -- both sides of a group of eight and of sixteen
for _i, (_c, _d) in enumerate(((1, 2), (7, 2), (8, 4), (9, 2), (15, 4), (16, 2), (17, 4), (24, 2))):
    WALK[f"chunk/{_c}_polls"] = _uniform(_c, _d, 4, S=3 + _i % 4, variant=(FULL, NOMODE)[_i % 2],
                                          expect=dict(tag=4, days=[_d] * 4, polls=[8 * _c] * 4))
# four polls per member: chunks 0, 1, 0, 1, 0, 1, 0, 1 -- waves with an empty chunk
WALK["chunk/empty_chunks"] = functools.partial(design, S=4, T=8, K=4, variant=FULL, per_day=(1, 1), expect=dict(tag=4, days=[2] * 4, polls=[4] * 4))
# 100 polls on each of the last two days and none before: the first two members have 15 days and no poll, the other two a single day that carries
# all of their polls and straddles all eight chunks (12 or 13 polls each)
WALK["days/no_polls_and_one_day_with_all"] = functools.partial(design, S=5, T=32, K=4, variant=FULL, per_day=lambda t: (84, 16) if t > 30 else (0, 0),
                                                               expect=dict(tag=4, days=[15, 15, 1, 1], polls=[0, 0, 100, 100]))
# chunks of 24; the first chunk of every member is days of 8, 1, 7, 1 and 7 polls: a day ends on slot 7 and the next on slot 8 (groups of eight),
# one on slot 15 and the next on slot 16 (groups of sixteen), one on the chunk's last slot; three days of 56 polls straddle the other chunks
_EDGE = ((7, 1), (1, 0), (6, 1), (1, 0), (6, 1), (48, 8), (48, 8), (48, 8))
WALK["days/ends_at_group_edges"] = functools.partial(design, S=6, T=32, K=4, variant=NOMODE, per_day=lambda t: _EDGE[(t - 1) % 8],
                                                     expect=dict(tag=4, days=[8] * 4, polls=[192] * 4))
# tag 8 with 640 polls per member (that module's capacity design): chunks of 80 polls, a second trip of 64
WALK["chunk/second_trip_tag8"] = ALL["tag8/T256"]

# fixed builds (S = 51; tag 16 full, 17 no_mode_adjustment), K = 2 members of 8 days: chunks of 16, 17, 24, 25 and 32 polls -- both sides of the
# second and the third unrolled group, and ClFixed::NPCAP = 256 polls per member
for _c, _v in ((16, FULL), (17, NOMODE), (24, FULL), (25, FULL), (32, FULL)):
    WALK[f"fixed/{_c}_polls"] = _uniform(_c, 8, 2, S=51, variant=_v, expect=dict(tag=17 if _v == NOMODE else 16, days=[8, 8], polls=[8 * _c] * 2))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The design, the three points and the oracle's log density and gradient at them: computed once per design, never written to."""
    dz = WALK[name]()
    m = OracleModel(dz["data"], dz["variant"])
    rng = np.random.default_rng(SEED)
    q = np.vstack([np.zeros((1, m.D)), rng.uniform(-2, 2, (1, m.D)), 0.2 * rng.standard_normal((1, m.D))])
    lpg = [m.log_prob_grad(qi) for qi in q]
    for a in (q, *(g for _, g in lpg)):
        a.setflags(write=False)
    return dz, q, lpg


@pytest.mark.parametrize("name", list(WALK))
def test_log_density_and_gradient_at_the_edges_of_the_walk(name, monkeypatch):
    dz, q, lpg = reference(name)
    assert_preconditions(dz)
    monkeypatch.setenv("POTUS_CL_MFMA", "0")            # the walk, however dense the calendar
    h = open_handle(dz)
    try:
        assert h.L.potus_debug_build_tag(h.h) == dz["tag"]
        lp, grad = h.log_prob_grad(q)
    finally:
        h.close()
    for i, (lpo, go) in enumerate(lpg):
        scale = np.abs(go).max()
        err = np.abs(grad[i] - go)
        per_block = {k: float(err[a:b].max() / scale) for k, (a, b) in _blocks(dz["data"], dz["variant"]).items() if b > a}
        print(f"{name} point {i}: lp rel err {abs(lp[i] - lpo) / abs(lpo):.2e}, grad rel err {err.max() / scale:.2e}")
        assert abs(lp[i] - lpo) <= LP_RTOL * abs(lpo), (name, i, lp[i], lpo)
        assert err.max() <= GRAD_RTOL * scale, (name, i, per_block)


@pytest.mark.parametrize("name", ["days/ends_at_group_edges", "fixed/25_polls"])
def test_twin_gives_the_bytes_of_one_cluster_on_the_walk(name, monkeypatch):
    """k_cl_run<4, true> and <16, true> against <., false>: a warm-up of 40 with its metric update and 5 draws, one cluster per chain and two."""
    monkeypatch.setenv("POTUS_CL_MFMA", "0")
    dz = WALK[name]()
    assert_preconditions(dz)
    out = []
    for twin in (0, 1):
        h = Handle(dz["data"], dz["variant"], chains=2, num_warmup=40, num_samples=5, save_warmup=1, seed=99, cus_per_chain=dz["K"], twin=twin)
        assert h.L.potus_debug_build_tag(h.h) == dz["tag"] and h.clusters_per_chain == 1 + twin
        h.init(); h.run(45)
        out.append((h.draws().copy(), h.adaptation()))
        h.close()
    (a, ada), (b, adb) = out
    assert np.isfinite(a).all() and np.array_equal(a, b), np.argwhere(a != b)[:5]
    assert np.array_equal(ada[0], adb[0]) and np.array_equal(ada[1], adb[1])
