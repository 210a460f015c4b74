"""Every build of the cluster pass (potus_cluster.hpp, tags 4 / 8 / 12 / 16 / 17) at the edges of its partition.

build_cluster (potus_hmc.hip) picks the build from the shape of the data and cuts the days and polls into members, waves, chunks,
level-1 tasks and (state, day) cells -- all of it a function of the poll calendar.  The designs below FORCE the calendar: synthetic.make
for the outcomes and the priors, then day_state / day_national / state overwritten with p state polls (states dealt round-robin) and n
national polls on each listed day.  The outcomes are then not consistent with the calendar; the priors keep the posterior proper.

Every design states the partition it expects (days per member, the build's tag) as a literal and asserts it as a precondition on its OWN
arrays: `partition` restates the cost balance (a day costs 30, a poll 45; contiguous ranges, smallest largest cost, at most 8 waves x 4 or 8
days), nothing is read back from the library but the tag under test.  Every design then gets
  1. potus_debug_build_tag;
  2. log density to 1e-11 relative and gradient to 1e-10 of its max-norm against the fp64 oracle at zeros, uniform(-2, 2), 0.2 x normal;
  3. 12 warm-up transitions of 2 chains against OracleModel.sample_chain: tree depth / leapfrogs / divergence equal, values to 1e-6 / 1e-7
     (a chain that falls out of step with the oracle's on a 13th digit is replayed transition by transition from its own previous row,
     adaptation_replay.py, with the same tolerances);
  4. on the oracle's rows alone: a non-divergent transition of depth >= 5 among the rows compared, for each chain.

Designs whose parameters differ from a plain reading of their name:
  * `kinds/polls_on_the_last_days_T104`: with T = 32 on K = 4 the cost balance gives the eight polled days to three members and the 24 empty days to
    the first one (26 + 2 + 2 + 2: design `kinds/polls_on_days_25_to_32`, kept), so no member is without polls; with T = 104 the 32-day cap
    binds first (32 + 32 + 32 + 8) and three members have days and no polls.
  * `members/K16` has S = 3 and 9 polls per day so that sixteen members of 17 days stay a small model (D = 3 300).
  * the fixed layout at capacity: no other capacity binds before NPCAP with P = 5 (16 days x 16 polls = 256 polls, about 80 level-1 tasks of
    the 384, 1 100 of the 1 920 elements per member), so P stays 5.
  * tag 8 at capacity: T = 256, S = 6 fits the LDS limit (640 polls per member: about 60 KB), so T = 256 is the capacity design and T = 257 is
    the refusal ("T = 257 days do not fit 4 members of at most 64 days").

Wall time of this module on the MI355X: 19 s for its 41 cases, the oracle's share included (the slowest, 64 days per member on tag 8, 2 s)."""
import functools

import numpy as np
import pytest

from adaptation_replay import adaptation_replayed_from_the_device_rows
from oracle_lib import OracleModel
from us_potus_model_amd import Handle, _abi, sampler, synthetic

pytestmark = pytest.mark.gpu

LP_RTOL, GRAD_RTOL = 1e-11, 1e-10
SEED = 3
WAVES, CW_DAY, CW_POLL, DW4_MAXAVG = 8, 30, 45, 26      # waves per member; the cost balance; average days per member up to which a wave takes 4 days


# ------------------------------------------------------------------------------------------------------------ designs
def design(S, T, K, variant, per_day, expect, seed=SEED, P=5, extra=(), pollsters=None):
    """per_day: (p, n) for every day, or a function of the 1-based day; extra: [(day, state, count)] more polls of one state on one day (1-based);
    pollsters: a function of (state polls, national polls) that returns the 1-based poll_state and poll_national to overwrite synthetic.make's with."""
    pn = [per_day(t) if callable(per_day) else per_day for t in range(1, T + 1)]
    day_state = [t for t, (p, _) in enumerate(pn, 1) for _ in range(p)]
    state = [i % S + 1 for p, _ in pn for i in range(p)]
    for t, s, cnt in extra:
        day_state += [t] * cnt
        state += [s] * cnt
    day_national = [t for t, (_, n) in enumerate(pn, 1) for _ in range(n)]
    data = synthetic.make(S=S, T=T, N_state=len(day_state), N_national=len(day_national), P=P, seed=seed, variant=variant)
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    data.update(day_state=i32(day_state), state=i32(state), day_national=i32(day_national))
    if pollsters is not None:
        of_state, of_national = pollsters(len(day_state), len(day_national))
        assert len(of_state) == len(day_state) and len(of_national) == len(day_national)
        data.update(poll_state=i32(of_state), poll_national=i32(of_national))
    return dict(data=data, variant=variant, K=K, seed=seed, **expect)


def partition(data, K):
    """(days per wave, [days of every member]) of the cost balance, or None where the days do not fit: contiguous ranges of at most 8 waves x
    DW days, the smallest bound on a member's cost (30 a day + 45 a poll) that K ranges meet, ranges filled greedily."""
    T = int(data["T"])
    per_day = np.bincount(np.concatenate([data["day_state"], data["day_national"]]).astype(int) - 1, minlength=T)
    dw = 4 if -(-T // K) <= DW4_MAXAVG else 8
    cost = CW_DAY + CW_POLL * per_day

    def ranges(bound):
        out, t = [], 0
        while t < T:
            nd = c = 0
            while t < T and nd < WAVES * dw and (nd == 0 or c + cost[t] <= bound):
                c += cost[t]; nd += 1; t += 1
            out.append(nd)
        return out

    lo, hi = 1, int(cost.sum())
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if len(ranges(mid)) <= K else (mid + 1, hi)
    days = ranges(lo)
    return None if len(days) > K else (dw, days + [0] * (K - len(days)))


def members(data, days):
    """[(polls, polled (state, day) cells, polls of the fullest cell)] of every member; national polls are the pseudo-state S + 1."""
    S = int(data["S"])
    day = np.concatenate([data["day_state"], data["day_national"]]).astype(int)
    st = np.concatenate([np.asarray(data["state"]).astype(int), np.full(len(data["day_national"]), S + 1)])
    out, d0 = [], 0
    for nd in days:
        own = (day > d0) & (day <= d0 + nd)
        cells = np.unique(day[own] * 100 + st[own], return_counts=True)[1]
        out.append((int(own.sum()), len(cells), int(cells.max()) if len(cells) else 0))
        d0 += nd
    return out


def assert_preconditions(dz):
    """What the design says about its own arrays, before the library sees them."""
    data, K = dz["data"], dz["K"]
    T, Np = int(data["T"]), len(data["day_state"]) + len(data["day_national"])
    got = partition(data, K)
    if dz.get("days") is None:
        assert got is None
        return
    dw, days = got
    assert days == dz["days"], (days, dz["days"])
    assert dw == dz.get("dw", 4)
    mem = members(data, days)
    dense = Np > 8 * T
    scatter_ok = all(np_ < 1024 and cells <= 1024 and most <= 63 for np_, cells, most in mem)
    if dz["tag"] == 12:
        assert dw == 4 and dense and scatter_ok, (dw, Np, T, mem)
    for key, col in (("polls", 0), ("cells", 1)):
        if key in dz:
            assert [m[col] for m in mem] == dz[key], (key, mem)
    if "fullest_cell" in dz:
        assert max(m[2] for m in mem) == dz["fullest_cell"], mem
    return mem


FULL, NOMODE = "full", "no_mode_adjustment"
TAG12 = {}


def _add(name, walk_tag, **kw):
    TAG12[name] = functools.partial(design, expect=dict(tag=12, walk_tag=walk_tag, **kw.pop("expect", {})), **kw)


for _v, _vn in ((FULL, "full"), (NOMODE, "nomode")):
    # the day tile of the prefix-with-carry (16 days): members of 1, 15, 16, 17, 26 and 32 days
    for _T, _days in ((2, [1, 1]), (31, [16, 15]), (32, [16, 16]), (34, [17, 17]), (52, [26, 26])):
        _add(f"tiles/T{_T}_{_vn}", 4, S=6, T=_T, K=2, variant=_v, per_day=(8, 2), expect=dict(days=_days))
    # 9 polls on days 1-32 and 40 on days 33-40: the 32-day cap with two full tiles, and a member of 8 days
    _add(f"tiles/T40_cap_{_vn}", 4, S=6, T=40, K=2, variant=_v, per_day=lambda t: (7, 2) if t <= 32 else (32, 8), expect=dict(days=[32, 8], polls=[288, 320]))
# states: wave w < 4 owns the factor columns 16 w ..; GROWS = 4 ceil((S + 1) / 4); the clamps at S + 1 and at the last row of G
for _i, _S in enumerate((1, 3, 4, 15, 16, 17, 48, 51, 63)):
    _v = (FULL, NOMODE)[_i % 2]
    _add(f"states/S{_S}", (17 if _v == NOMODE else 16) if _S == 51 else 4, S=_S, T=34, K=2, variant=_v, per_day=(8, 2), expect=dict(days=[17, 17]))
# kinds of poll
_add("kinds/national_only", 4, S=6, T=32, K=4, variant=FULL, per_day=(0, 10), expect=dict(days=[8, 8, 8, 8]))
_add("kinds/state_only", 4, S=6, T=32, K=4, variant=NOMODE, per_day=(10, 0), expect=dict(days=[8, 8, 8, 8]))
_add("kinds/polls_on_days_25_to_32", 4, S=6, T=32, K=4, variant=FULL, per_day=lambda t: (32, 8) if t > 24 else (0, 0),
     expect=dict(days=[26, 2, 2, 2], polls=[80, 80, 80, 80]))
_add("kinds/polls_on_the_last_days_T104", 4, S=6, T=104, K=4, variant=FULL, per_day=lambda t: (90, 15) if t > 96 else (0, 0),
     expect=dict(days=[32, 32, 32, 8], polls=[0, 0, 0, 840]))
_add("kinds/members_without_days", 4, S=6, T=6, K=8, variant=FULL, per_day=(8, 2), expect=dict(days=[1, 1, 1, 1, 1, 1, 0, 0]))
# cells: the second cell slot of a thread (more than 512 polled cells in a member); a cell of exactly 63 polls
_add("cells/592_cells", 4, S=51, T=32, K=2, variant=NOMODE, per_day=(36, 1), expect=dict(days=[16, 16], polls=[592, 592], cells=[592, 592]))
_add("cells/63_polls_in_one", 16, S=51, T=32, K=2, variant=FULL, per_day=(8, 2), extra=[(20, 40, 63)], expect=dict(days=[19, 13], fullest_cell=63))
# more members
_add("members/K16", 4, S=3, T=272, K=16, variant=NOMODE, per_day=(7, 2), expect=dict(days=[17] * 16))
_add("members/K32", 4, S=6, T=32, K=32, variant=FULL, per_day=(8, 2), expect=dict(days=[1] * 32))

# the fixed layout (tags 16 / 17) at ClFixed::NPCAP = 256 polls per member, and one poll beyond it; the walk is forced (16 polls a day would take tag 12)
FIXED = {}
for _v, _vn, _tag in ((FULL, "full", 16), (NOMODE, "nomode", 17)):
    FIXED[f"fixed/256_polls_{_vn}"] = functools.partial(design, S=51, T=256, K=16, variant=_v, per_day=(13, 3),
                                                        expect=dict(tag=_tag, days=[16] * 16, polls=[256] * 16))
    FIXED[f"fixed/257_polls_{_vn}"] = functools.partial(design, S=51, T=256, K=16, variant=_v, per_day=lambda t: (14, 3) if t == 1 else (13, 3),
                                                        expect=dict(tag=4, days=[16] * 16, polls=[257] + [256] * 15))

# tag 8 at 64 days per member (8 waves x 8 days, every wave full), and one day beyond it
TAG8 = {"tag8/T256": functools.partial(design, S=6, T=256, K=4, variant=FULL, per_day=(8, 2), expect=dict(tag=8, dw=8, days=[64] * 4)),
        "tag8/T257": functools.partial(design, S=6, T=257, K=4, variant=FULL, per_day=(8, 2), expect=dict(tag=None, dw=8, days=None))}

# poll-dense calendars beyond what the adjoint scatter of tag 12 addresses: the walk runs them
BEYOND = {"beyond/70_polls_of_one_state_on_election_eve": functools.partial(design, S=6, T=32, K=2, variant=FULL, per_day=(8, 2), extra=[(32, 3, 69)],
                                                                         expect=dict(tag=4, days=[19, 13], fullest_cell=70, refusal="polls of one state on one day")),
          "beyond/1024_polls_in_a_member": functools.partial(design, S=6, T=32, K=2, variant=NOMODE, per_day=(54, 10),
                                                             expect=dict(tag=4, days=[16, 16], polls=[1024, 1024], refusal="has 1024 polls"))}

ALL = {**TAG12, **FIXED, **TAG8, **BEYOND}


# ------------------------------------------------------------------------------------------------------------ reference and checks
def _blocks(data, variant):
    layout, _ = _abi.column_layout(data, variant)
    D = _abi.num_params(data, variant)
    return {k: (a - 7, b - 7) for k, (a, b, _) in layout.items() if b - 7 <= D}


@functools.lru_cache(maxsize=None)
def reference(name, rows=12):
    """The design, its three points with the oracle's log density and gradient, and the oracle's first `rows` warm-up transitions of two chains
    (computed once per design, shared by the tests, never written to).  Precondition 4 is asserted here, on the oracle's rows alone."""
    dz = ALL[name]()
    data, variant = dz["data"], dz["variant"]
    m = OracleModel(data, variant)
    rng = np.random.default_rng(SEED)
    q = np.vstack([np.zeros((1, m.D)), rng.uniform(-2, 2, (1, m.D)), 0.2 * rng.standard_normal((1, m.D))])
    lpg = [m.log_prob_grad(qi) for qi in q]
    o = m.default_opts(num_warmup=rows, num_samples=0, save_warmup=1, seed=dz["seed"], fast_grad=1)
    chains = [m.sample_chain(c + 1, o)[0] for c in (0, 1)]
    for c, ref in enumerate(chains):
        assert ((ref[:, 3] >= 5) & (ref[:, 5] == 0)).any(), (name, c, ref[:, 3:6])
    for a in (q, *chains, *(g for _, g in lpg)):
        a.setflags(write=False)
    return dz, q, lpg, chains


def check_against_the_oracle(name, h, rows=12):
    """Checks 2 and 3 of the module docstring on an open handle (num_warmup = rows, save_warmup = 1, two chains, the design's seed)."""
    dz, q, lpg, chains = reference(name, rows)
    data, variant = dz["data"], dz["variant"]
    lp, grad = h.log_prob_grad(q)
    for i, (lpo, go) in enumerate(lpg):
        scale = np.abs(go).max()
        err = np.abs(grad[i] - go)
        if err.max() > GRAD_RTOL * scale or abs(lp[i] - lpo) > LP_RTOL * abs(lpo):
            per_block = {k: float(err[a:b].max() / scale) for k, (a, b) in _blocks(data, variant).items() if b > a}
            pytest.fail(f"{name} point {i}: lp {lp[i]!r} vs {lpo!r}; grad rel err by block {per_block}")
    h.init(); h.run(rows)
    d = h.draws()
    assert d.shape[1] == rows
    for c, ref in enumerate(chains):
        if np.array_equal(d[c][:, 3:6], ref[:, 3:6]) and np.allclose(d[c][:, 7:], ref[:, 7:], rtol=1e-6, atol=1e-7):
            continue
        # out of step with the oracle's chain: every transition from the device's own previous row instead (same tolerances; this raises where they differ)
        first = next(i for i in range(rows) if not (np.array_equal(d[c][i, 3:6], ref[i, 3:6]) and np.allclose(d[c][i, 7:], ref[i, 7:], rtol=1e-6, atol=1e-7)))
        print(f"{name} chain {c + 1}: out of step with the oracle's chain at row {first}; replaying every row from the device's previous one")
        adaptation_replayed_from_the_device_rows(data, variant, h, c, dz["seed"], [(0, rows)])
    return d


def open_handle(dz, rows=12, **kw):
    return Handle(dz["data"], dz["variant"], chains=2, num_warmup=rows, num_samples=0, save_warmup=1, seed=dz["seed"], cus_per_chain=dz["K"], **kw)


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", list(TAG12))
def test_matrix_core_build_and_the_walk_on_a_forced_partition(name, monkeypatch):
    """Tag 12 as the library selects it (more than 8 polls per day), then the same design on the walk (POTUS_CL_MFMA = 0: tag 4, or the fixed
    layout where 51 states fit it): both against the oracle, and the tree columns of the two bit for bit."""
    dz = reference(name)[0]
    assert_preconditions(dz)
    trees = []
    for flag, tag in ((None, 12), ("0", dz["walk_tag"])):
        if flag is None:
            monkeypatch.delenv("POTUS_CL_MFMA", raising=False)
        else:
            monkeypatch.setenv("POTUS_CL_MFMA", flag)
        h = open_handle(dz)
        assert h.L.potus_debug_build_tag(h.h) == tag
        trees.append(check_against_the_oracle(name, h)[:, :, 3:6].copy())
        h.close()
    assert np.array_equal(trees[0], trees[1])


@pytest.mark.parametrize("name", list(FIXED))
def test_fixed_layout_at_its_poll_capacity_and_one_poll_beyond(name, monkeypatch):
    """S = 51, T = 256 on 16 members of 16 days x 16 polls = ClFixed::NPCAP: tag 16 (full) / 17 (no_mode_adjustment); one more poll on day 1 and the
    first member holds 257: the dynamic walk (tag 4).  8 transitions (D = 17 523)."""
    dz = reference(name, 8)[0]
    mem = assert_preconditions(dz)
    assert max(m[0] for m in mem) == (256 if dz["tag"] >= 16 else 257)
    monkeypatch.setenv("POTUS_CL_MFMA", "0")
    h = open_handle(dz, rows=8)
    assert h.L.potus_debug_build_tag(h.h) == dz["tag"]
    check_against_the_oracle(name, h, rows=8)
    h.close()


def test_eight_days_per_wave_with_every_wave_full(monkeypatch):
    """Tag 8 at its limit: 256 days on 4 members = 64 days each = 8 waves x 8 days."""
    monkeypatch.delenv("POTUS_CL_MFMA", raising=False)
    dz = reference("tag8/T256")[0]
    assert_preconditions(dz)
    h = open_handle(dz)
    assert h.L.potus_debug_build_tag(h.h) == 8
    check_against_the_oracle("tag8/T256", h)
    h.close()


def test_one_day_beyond_eight_full_waves_is_refused(monkeypatch):
    monkeypatch.delenv("POTUS_CL_MFMA", raising=False)
    dz = TAG8["tag8/T257"]()
    assert_preconditions(dz)
    with pytest.raises(sampler.PotusError, match="T = 257 days do not fit 4 members of at most 64 days"):
        open_handle(dz)


@pytest.mark.parametrize("name", ["tiles/T34_full", "states/S63", "cells/592_cells"])
def test_twin_gives_the_bytes_of_one_cluster_on_the_matrix_core_build(name, monkeypatch):
    """k_cl_run<12, true>: a warm-up of 40 with its metric update and 5 draws, one cluster per chain and two: the same bytes."""
    monkeypatch.delenv("POTUS_CL_MFMA", raising=False)
    dz = ALL[name]()
    assert_preconditions(dz)
    out = []
    for twin in (0, 1):
        h = Handle(dz["data"], dz["variant"], chains=2, num_warmup=40, num_samples=5, save_warmup=1, seed=99, cus_per_chain=dz["K"], twin=twin)
        assert h.L.potus_debug_build_tag(h.h) == 12 and h.clusters_per_chain == 1 + twin
        h.init(); h.run(45)
        out.append((h.draws().copy(), h.adaptation()))
        h.close()
    (a, ada), (b, adb) = out
    assert np.isfinite(a).all() and np.array_equal(a, b), np.argwhere(a != b)[:5]
    assert np.array_equal(ada[0], adb[0]) and np.array_equal(ada[1], adb[1])


@pytest.mark.parametrize("name", list(BEYOND))
def test_poll_dense_calendars_beyond_the_adjoint_scatter_take_the_walk(name, monkeypatch):
    """The choice of tag 12 by poll density is about speed: a member of 1024 polls, or 64 or more polls of one state on one day, is beyond its
    adjoint scatter but not beyond the walk, so the library takes the walk by itself; forced onto the matrix cores it is refused as before."""
    dz = reference(name)[0]
    mem = assert_preconditions(dz)
    data = dz["data"]
    assert len(data["day_state"]) + len(data["day_national"]) > 8 * int(data["T"])
    assert max(m[0] for m in mem) >= 1024 or max(m[2] for m in mem) > 63
    monkeypatch.delenv("POTUS_CL_MFMA", raising=False)
    h = open_handle(dz)
    assert h.L.potus_debug_build_tag(h.h) == dz["tag"]
    check_against_the_oracle(name, h)
    h.close()
    monkeypatch.setenv("POTUS_CL_MFMA", "1")
    with pytest.raises(sampler.PotusError, match="error 6.*" + dz["refusal"]):
        open_handle(dz)
