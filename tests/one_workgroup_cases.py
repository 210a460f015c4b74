"""Designs for the one-workgroup model pass (csrc/potus_model.hpp, model_pass) at the edges of its layout, and the schedule build_model (potus_hmc.hip)
derives from a poll calendar, restated here from its description (test infrastructure for test_gpu_one_workgroup_edges.py and
test_one_workgroup_edges_host.py).

The calendar is forced as in test_gpu_cluster_builds.py (its `design`): synthetic.make for the outcomes and the priors, then the days, the states
and -- through `pollsters` -- the pollster of every poll overwritten.  Every design states the structure it is there for as literals (`expect`) and
`assert_preconditions` holds them against `structure`, which reads nothing but the design's own arrays:

  * the parameter order of make_layout: raw_mu_b_T [S] | raw_mu_b [S x T] | raw_mu_c [P] | full: raw_mu_m [M] | raw_mu_pop [Pop] | mu_e | rho | raw_e_bias [T] |
    national noise | state noise | raw_polling_bias [S]; nmid = what lies between the S x T block and the noise = P (+ M + Pop + 2 + T);
  * the level-2 segments, in this order: pollsters (kind 0) | full: modes, populations (kind 0) | states and the national pseudo-state (kind 1) |
    full: days (kind 2); thread `tid` finishes segment `tid`, the segments from PT_THREADS = 512 on are finished by the loop at the end of phase E;
  * every segment's list of polls is cut into level-1 tasks of PT_SUBLEN = 16;
  * the AR(1) scans give every lane per = ceil(T / 64) days, so ceil(T / per) lanes hold days;
  * the gather schedule: polled days, longest first (ties: earliest first), each onto the least-loaded wave (load = polls + 2 per day; ties: lowest wave)
    among those with fewer than 64 days and room for the day's polls within 256; no such wave: refused.

Designs whose parameters differ from a plain reading of their name:
  * `many_days_few_pollsters`: with S = 6 its states' segments (kind 1) sit at 261 .. 267, so the loop beyond 512 sees days (kind 2) only, one of them (day 245)
    without polls; kind 1 beyond 512 is what `many_pollsters_short` (states at 520 / 526 ..) and `capacity` are there for, kind 0 beyond 512 too.
  * `capacity`: only the odd-numbered pollsters hold polls (300 of 600, 513 .. 599 among them), the even-numbered hold none.
  * `lds_S63_T256` is a refusal: S x (T | 1) + (S + 1) x (S | 1) + 2 x 8 x (S + 1) doubles, the first three buffers of the layout, are 169 976 bytes > 160 KiB."""
import functools

import numpy as np

from test_gpu_cluster_builds import FULL, NOMODE, design

THREADS, WAVES, WAVE_DAYS, WAVE_POLLS, SUBLEN, LANES, DAYS_PER_WAVE, LDS_LIMIT = 512, 8, 64, 256, 16, 64, 32, 160 * 1024


# ------------------------------------------------------------------------------------------------------------ build_model's rules, restated
def gather_waves(per_day):
    """[(polls, days)] of the eight waves, or None where a day finds no wave."""
    polls, days = [0] * WAVES, [0] * WAVES
    for t in sorted((t for t in range(len(per_day)) if per_day[t]), key=lambda t: -per_day[t]):      # sorted() is stable: ties keep the day order
        room = [w for w in range(WAVES) if days[w] < WAVE_DAYS and polls[w] + per_day[t] <= WAVE_POLLS]
        if not room:
            return None
        w = min(room, key=lambda w: polls[w] + 2 * days[w])                                             # min() keeps the first of equals
        polls[w] += int(per_day[t]); days[w] += 1
    return list(zip(polls, days))


def structure(data, variant):
    full = variant == FULL
    S, T, P = int(data["S"]), int(data["T"]), int(data["P"])
    M, Pop = (int(data["M"]), int(data["Pop"])) if full else (0, 0)
    Nn = len(data["day_national"])
    cat = lambda a, b: np.concatenate([np.asarray(data[a]), np.asarray(data[b])]).astype(int) - 1
    day, pollster = cat("day_state", "day_national"), cat("poll_state", "poll_national")
    state = np.concatenate([np.asarray(data["state"]).astype(int) - 1, np.full(Nn, S)])
    groups = [(0, np.bincount(pollster, minlength=P))]
    if full:
        groups += [(0, np.bincount(cat("poll_mode_state", "poll_mode_national"), minlength=M)), (0, np.bincount(cat("poll_pop_state", "poll_pop_national"), minlength=Pop))]
    groups.append((1, np.bincount(state, minlength=S + 1)))
    if full:
        groups.append((2, np.bincount(day, minlength=T)))
    kinds = [k for k, l in groups for _ in l]
    per = -(-T // LANES)
    return dict(nmid=P + (M + Pop + 2 + T if full else 0), nseg=len(kinds), per=per, lanes=-(-T // per), polls=len(day),
                tasks=sum(int((-(-l // SUBLEN)).sum()) for _, l in groups), beyond=sorted(set(kinds[THREADS:])),
                waves=gather_waves(np.bincount(day, minlength=T)), pollster_lists=groups[0][1], per_day=np.bincount(day, minlength=T),
                lds_at_least=8 * (S * (T | 1) + (S + 1) * (S | 1) + 2 * WAVES * (S + 1)))


def assert_preconditions(dz):
    """What the design says about its own arrays, before the library sees them."""
    st = structure(dz["data"], dz["variant"])
    for key in ("nmid", "nseg", "per", "lanes", "polls", "tasks", "beyond", "waves"):
        assert st[key] == dz[key], (key, st[key], dz[key])
    for p, n in dz.get("lists", {}).items():
        assert st["pollster_lists"][p - 1] == n, (p, st["pollster_lists"][p - 1], n)
    if "days_of" in dz:
        for n, count in dz["days_of"].items():
            assert int((st["per_day"] == n).sum()) == count, (n, st["per_day"])
    if "lds_more_than" in dz:
        assert st["lds_at_least"] > dz["lds_more_than"] >= LDS_LIMIT
    else:
        assert st["lds_at_least"] < LDS_LIMIT // 2
    return st


# ------------------------------------------------------------------------------------------------------------ designs
def _odd_pollsters(ns, nn):                      # capacity: 1, 3, .., 599 in turn; the even-numbered hold no poll
    p = [1 + 2 * (i % 300) for i in range(ns + nn)]
    return p[:ns], p[ns:]


def _in_turn(P):
    def f(ns, nn):
        p = [1 + i % P for i in range(ns + nn)]
        return p[:ns], p[ns:]
    return f


def _lists_of(counts):                            # pollster k + 1 holds exactly counts[k] polls, the lists interleaved
    def f(ns, nn):
        p = np.repeat(np.arange(1, len(counts) + 1), counts)
        assert len(p) == ns + nn
        p = np.random.default_rng(5).permutation(p)
        return p[:ns], p[ns:]
    return f


CAP_BIG = (20, 52, 84, 116, 148, 180, 212)                                                # seven days of 214 state + 42 national polls
CAP_SMALL = (1, 255, 256) + tuple(t for t in range(2, 255, 4))[:61]                       # 64 days of 3 + 1
CAP_65TH = 254


def _capacity(more=()):
    return lambda t: (214, 42) if t in CAP_BIG else (3, 1) if t in CAP_SMALL or t in more else (0, 0)


def _sparse(T):
    return lambda t: (4, 2) if t in (1, T - 1, T) or t % 9 == 0 else (0, 0)


def _one_day(day, pn):
    return lambda t: pn if t == day else (3, 1)


# name: the design's arguments with, in `expect`, the structure it is there for
DESIGNS = {}


def _add(name, expect, variants=(FULL,), S=6, **kw):
    for v in variants:
        DESIGNS[name + ("" if v == FULL else "/nomode")] = functools.partial(design, S=S, K=1, variant=v, expect=expect[v], **kw)


_add("capacity", variants=(FULL, NOMODE), T=256, P=600, per_day=_capacity(), pollsters=_odd_pollsters, expect={
    FULL: dict(nmid=864, nseg=869, per=4, lanes=64, polls=2048, tasks=867, beyond=[0, 1, 2], waves=[(256, 1)] * 7 + [(256, 64)], days_of={256: 7, 4: 64, 0: 185},
               lists={1: 7, 2: 0, 513: 6, 514: 0, 599: 6, 600: 0}),
    NOMODE: dict(nmid=600, nseg=607, per=4, lanes=64, polls=2048, tasks=431, beyond=[0, 1], waves=[(256, 1)] * 7 + [(256, 64)], days_of={256: 7, 4: 64, 0: 185},
                 lists={1: 7, 2: 0, 513: 6, 514: 0, 599: 6, 600: 0})})
_add("many_pollsters_short", variants=(FULL, NOMODE), T=40, P=520, per_day=(12, 3), pollsters=_in_turn(520), expect={
    FULL: dict(nmid=568, nseg=573, per=1, lanes=40, polls=600, tasks=676, beyond=[0, 1, 2], waves=[(75, 5)] * 8, lists={1: 2, 80: 2, 81: 1, 520: 1}),
    NOMODE: dict(nmid=520, nseg=527, per=1, lanes=40, polls=600, tasks=558, beyond=[0, 1], waves=[(75, 5)] * 8, lists={1: 2, 80: 2, 81: 1, 520: 1})})
_add("many_days_few_pollsters", T=250, P=255, per_day=lambda t: (0, 0) if t % 7 == 0 else (2, 1), pollsters=_in_turn(255), expect={
    FULL: dict(nmid=513, nseg=518, per=4, lanes=63, polls=645, tasks=595, beyond=[2], waves=[(81, 27)] * 7 + [(78, 26)], days_of={3: 215, 0: 35})})
for _T, _per, _lanes, _polls, _tasks, _waves in ((64, 1, 64, 54, 30, [(12, 2)] + [(6, 1)] * 7), (65, 2, 33, 60, 34, [(12, 2)] * 2 + [(6, 1)] * 6),
                                                (129, 3, 43, 102, 53, [(18, 3)] + [(12, 2)] * 7), (193, 4, 49, 144, 68, [(18, 3)] * 8)):
    _add(f"T{_T}", T=_T, per_day=_sparse(_T), expect={FULL: dict(nmid=13 + _T, nseg=18 + _T, per=_per, lanes=_lanes, polls=_polls, tasks=_tasks, beyond=[], waves=_waves,
                                                                 days_of={6: _polls // 6, 0: _T - _polls // 6})})
for _T, _per, _lanes, _tasks, _waves in ((32, 1, 32, 71, [(16, 4)] * 8), (33, 1, 33, 76, [(20, 5)] + [(16, 4)] * 7), (225, 4, 57, 457, [(116, 29)] + [(112, 28)] * 7)):
    _add(f"T{_T}", T=_T, per_day=(3, 1), expect={FULL: dict(nmid=13 + _T, nseg=18 + _T, per=_per, lanes=_lanes, polls=4 * _T, tasks=_tasks, beyond=[], waves=_waves, days_of={4: _T})})
for _n, _pn, _tasks, _waves in ((8, (6, 2), 89, [(24, 5)] + [(20, 5)] * 7), (9, (7, 2), 90, [(25, 5)] + [(20, 5)] * 7), (256, (214, 42), 167, [(256, 1)] + [(24, 6)] * 4 + [(20, 5)] * 3)):
    _add(f"day_of_{_n}", T=40, per_day=_one_day(17, _pn), expect={FULL: dict(nmid=53, nseg=58, per=1, lanes=40, polls=39 * 4 + _n, tasks=_tasks, beyond=[], waves=_waves,
                                                                             days_of={_n: 1, 4: 39})})
_add("one_pollster_2048", T=128, P=1, per_day=(13, 3), expect={
    FULL: dict(nmid=1 + 8 + 128, nseg=1 + 6 + 7 + 128, per=2, lanes=64, polls=2048, tasks=644, beyond=[], waves=[(256, 16)] * 8, lists={1: 2048})})
_add("pollster_lists_0_1_16_17", T=40, P=6, per_day=lambda t: (2, 1) if t <= 33 else (0, 0), pollsters=_lists_of([0, 1, 16, 17, 32, 33]), expect={
    FULL: dict(nmid=6 + 8 + 40, nseg=6 + 6 + 7 + 40, per=1, lanes=40, polls=99, tasks=66, beyond=[], waves=[(15, 5)] + [(12, 4)] * 7, lists={1: 0, 2: 1, 3: 16, 4: 17, 5: 32, 6: 33})})
for _S, _tasks in ((8, 107), (9, 107), (16, 108), (17, 109)):
    _add(f"S{_S}", S=_S, T=40, per_day=(5, 1), expect={FULL: dict(nmid=53, nseg=52 + _S, per=1, lanes=40, polls=240, tasks=_tasks, beyond=[], waves=[(30, 5)] * 8)})

# what one workgroup per chain must refuse (`refusal`: the text of build_model's message); a cluster runs every one of them
REFUSED = {
    "T257": functools.partial(design, S=6, T=257, K=1, variant=FULL, per_day=(3, 1), expect=dict(
        refusal="T = 257: one workgroup per chain handles T <= 256 days", nmid=270, nseg=275, per=5, lanes=52, polls=1028, tasks=523, beyond=[], waves=[(132, 33)] + [(128, 32)] * 7)),
    "day_of_257": functools.partial(design, S=6, T=40, K=1, variant=FULL, per_day=_one_day(17, (215, 42)), expect=dict(
        refusal="poll schedule of one workgroup per chain does not fit: more than 2048 polls or 512 polled days", nmid=53, nseg=58, per=1, lanes=40, polls=39 * 4 + 257,
        tasks=170, beyond=[], waves=None, days_of={257: 1, 4: 39})),
    "capacity_and_a_65th_day": functools.partial(design, S=6, T=256, K=1, variant=FULL, P=600, per_day=_capacity((CAP_65TH,)), pollsters=_odd_pollsters, expect=dict(
        refusal="poll schedule of one workgroup per chain does not fit: more than 2048 polls or 512 polled days", nmid=864, nseg=869, per=4, lanes=64, polls=2052,
        tasks=867, beyond=[0, 1, 2], waves=None, days_of={256: 7, 4: 65, 0: 184})),
    "lds_S63_T256": functools.partial(design, S=63, T=256, K=1, variant=FULL, per_day=lambda t: (3, 1) if t % 4 == 0 else (0, 0), expect=dict(
        refusal=r"one workgroup per chain needs \d+ bytes of LDS \(> 160 KiB\): T=256, polls=256", nmid=269, nseg=5 + 6 + 64 + 256, per=4, lanes=64, polls=256,
        tasks=132, beyond=[], waves=[(32, 8)] * 8, lds_more_than=169000)),
}
ALL = {**DESIGNS, **REFUSED}
ROWS = 12


# ------------------------------------------------------------------------------------------------------------ the oracle's side
def points(D, seed):
    """The three points of test_gpu_cluster_builds: zeros, uniform(-2, 2), 0.2 x normal."""
    rng = np.random.default_rng(seed)
    return np.vstack([np.zeros((1, D)), rng.uniform(-2, 2, (1, D)), 0.2 * rng.standard_normal((1, D))])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The design, its three points with the oracle's log density and gradient (the literal form), and -- for the designs that one workgroup runs -- the
    oracle's first ROWS warm-up transitions of two chains.  Computed once per design, shared by the tests, never written to."""
    from oracle_lib import OracleModel
    dz = ALL[name]()
    m = OracleModel(dz["data"], dz["variant"])
    q = points(m.D, dz["seed"])
    lpg = [m.log_prob_grad(qi) for qi in q]
    rows = []
    if name in DESIGNS:
        o = m.default_opts(num_warmup=ROWS, num_samples=0, save_warmup=1, seed=dz["seed"], fast_grad=1)
        rows = [m.sample_chain(c + 1, o)[0] for c in (0, 1)]
    for a in (q, *rows, *(g for _, g in lpg)):
        a.setflags(write=False)
    return dz, q, lpg, rows


def assert_real_trees(name, rows):
    """On the oracle's rows alone: a non-divergent transition of depth >= 5 in each chain."""
    for c, ref in enumerate(rows):
        assert ((ref[:, 3] >= 5) & (ref[:, 5] == 0)).any(), (name, c, ref[:, 3:6])
