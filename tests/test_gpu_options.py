"""Sampler options, user inits and init retries on every device path, against the CPU oracle.

The rest of the GPU suite runs the sampler at potus_default_opts() from the library's own first-attempt random point.  Here every sampler
form the library has is driven through what users change first (`inits`, `init`, `adapt_delta`, `stepsize`, the warm-up length):

  (a) user inits                 potus_init(handle, q0): k_init, k_cl_init (scatter through the cluster permutation), k_init_ds, dense import
  (b) inits the model rejects    POTUS_ERR_INIT for a point of density -inf (with a finite or a non-finite gradient) or with a NaN
  (c) retries                    chains of one handle that need 0, 1 and 2 retries of stan::services::util::initialize
  (d) the first step-size search doubling, halving, a search that stops at once, the early return for a step size beyond 1e7
  (e) dual averaging and windows delta / gamma / kappa / t0 / stepsize / window sizes away from the defaults; rescaled and absent windows
  (f) options the library must refuse, before it touches the device

Everything is compared with the oracle (tests/oracle_lib.py); "same bytes as" is said where a run is compared with an already verified path.

PATHS below names the Handle arguments of every sampler form; `_open` confirms through potus_debug_build_tag / cus_per_chain / clusters_per_chain
that the intended kernel ran.  The internal vector length of a cluster layout (parameters + padding elements) cannot be read through the ABI, so the
scatter of q0 through the permutation is exercised on four different layouts (small_full and small_nomode on clusters of 8, 2016 and 2012 on the
fixed-layout clusters of 16), with q0 rows without a zero so that a value landing in a padding slot or a parameter left out changes the density.

POTUS_ERR_STEPSIZE is returned by no test: the search leaves (0, 1e7) only where the energy error stays large at every step size, which no point
of finite density of these posteriors gives (Stan's own comment there: the posterior is improper).  What can be reached of that code is the early
return (d, stepsize = 2e7).

Conditioning of every compared trajectory, established on the oracle alone: its literal and its fast gradient form over the compared rows give
identical tree columns, and the figure below is the largest |difference| / max(1, |value|) over all other columns.  A case is kept only below 1e-8, a
factor 100 under the 1e-6 the device is held to; none had to be dropped.  (b) otherwise compares row 0 of (a) again.  For (e) the compared
rows are single transitions from given states: measured on the oracle's own chain of the option set (chains 1 and 2), the literal form replaying the
rows of the fast form's chain before its first window end and after its last.

  case                                                        chains  rows   diagonal   dense (unit metric)
  (a) small_full, q0 = zeros / U(-2,2) / 0.2 N(0,1) / U(-2,2)  1-4     0-7    3.6e-11    3.6e-11
  (a) small_nomode, the same                                  1-3     0-7    1.2e-10    1.2e-10
  (a) small_full, four chains over two of make_datasets' sets  1-4     0-7    1.3e-10
  (a) 2016, the same                                          1-3     0-1    1.3e-13
  (a) 2012, the same                                          1-3     0-1    1.6e-14
  (a) small_full, inits through PotusModel.sample, seed 5     1-5     0-5    6.0e-13
  (b) small_full, chain c on make_datasets' set c              1-3     0      5.9e-15
  (c) small_full, seed 7119, radius 40                        1-3     0-7    1.2e-14    1.2e-14
  (c) the same, chain c on make_datasets' set c               1-3     0-7    6.9e-15
  (c) 2016, seed 153, radius 40                               1-3     0-1    2.2e-14
  (d) small_full, stepsize 1e-4                               1-2     0-2    1.1e-13    1.1e-13
  (d) small_full, stepsize 1                                  1-2     0-2    7.4e-15    7.4e-15
  (d) small_full, stepsize 0.1                                1-2     0-2    6.4e-15    6.4e-15
  (d) small_full, stepsize 2e7                                1-2     0-2    0          0            (no row moves)
  (d) 2016, stepsize 1e-4                                     1-2     0-1    7.8e-16
  (e) small_full "da" (dense: max_depth 5)                    1-2            7.5e-13    1.5e-11
  (e) small_full "windows" (dense: max_depth 5)               1-2            3.2e-12    2.8e-12
  (e) small_full "nw60"                                       1-2            7.0e-13    4.1e-11
  (e) small_full "nw25"                                       1-2            4.7e-12    3.9e-11
  (e) small_full "nw19"                                       1-2            4.5e-13    4.5e-13
  (e) small_full "nw0", 2016 "nw0"                            1-2            0          0            (no row moves)
  (e) 2016 "nw60"                                             1-2            7.4e-11
  (e) 2016 "nw19"                                             1-2            1.6e-10
  (f) small_full, init radius 0, windows 0 | 30 | 0           1-2     0-2    4.7e-15

Wall time on an MI355X: 34 s for the 141 cases.
"""
import ctypes as C

import numpy as np
import pytest

from adaptation_replay import adaptation_replayed_from_the_device_rows, initial_point, rows_around, run_through_the_windows, window_schedule
from oracle_lib import OracleModel
from us_potus_model_amd import Handle, PotusModel, _abi, sampler

pytestmark = pytest.mark.gpu

DENSE = _abi.METRIC_DENSE
ERR_ARG, ERR_INIT = 1, 3

# every sampler form: its Handle arguments and the build tag it must run (None: not pinned).  The one-workgroup path comes first in every
# parametrisation: a disagreement between the members of a cluster would end in the library's watchdog error.
PATHS = {
    "wg1": (dict(cus_per_chain=1, twin=0), 0),
    "wg1_twin": (dict(cus_per_chain=1, twin=1), 0),
    "cl8": (dict(cus_per_chain=8, twin=0), (4, 8)),
    "cl8_twin": (dict(cus_per_chain=8, twin=1), (4, 8)),
    "cl16": (dict(cus_per_chain=16, twin=0), {"2016": (16,), "2012": (17,)}),
    "cl16_twin": (dict(cus_per_chain=16, twin=1), {"2016": (16,), "2012": (17,)}),
    "dense_wg1": (dict(metric=DENSE, cus_per_chain=1), None),
    "dense_cl8": (dict(metric=DENSE, cus_per_chain=8), None),
    "pooled": (dict(metric=DENSE, pooled_metric=1, cus_per_chain=1), None),
    "datasets": (dict(cus_per_chain=1, twin=0), 0),
}
SMALL_PATHS = ["wg1", "wg1_twin", "cl8", "cl8_twin", "dense_wg1", "dense_cl8", "pooled", "datasets"]
BIG = [("wg1", "2016"), ("cl16_twin", "2016")]              # what runs once more at the size of the reference's posterior


def _open(cases, design, path, datasets=None, **opts):
    """(handle, [oracle model of chain c]) of a sampler form; asserts that the form asked for is the one that runs."""
    data, variant = cases[design]
    kw, tag = PATHS[path]
    h = Handle(data, variant, **kw, **opts)
    assert h.cus_per_chain == kw["cus_per_chain"] and h.clusters_per_chain == (2 if kw.get("twin") == 1 else 1), (path, h.cus_per_chain, h.clusters_per_chain)
    if tag is not None:
        want = tag[design] if isinstance(tag, dict) else tag
        got = h.L.potus_debug_build_tag(h.h)
        assert got in (want if isinstance(want, tuple) else (want,)), (path, design, got)
    if path != "datasets":
        return h, [_model(cases, design)] * h.opts.chains
    ys, yn = datasets                                         # one data set per chains / n consecutive chains
    n = len(ys)
    h.set_datasets(ys, yn)
    per = h.opts.chains // n
    return h, [_model(cases, design, ys[c // per], yn[c // per]) for c in range(h.opts.chains)]


_MODELS = {}


def _model(cases, design, ys=None, yn=None):
    key = (design, None if ys is None else ys.tobytes() + yn.tobytes())
    if key not in _MODELS:
        data, variant = cases[design]
        _MODELS[key] = OracleModel(data if ys is None else dict(data, n_democrat_state=ys, n_democrat_national=yn), variant)
    return _MODELS[key]


def make_datasets(data, n, seed=77):
    """n sets of poll outcomes for a design: every poll's Democratic count drawn again, binomial around its observed share shifted by N(0, 0.03)."""
    rng = np.random.default_rng(seed)
    out = []
    for kind in ("state", "national"):
        dem, two = np.asarray(data[f"n_democrat_{kind}"]), np.asarray(data[f"n_two_share_{kind}"])
        p = np.clip(dem / two + 0.03 * rng.standard_normal((n, len(two))), 0.05, 0.95)
        out.append(rng.binomial(two, p).astype(np.int32))
    return out[0], out[1]


@pytest.fixture(scope="module")
def datasets(cases):
    """Four sets of poll outcomes for small_full (potus_set_datasets: k_init_ds / k_run_ds)."""
    return make_datasets(cases["small_full"][0], 4)


def _oracle_opts(m, h, **kw):
    o = h.opts
    return m.default_opts(num_warmup=o.num_warmup, num_samples=o.num_samples, save_warmup=o.save_warmup, seed=int(o.seed), max_depth=o.max_depth,
                          init_buffer=o.init_buffer, term_buffer=o.term_buffer, window=o.window, delta=o.delta, gamma=o.gamma, kappa=o.kappa, t0=o.t0,
                          stepsize=o.stepsize, init_radius=o.init_radius, dense_metric=1 if o.metric == DENSE else 0, fast_grad=1, **kw)


_CHAINS = {}


def _oracle_chain(m, h, chain_id, q0=None):
    """The oracle's chain under the handle's options (computed once for all the paths that share it; nobody writes to it)."""
    o = _oracle_opts(m, h)
    key = (id(m), chain_id, bytes(o), None if q0 is None else np.asarray(q0).tobytes())
    if key not in _CHAINS:
        _CHAINS[key] = m.sample_chain(chain_id, o, q0=q0)[0]
        _CHAINS[key].setflags(write=False)
    return _CHAINS[key]


def _unit_metric(h):
    return (np.eye(h.D), np.eye(h.D)) if h.opts.metric == DENSE else (np.ones(h.D), None)


def _same_rows(got, ref, what):
    """The comparison of the existing oracle tests: the tree exactly, the first step size exactly, values to rtol 1e-6 / atol 1e-7."""
    assert np.array_equal(got[:, 3:6], ref[:, 3:6]), (what, got[:, :7], ref[:, :7])          # treedepth__, n_leapfrog__, divergent__
    assert got[0, 2] == ref[0, 2], (what, got[0, 2], ref[0, 2])
    assert np.allclose(got[:, [0, 1, 2, 6]], ref[:, [0, 1, 2, 6]], rtol=1e-6, atol=1e-7), (what, got[:, :7], ref[:, :7])
    assert np.allclose(got[:, 7:], ref[:, 7:], rtol=1e-6, atol=1e-7), (what, np.abs(got[:, 7:] - ref[:, 7:]).max())


def _starts_from(h, m, chain, q_init, row, what):
    """Row 0 of a chain is the oracle's transition from q_init under the unit metric, and its step size the first search's from q_init."""
    o = _oracle_opts(m, h)
    cid = h.opts.chain_id_offset + chain + 1
    minv, chol = _unit_metric(h)
    eps0 = m.init_stepsize_from(cid, o, 0xFFFFFFFF, q_init, h.opts.stepsize, minv, chol)
    if h.opts.num_warmup > 0:
        assert row[2] == eps0, (what, row[2], eps0)
    _same_rows(row[None], m.transitions_from(cid, o, 0, q_init, row[2], minv, chol), what)
    return eps0


def user_inits(n, D, seed=20240):
    """One point per chain: all zeros, U(-2,2), 0.2 N(0,1), U(-2,2), ... (no zero in the random rows)."""
    rng = np.random.default_rng(seed)
    rows = [np.zeros(D) if c % 4 == 0 else 0.2 * rng.standard_normal(D) if c % 4 == 2 else rng.uniform(-2, 2, D) for c in range(n)]
    return np.array(rows)


def _sizes(design):
    """(warm-up length, transitions compared): a few on the small designs, two at the reference's sizes"""
    return (10, 8) if design.startswith("small") else (2, 2)


# ------------------------------------------------------------------------------------------------ (a) user inits
USER_INIT_CASES = ([(p, d) for d in ("small_full", "small_nomode") for p in SMALL_PATHS if not (p == "datasets" and d != "small_full")] +
                   [("wg1", "2016"), ("cl16", "2016"), ("cl16_twin", "2016"), ("cl16", "2012"), ("cl16_twin", "2012")])


@pytest.mark.parametrize("path,design", USER_INIT_CASES)
def test_user_inits_start_every_path_where_they_say(cases, datasets, path, design):
    """potus_init(handle, q0): every chain starts from ITS row of q0 -- the first transitions are the oracle's sample_chain(q0 = that row), and
    row 0 is the oracle's single transition from exactly that point (its step size the first search's from that point)."""
    nw, iters = _sizes(design)
    chains = 4 if path == "datasets" else 3
    h, models = _open(cases, design, path, datasets=(datasets[0][:2], datasets[1][:2]), chains=chains, num_warmup=nw, num_samples=0, save_warmup=1, seed=1843)
    q0 = user_inits(chains, h.D)
    h.init(q0)
    h.run(iters)
    d = h.draws()[:, :iters]
    for c in range(chains):
        m = models[c]
        _same_rows(d[c], _oracle_chain(m, h, c + 1, q0[c])[:iters], (path, design, c))
        _starts_from(h, m, c, q0[c], d[c, 0], (path, design, c, "row 0"))
    h.close()


def test_inits_through_the_model_surface_reach_the_right_chains(cases):
    """PotusModel.sample(inits=...): each device's handle gets the rows of ITS chains (inits[off:off + n_loc]).  Five chains over two handles
    (the second on device 1 where there is one) give the same bytes as one handle with all five, and chain 4 -- the first of the second block
    -- is the oracle's chain from row 3 of inits."""
    from conftest import second_device
    data, variant = cases["small_full"]
    kw = dict(seed=5, chains=5, iter_warmup=30, iter_sampling=6, refresh=10, save_warmup=True, cus_per_chain=1, twin=0)
    q0 = user_inits(5, _abi.num_params(data, variant), seed=9)
    one = PotusModel(variant).sample(data, inits=q0, **kw)
    two = PotusModel(variant).sample(data, inits=q0, devices=[0, second_device()], **kw)
    assert len(two._hs) == 2 and [h.opts.chains for h in two._hs] == [3, 2]
    assert one.unconstrained().tobytes() == two.unconstrained().tobytes()
    assert one._write_array(0, 7).tobytes() == two._write_array(0, 7).tobytes()
    m = _model(cases, "small_full")
    o = m.default_opts(num_warmup=30, num_samples=6, save_warmup=1, seed=5, fast_grad=1)
    rows = np.concatenate([h.draws() for h in two._hs])
    for c in (2, 3, 4):                                                     # last of the first block, both of the second
        _same_rows(rows[c][:6], m.sample_chain(c + 1, o, q0=q0[c])[0][:6], c)
    for f in (one, two):
        for h in f._hs:
            h.close()


# ------------------------------------------------------------------------------------------------ (b) inits the model rejects
def _rho_index(cases, design):
    data, variant = cases[design]
    layout, _ = _abi.column_layout(data, variant)
    return layout["rho_e_bias"][0] - _abi.N_SAMPLER_COLS


# (value of the unconstrained rho_e_bias coordinate or of coordinate 3, chains it is put into): 40 -> rho = 1, density -inf and a non-finite
# gradient; -746 -> rho = 0, density -inf with a finite gradient; NaN anywhere
REJECTED = [("rho", 40.0, (0, 1, 2)), ("rho", 40.0, (1,)), ("rho", -746.0, (2,)), ("other", float("nan"), (0,))]


@pytest.mark.parametrize("path,design", [(p, "small_full") for p in SMALL_PATHS] + BIG + [("cl16", "2016")])
def test_rejected_inits_are_answered_by_a_status(cases, datasets, path, design):
    """Stan's "Rejecting initial value": potus_init answers a user point without a finite density and gradient with POTUS_ERR_INIT and a
    message -- all chains bad, one of three, the density -inf with a finite gradient, a NaN -- exactly where the oracle refuses the same
    point; the handle can be destroyed and a fresh one on the same device inits and runs.  With several data sets in a handle a chain
    without a start is reported by potus_chain_status and the others go on (the declared behaviour of potus_set_datasets)."""
    i_rho = _rho_index(cases, design)
    kw = dict(chains=3, num_warmup=1, num_samples=0, save_warmup=1, seed=1843)
    ds = (datasets[0][:3], datasets[1][:3])
    for where, value, bad in REJECTED:
        h, models = _open(cases, design, path, datasets=ds, **kw)
        q0 = user_inits(3, h.D)                                             # three points the model accepts
        for c in bad:
            q0[c, i_rho if where == "rho" else 3] = value
        for c in range(3):                                                  # the oracle's verdict on every point
            if c in bad:
                with pytest.raises(RuntimeError, match="rc=3"):
                    models[c].sample_chain(c + 1, _oracle_opts(models[c], h), q0=q0[c])
            else:
                models[c].sample_chain(c + 1, _oracle_opts(models[c], h), q0=q0[c])
        if path == "datasets":
            h.init(q0)
            assert h.chain_status()[0] == [ERR_INIT if c in bad else 0 for c in range(3)], (value, bad)
        else:
            rc = h.L.potus_init(h.h, q0.ctypes.data_as(C.POINTER(C.c_double)))
            buf = C.create_string_buffer(512)
            h.L.potus_last_error(buf, 512)
            assert rc == ERR_INIT and f"chain {bad[0] + 1}: the initial point handed in" in buf.value.decode(), (value, bad, rc, buf.value)
        hid = h.h
        h.close()
        g, models = _open(cases, design, path, datasets=ds, **kw)
        assert g.h == hid
        q0 = user_inits(3, g.D)
        g.init(q0)
        g.run(1)
        for c in range(3):
            _starts_from(g, models[c], c, q0[c], g.draws()[c, 0], (path, value, c))
        g.close()


# ------------------------------------------------------------------------------------------------ (c) retries
# design: (seed, init radius, {chain id: retries its first accepted point needed}) -- found on the CPU: with radius 40 an attempt fails exactly
# when the draw of the rho_e_bias coordinate exceeds 36.74 (rho rounds to 1); these are the first seeds whose chains 1-3 need 0, 1 and 2 retries
RETRY = {"small_full": (7119, 40.0, {1: 1, 2: 2, 3: 0}), "2016": (153, 40.0, {1: 0, 2: 2, 3: 1})}


@pytest.mark.parametrize("path,design", [(p, "small_full") for p in SMALL_PATHS] + BIG)
def test_chains_of_one_handle_retry_their_inits_different_numbers_of_times(cases, datasets, path, design):
    """CmdStan's "up to 100 attempts": the three chains of the handle need 0, 1 and 2 retries, so the workgroups of different chains loop different
    numbers of times (and on clusters every member, on both clusters in twin mode, must reach the same verdict each time).  The chain is the
    oracle's; the point of attempt k -- k written out above -- is what its first transition started from, and every earlier attempt is a point
    the oracle refuses."""
    seed, radius, retries = RETRY[design]
    nw, iters = _sizes(design)
    h, models = _open(cases, design, path, datasets=(datasets[0][:3], datasets[1][:3]), chains=3, num_warmup=nw, num_samples=0, save_warmup=1, seed=seed,
                      init_radius=radius)
    h.init()
    h.run(iters)
    d = h.draws()[:, :iters]
    for c in range(3):
        m, k = models[c], retries[c + 1]
        for attempt in range(k + 1):
            lp, g = m.log_prob_grad(initial_point(m, seed, c + 1, radius, attempt))
            assert (np.isfinite(lp) and np.isfinite(g).all()) == (attempt == k), (c, attempt, lp)
        _same_rows(d[c], _oracle_chain(m, h, c + 1)[:iters], (path, design, c))
        _starts_from(h, m, c, initial_point(m, seed, c + 1, radius, k), d[c, 0], (path, design, c, "attempt", k))
    h.close()


def test_no_start_in_100_attempts_is_err_init(cases):
    """init_radius = 1e6 puts rho_e_bias beyond 36.74 or below -745 in all but 4e-4 of the attempts: neither the oracle nor the library finds a
    start in 100 (seed 1843, chains 1 and 2: checked on the oracle here), and the library says POTUS_ERR_INIT."""
    m = _model(cases, "small_full")
    for path in ("wg1", "cl8_twin"):
        h, _ = _open(cases, "small_full", path, chains=2, num_warmup=1, num_samples=0, seed=1843, init_radius=1e6)
        for c in (1, 2):
            with pytest.raises(RuntimeError, match="rc=3"):
                m.sample_chain(c, _oracle_opts(m, h))
        with pytest.raises(sampler.PotusError, match="error 3.*100 attempts"):
            h.init()
        h.close()


# ------------------------------------------------------------------------------------------------ (d) the first step-size search
# stepsize option -> log2(step size found / option) of chains 1 and 2 (seed 1843, from the library's own initial point; CPU run of the oracle):
# eleven doublings, four halvings, one doubling beside a search that stops at once, the early return of init_stepsize
SEARCH = {"small_full": {1e-4: (11, 11), 1.0: (-4, -4), 0.1: (1, 0), 2e7: (0, 0)}, "2016": {1e-4: (8, 8)}}


@pytest.mark.parametrize("path,design,stepsize", [(p, "small_full", s) for s in SEARCH["small_full"] for p in SMALL_PATHS if p != "datasets"] +
                         [(p, d, 1e-4) for p, d in BIG])
def test_first_step_size_search_in_both_directions(cases, path, design, stepsize):
    """base_hmc::init_stepsize before the first transition in its three forms (init_stepsize, cl_init_stepsize, the dense rounds): row 0's
    stepsize__ is the oracle's, which is the option times the power of two written out above; the transitions that follow are the oracle's
    (after 1e-4: from row 1 on trees of depth 10, 1023 leapfrogs each)."""
    iters = 3 if design == "small_full" else 2
    h, models = _open(cases, design, path, chains=2, num_warmup=iters, num_samples=0, save_warmup=1, seed=1843, stepsize=stepsize)
    h.init()
    h.run(iters)
    d = h.draws()[:, :iters]
    m = models[0]
    for c in (0, 1):
        eps0 = _starts_from(h, m, c, initial_point(m, 1843, c + 1, 2.0), d[c, 0], (path, stepsize, c))
        assert eps0 == stepsize * 2.0 ** SEARCH[design][stepsize][c], (c, eps0)
        _same_rows(d[c], _oracle_chain(m, h, c + 1)[:iters], (path, stepsize, c))
        if stepsize == 1e-4:                                                # row 0 diverges at the step size found; learn_stepsize then answers with 2.3e-4
            assert (d[c, 1:, 3] == 10).all() and (d[c, 1:, 4] == 1023).all()
        if stepsize == 2e7:
            assert (d[c, :, 5] == 1).all() and (d[c, :, 4] == 1).all()      # one leapfrog, divergent, the chain stays where it is
    h.close()


# ------------------------------------------------------------------------------------------------ (e) dual averaging and windows
# name: (options, the windows [(first row, last row)] they must give)
OPTION_SETS = {
    "da": (dict(num_warmup=200, delta=0.95, gamma=0.1, kappa=0.6, t0=5.0, stepsize=1e-4), [(75, 99), (100, 149)]),
    "windows": (dict(num_warmup=100, delta=0.6, init_buffer=20, term_buffer=10, window=15), [(20, 34), (35, 89)]),
    "nw60": (dict(num_warmup=60), [(9, 53)]),               # 75 + 25 + 50 > 60: rescaled to 15 % | 75 % | 10 % = 9 | 45 | 6
    "nw25": (dict(num_warmup=25), [(3, 22)]),               # 3 | 20 | 2
    "nw19": (dict(num_warmup=19), []),                      # below 20: no window, the unit metric stays, learn_stepsize only
    "nw0": (dict(num_warmup=0), []),
}


@pytest.mark.parametrize("path,design,name", [(p, "small_full", n) for n in OPTION_SETS for p in ("wg1", "cl8_twin", "dense_wg1", "pooled")] +
                         [(p, d, n) for n in ("nw60", "nw19", "nw0") for p, d in BIG])
def test_adaptation_away_from_the_defaults(cases, path, design, name):
    """Stan's warm-up restated from the device's OWN rows (tests/adaptation_replay.py: every step size from learn_stepsize with the handle's
    delta, gamma, kappa and t0; the metric the device holds after every window end; init_stepsize after it; the oracle's transitions around every
    window end, at the start and in the sampling phase) under options nobody else sets, and under the window schedules of short warm-ups.
    num_warmup = 0 has little power: complete_adaptation leaves the step size exp(x_bar) = exp(0) = 1 whatever the options say, and at that step
    size every row is a one-leapfrog divergent transition that does not move -- from the random start and, on the oracle, from a posterior draw
    alike.  It gets a q0 so that what can be pinned is: step size 1 on every row, lp__ of every row the density at q0 and energy__ the oracle's
    (the momentum draws), the point unchanged."""
    opts, windows = OPTION_SETS[name]
    nw, ns = opts["num_warmup"], 4 if name == "nw0" else 2
    chains = 2
    if name in ("da", "windows") and PATHS[path][0].get("metric") == DENSE:
        # "da" spends 75 iterations near step size 1e-3, "windows" makes its first 292 x 292 metric from 15 draws: both grow trees of up to 1023
        # leapfrogs, which are for (d); the dense forms take 0.8 ms per leapfrog, so here they stop at 31
        opts = dict(opts, max_depth=5)
    h, models = _open(cases, design, path, chains=chains, num_samples=ns, save_warmup=1, seed=1843, **opts)
    m = models[0]
    assert window_schedule(nw, h.opts.init_buffer, h.opts.term_buffer, h.opts.window) == windows
    assert m.window_ends(_oracle_opts(m, h)) == [e for _, e in windows]
    q0 = 0.2 * np.random.default_rng(3).standard_normal((chains, h.D)) if name == "nw0" else None
    h.init(q0)
    held = run_through_the_windows(h, nw + ns)
    assert sorted(held) == [e for _, e in windows]
    rows = ([(0, 2)] if nw else []) + rows_around([e for _, e in windows], 2) + [(nw, ns)]
    eps, diag = h.adaptation()
    for c in range(chains):
        n = adaptation_replayed_from_the_device_rows(*cases[design], h, c, 1843, rows, held, q0=None if q0 is None else q0[c])
        assert n == len(windows)
        if not windows:
            assert np.array_equal(diag[c], np.ones(h.D))
    if name == "nw0":
        d = h.draws()
        assert (d[:, :, 2] == 1.0).all() and (eps == 1.0).all()
        for c in range(chains):
            _same_rows(d[c], _oracle_chain(m, h, c + 1, q0[c]), (path, c))
            assert np.array_equal(d[c, :, 7:], np.tile(q0[c], (ns, 1)))
    h.close()


# ------------------------------------------------------------------------------------------------ (f) options the library must refuse
# CmdStan 2.24's argument bounds: delta in (0, 1); gamma, kappa, t0, stepsize > 0; init radius >= 0; no negative buffer or window; all finite
NAN, INF = float("nan"), float("inf")
REFUSED = ([("delta", v) for v in (0.0, 1.0, -0.2, 1.5, NAN, INF)] +
           [(f, v) for f in ("gamma", "kappa", "t0", "stepsize") for v in (0.0, -1.0, NAN, INF, -INF)] +
           [("init_radius", v) for v in (-1e-9, -2.0, NAN, INF)] +
           [(f, v) for f in ("init_buffer", "term_buffer", "window") for v in (-1, -2 ** 31)])


def _assert_refused(data, variant, field, value):
    """potus_create must answer POTUS_ERR_ARG and name the field.  A handle that does come back is closed, never inited or run."""
    try:
        h = Handle(data, variant, chains=1, num_warmup=10, num_samples=0, **{field: value})
    except sampler.PotusError as e:
        assert f"error {ERR_ARG}:" in str(e) and field in str(e), (field, value, str(e))
        return
    h.close()
    pytest.fail(f"potus_create accepted {field} = {value!r}")


@pytest.mark.parametrize("field,value", REFUSED)
def test_create_refuses_options_outside_cmdstans_bounds(cases, field, value):
    _assert_refused(*cases["small_full"], field, value)


def test_create_still_accepts_the_edges_of_the_bounds(cases):
    """init radius 0 (every chain starts at the origin: the oracle's chain from q0 = 0), empty buffers."""
    data, variant = cases["small_full"]
    h = Handle(data, variant, chains=2, num_warmup=30, num_samples=0, save_warmup=1, init_radius=0.0, init_buffer=0, term_buffer=0, window=30, cus_per_chain=1, twin=0)
    h.init()
    h.run(3)
    m = _model(cases, "small_full")
    for c in (0, 1):
        _same_rows(h.draws()[c, :3], _oracle_chain(m, h, c + 1)[:3], c)
        _starts_from(h, m, c, np.zeros(h.D), h.draws()[c, 0], c)
    h.close()


def test_r_create_refuses_them_too(cases):
    """potus_R_create (R's .C() surface) hands its dopts to potus_create: the same refusals, status by pointer."""
    from test_gpu_boundary import RShim

    class CreateOnly(RShim):
        def call(self, name, *args):
            if name == "potus_R_init":                                      # the library accepted the value: close the handle, never init it
                st = C.c_int(-1)
                super().call("potus_R_destroy", args[0], C.byref(st))
                pytest.fail("potus_R_create accepted the option")
            super().call(name, *args)

    data, variant = cases["small_full"]
    r = CreateOnly()
    for kw, field in ((dict(adapt_delta=1.0), "delta"), (dict(adapt_delta=NAN), "delta"), (dict(init=-1.0), "init_radius")):
        with pytest.raises(RuntimeError, match=f"error {ERR_ARG}: {field}"):
            r.sample(data, variant, seed=1, chains=1, iter_warmup=10, iter_sampling=0, refresh=0, **kw)
