"""The per-poll binomial-logit term on the MI355X over its whole domain: exp underflowing, log1p(ex) == ex, pr exactly 0 or 1, y = 0, y = n,
n = 0, n |eta| of order 1e9.  The term is written out in five places (potus_model.hpp phase C, potus_cluster.hpp phase C, loo_poll_ll,
binomial_logit_draw, d_inv_logit); each is held here to a plain high-precision reference:

  loo_poll_ll            potus_poll_ll_probe against 40-digit quadrature (tests/golden/poll_terms.npz), 1e-9 max(1, |ref|)
  the model passes       Handle.log_prob_grad on the tail designs against 60-digit values, 16 e_orc of A_lp / A_i (poll_terms_ref.py), on one
                         workgroup and on clusters of 4 / 8 / 16 (dynamic build, matrix-core adjoint), and on 2016 / 2012 with the same edge counts
                         against the oracle block by block (fixed-layout builds, twin or not)
  rho_e_bias, inv_logit  far out, against the oracle and scipy
  binomial_logit_draw    potus_binomial_draw_probe, chi-square against scipy.stats.binom.pmf cell by cell (both branches, the branch switch)

A variant of this arithmetic (docs/HISTORY.md knob table) has this file to pass."""
import ctypes as C

import numpy as np
import pytest
from scipy import special, stats

import poll_terms_ref as ptr
from conftest import GOLD
from oracle_lib import OracleModel
from us_potus_model_amd import Handle, _abi, dataprep, sampler

pytestmark = pytest.mark.gpu

LL_TOL = 1e-9                       # |device - ref| <= LL_TOL max(1, |ref|): the bar of test_gpu_loo.py; the 16-node form itself is within 6.4e-15 (numpy, host test)
LP_RTOL, GRAD_RTOL = 1e-11, 1e-10   # against the oracle (test_gpu_parity.py)
DRAWS = 60_000


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def poll_ll(y, n, eta, sigma, z, integrate):
    L = sampler.load_library()
    L.potus_poll_ll_probe.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    a = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), np.shape(eta))) for v in (y, n, eta, sigma, z)]
    out = np.full(len(a[0]), np.nan)
    assert L.potus_poll_ll_probe(0, len(out), *[_vp(v) for v in a], int(integrate), _vp(out)) == 0
    return out


def binomial_draws(seed, n, eta, draws):
    L = sampler.load_library()
    L.potus_binomial_draw_probe.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    n, eta = np.ascontiguousarray(n, dtype=np.int32), np.ascontiguousarray(eta, dtype=np.float64)
    out = np.full((len(n), draws), -1, np.int32)
    assert L.potus_binomial_draw_probe(0, seed, len(n), _vp(n), _vp(eta), draws, _vp(out)) == 0
    return out


def _within(got, ref, what):
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    k = int(np.nanargmax(np.where(np.isfinite(err), err, np.inf)))
    print(f"{what}: worst |device - ref| / max(1, |ref|) = {err[k]:.3e} at cell {k} (device {got[k]!r}, ref {ref[k]!r})")
    assert np.isfinite(got).all(), (what, np.flatnonzero(~np.isfinite(got))[:10])
    bad = np.flatnonzero(err > LL_TOL)
    assert bad.size == 0, (what, [(int(i), float(got[i]), float(ref[i])) for i in bad[:12]], bad.size)


# ------------------------------------------------------------------------------------------------ loo_poll_ll
def test_plain_log_likelihood_over_the_grid_and_the_tails():
    F = ptr.fixture()
    for k, z in enumerate(F["ll_z"]):
        _within(poll_ll(F["ll_y"], F["ll_n"], F["ll_eta"], F["ll_sigma"], z, 0), F["ll_plain"][:, k], f"plain, z = {z}")
    for sigma, z in ((0.04, 0.0), (0.0, 2.0)):                          # eta itself: +-36 ... +-800
        _within(poll_ll(F["tail_y"], F["tail_n"], F["tail_eta"], sigma, z, 0), F["tail_plain"], f"plain tail cells, sigma = {sigma}")
    none = F["ll_n"] == 0
    assert none.sum() == 30 and (poll_ll(0.0, 0.0, F["ll_eta"][none], F["ll_sigma"][none], 2.0, 0) == 0).all()


def test_integrated_log_likelihood_over_the_grid():
    """Every cell of sigma x n x y x mismatch against 40-digit quadrature.  With the eight undamped Newton steps this kernel took until the
    bracketed search, the cells 2.5, 3 and -6 logits off with large sigma^2 n failed this by orders (sigma 0.04, n 100 000, y 50 000, +3:
    -6 123 499 for -72 060)."""
    F = ptr.fixture()
    got = poll_ll(F["ll_y"], F["ll_n"], F["ll_eta"], F["ll_sigma"], 0.7, 1)           # (z is not read)
    _within(got, F["ll_integrated"], "integrated")
    none = F["ll_n"] == 0
    assert np.abs(got[none]).max() <= LL_TOL, got[none]                 # no poll: log of the prior's mass, 0
    flat = F["ll_sigma"] == 0
    plain0 = poll_ll(F["ll_y"], F["ll_n"], F["ll_eta"], F["ll_sigma"], 0.0, 0)
    assert flat.sum() == 144 and got[flat].tobytes() == plain0[flat].tobytes()
    # sigma = 0, integrate = 1 is the plain value at z = 0 on every cell, the tails included, byte for byte
    for y, n, eta in ((F["ll_y"], F["ll_n"], F["ll_eta"]), (F["tail_y"], F["tail_n"], F["tail_eta"])):
        assert poll_ll(y, n, eta, 0.0, 0.3, 1).tobytes() == poll_ll(y, n, eta, 0.0, 0.0, 0).tobytes()
    _within(poll_ll(F["tail_y"], F["tail_n"], F["tail_eta"], 0.0, 0.0, 1), F["tail_plain"], "integrated tail cells, sigma = 0")


# ------------------------------------------------------------------------------------------------ the model passes
@pytest.fixture(scope="module")
def designs():
    out = {name: ptr.design(name) for name in ptr.design_names()}
    for d in out.values():
        for a in d[2:]:
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("cus", [1, 4, 8, 16])
@pytest.mark.parametrize("name", ["s6_full", "s6_nomode", "s1_full", "s1_nomode"])
def test_model_pass_on_the_tail_designs(designs, name, cus, monkeypatch):
    data, variant, q, lp_ref, g_ref, A_lp, A = designs[name]
    builds = [({}, 0 if cus == 1 else 4)]
    if cus > 1:
        builds.append(({"POTUS_CL_DYNAMIC": "1"}, 4))
        if name.startswith("s6"):
            builds.append(({"POTUS_CL_MFMA": "1"}, 12))
    tol_lp, tol_g = ptr.DEVICE_FACTOR * ptr.E_ORC_LP, ptr.DEVICE_FACTOR * ptr.E_ORC_GRAD
    for env, tag in builds:
        for k in ("POTUS_CL_DYNAMIC", "POTUS_CL_MFMA"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        h = Handle(data, variant, chains=1, cus_per_chain=cus)
        assert h.L.potus_debug_build_tag(h.h) == tag, (env, h.L.potus_debug_build_tag(h.h))
        lp, g = h.log_prob_grad(q)
        lp2, g2 = h.log_prob_grad(q)
        h.close()
        worst = [0.0, 0.0]
        for i in range(len(q)):
            a, b = ptr.scaled_errors(lp[i], g[i], lp_ref[i], g_ref[i], A_lp[i], A[i])
            worst = [max(worst[0], a), max(worst[1], b)]
        print(f"{name} K={cus} {env}: lp {worst[0]:.2e} of A_lp (allowed {tol_lp:.2e}), gradient {worst[1]:.2e} of A_i (allowed {tol_g:.2e})")
        for i in range(len(q)):
            assert abs(lp[i] - lp_ref[i]) <= tol_lp * A_lp[i], (env, i, lp[i], lp_ref[i])
            bad = np.flatnonzero(np.abs(g[i] - g_ref[i]) > tol_g * A[i])
            assert bad.size == 0, (env, i, [(int(j), float(g[i, j]), float(g_ref[i, j]), float(A[i, j])) for j in bad[:8]])
        assert lp.tobytes() == lp2.tobytes() and g.tobytes() == g2.tobytes(), env


EDGE_51 = {"2016": ("full", 16), "2012": ("no_mode_adjustment", 17)}


@pytest.fixture(scope="module")
def edge_51():
    """2016 / 2012 with sigma_measure_noise_* = 25, twenty polls edited to the edge counts (their days kept), six points with the tail designs'
    cycle on the noise coordinates, and the oracle's values: pinned to the 60-digit ones on the small designs by test_poll_terms_host.py."""
    g, out = ptr.gen(), {}
    for year, (variant, tag) in EDGE_51.items():
        data = dict(dataprep.load_npz(GOLD / f"data_{year}.npz")["data"])
        data["sigma_measure_noise_state"] = data["sigma_measure_noise_national"] = g.NOISE_SIGMA
        for kind in ("state", "national"):
            n, y = (np.array(data[f"{k}_{kind}"]) for k in ("n_two_share", "n_democrat"))
            g.edit_counts(g.EDIT_COUNTS, n, y, np.array(data[f"day_{kind}"]), int(data["T"]))
            data[f"n_two_share_{kind}"], data[f"n_democrat_{kind}"] = n, y
        q = g.tail_points(data, variant)
        m = OracleModel(data, variant)
        ref = [m.log_prob_grad(qi) for qi in q]
        assert all(np.isfinite(lp) and np.isfinite(gr).all() for lp, gr in ref)
        q.setflags(write=False)
        out[year] = (data, variant, tag, q, ref)
    return out


@pytest.mark.parametrize("twin", [0, 1])
@pytest.mark.parametrize("cus", [1, 16])
@pytest.mark.parametrize("year", list(EDGE_51))
def test_edge_counts_and_tails_at_51_states(edge_51, year, cus, twin, monkeypatch):
    for k in ("POTUS_CL_DYNAMIC", "POTUS_CL_MFMA"):
        monkeypatch.delenv(k, raising=False)
    data, variant, tag, q, ref = edge_51[year]
    h = Handle(data, variant, chains=1, cus_per_chain=cus, twin=twin)
    assert h.L.potus_debug_build_tag(h.h) == (tag if cus == 16 else 0) and h.clusters_per_chain == 1 + twin
    lp, g = h.log_prob_grad(q)
    h.close()
    layout, _ = _abi.column_layout(data, variant)
    blocks = {k: (a - 7, b - 7) for k, (a, b, _) in layout.items() if b - 7 <= q.shape[1]}
    worst = ("", 0.0)
    for i, (lpo, go) in enumerate(ref):
        assert abs(lp[i] - lpo) <= LP_RTOL * abs(lpo), (i, lp[i], lpo)
        err = np.abs(g[i] - go)
        assert err.max() <= GRAD_RTOL * np.abs(go).max(), i
        for k, (a, b) in blocks.items():
            own = np.abs(go[a:b]).max()
            worst = max(worst, (k, float(err[a:b].max() / own)), key=lambda t: t[1])
            assert err[a:b].max() <= GRAD_RTOL * own, (i, k, float(err[a:b].max()), float(own))
    print(f"{year} K={cus} twin={twin}: worst block on its own scale {worst}")


# ------------------------------------------------------------------------------------------------ rho_e_bias and inv_logit far out
@pytest.mark.parametrize("cus", [1, 8])
def test_rho_e_bias_far_out(cases, cus):
    """lp has log(rho) + log1p(-rho) for the Jacobian of rho = inv_logit(x) in the device passes and in the oracle alike: it cancels as x
    grows and is -inf once rho rounds to 1 (x >= 37) or to 0 (x <= -746), where Stan's log_inv_logit(x) + log_inv_logit(-x) is finite
    (a known deviation; the formula is not changed here)."""
    data, variant = cases["small_full"]
    h = Handle(data, variant, chains=1, cus_per_chain=cus)
    m = OracleModel(data, variant)
    col = h.layout["rho_e_bias"][0] - _abi.N_SAMPLER_COLS
    base = np.random.default_rng(8).uniform(-2, 2, h.D)
    xs = [10.0, -10.0, 20.0, -20.0, 30.0, -30.0, 36.0, 37.0, -746.0]
    q = np.tile(base, (len(xs), 1))
    q[:, col] = xs
    lp, g = h.log_prob_grad(q)
    for i, x in enumerate(xs):
        lpo, go = m.log_prob_grad(q[i])
        if x in (37.0, -746.0):
            assert not np.isfinite(lpo) and not np.isfinite(lp[i]), (x, lp[i], lpo)
        else:
            assert abs(lp[i] - lpo) <= LP_RTOL * abs(lpo), (x, lp[i], lpo)
            assert np.abs(g[i] - go).max() <= GRAD_RTOL * np.abs(go).max(), x
    h.close()


def test_predicted_score_and_logit_pi_at_the_tail_points(designs):
    """potus_constrain on the tail points: logit_pi (|eta| up to 800) against the oracle's row, and predicted_score = inv_logit(mu_b) against
    scipy.special.expit of the row's own mu_b, with raw_mu_b_T chosen so that mu_b itself runs from -800 to 800: within 2 ulp (of the
    subnormals too), and exactly 0 or 1 only where the double is."""
    data, variant, q, *_ = designs["s6_full"]
    S, T = int(data["S"]), int(data["T"])
    h = Handle(data, variant, chains=1, cus_per_chain=1)
    m = OracleModel(data, variant)
    q = np.array(q)
    want_T = np.array([[0, 40, -40, 300, -300, 800], [-800, 746, -746, 745.2, -745.2, 744], [-744, 710, -710, 709, -709, 708],
                       [-708, 700, -700, 37.5, -37.5, 36.5], [20, -20, 17, -17, 100, -100], [1, -1, 0.5, -0.5, 1e-3, -1e-3]])
    L_T = m.cholesky()[1]
    q[:, :S] = np.linalg.solve(L_T, (want_T - np.asarray(data["mu_b_prior"])).T).T      # mu_b[:, T] = L_T raw_mu_b_T + mu_b_prior = want_T
    row = h.constrain(q)
    lay = {k: (a - _abi.N_SAMPLER_COLS, b - _abi.N_SAMPLER_COLS) for k, (a, b, _) in h.layout.items()}
    for i in range(len(q)):
        want = m.write_array(q[i])
        for k in ("logit_pi_democrat_state", "logit_pi_democrat_national", "mu_b"):
            a, b = lay[k]
            assert np.all(np.abs(row[i, a:b] - want[a:b]) <= 1e-12 * np.maximum(1.0, np.abs(want[a:b]))), (i, k)
    a, b = lay["mu_b"]
    mu_b = row[:, a:b].reshape(len(q), T, S)                             # column-major S x T
    a, b = lay["predicted_score"]
    ps = row[:, a:b].reshape(len(q), S, T).transpose(0, 2, 1)            # column-major T x S
    # (scipy's expit returns 0 below log(DBL_MIN) = -708.4 where the value is a subnormal double; there 1 + exp(x) == 1 and expit(x) is exp(x) to 1e-308)
    ref = np.where(mu_b < -708.0, np.exp(np.minimum(mu_b, 0.0)), special.expit(mu_b))
    assert np.abs(mu_b).max() > 746 and (ref == 0).any() and (ref == 1).any() and ((ref > 0) & (ref < 1e-300)).any()
    assert (ref[ps == 0] == 0).all() and (ref[ps == 1] == 1).all()
    ulp = np.abs(ps - ref) / np.spacing(ref)
    print(f"predicted_score: mu_b in [{mu_b.min():.1f}, {mu_b.max():.1f}], largest |device - expit| = {ulp.max():.2f} ulp")
    assert ulp.max() <= 2.0
    h.close()


# ------------------------------------------------------------------------------------------------ binomial_logit_draw
INVERSION = [(1, 0.0), (1, -3.0), (7, .3), (19, -.1), (21, .1), (1000, -4.6), (1_000_000, -11.6)]
BTRS = [(20, 0.0), (1000, -4.55), (4118, 2.5), (61771, .02), (61771, -8.0), (1_000_000, -11.4)]
SATURATED = [(300, 40.0), (300, -40.0)]


@pytest.fixture(scope="module")
def cell_draws():
    cells = INVERSION + BTRS + SATURATED
    d = binomial_draws(20201103, [c[0] for c in cells], [c[1] for c in cells], DRAWS)
    d.setflags(write=False)
    return dict(zip(cells, d))


def test_the_cells_take_the_branch_they_are_named_for():
    for cells, inversion in ((INVERSION, True), (BTRS, False)):
        for n, eta in cells:
            e = np.exp(-abs(eta))
            assert (n * (e / (1.0 + e)) < 10.0) == inversion, (n, eta)


@pytest.mark.parametrize("cell", INVERSION + BTRS, ids=lambda c: f"n{c[0]}_eta{c[1]}")
def test_binomial_draws_follow_the_pmf(cell_draws, cell):
    """Chi-square of 60 000 draws of one (n, eta) against scipy.stats.binom.pmf, bins merged to an expectation of at least 10 over the
    1e-9 ... 1 - 1e-9 quantile range (what lies outside goes to the end bins).  The seed is fixed: p >= 1e-4 is deterministic."""
    n, eta = cell
    x = cell_draws[cell]
    assert x.min() >= 0 and x.max() <= n
    p = special.expit(eta)
    lo, hi = int(stats.binom.ppf(1e-9, n, p)), int(stats.binom.ppf(1 - 1e-9, n, p))
    ks = np.arange(lo, hi + 1)
    expect = DRAWS * stats.binom.pmf(ks, n, p)
    expect[0] += DRAWS * stats.binom.cdf(lo - 1, n, p)
    expect[-1] += DRAWS * stats.binom.sf(hi, n, p)
    obs = np.bincount(np.clip(x, lo, hi) - lo, minlength=len(ks)).astype(float)
    E, O, e, o = [], [], 0.0, 0.0
    for a, b in zip(expect, obs):
        e, o = e + a, o + b
        if e >= 10.0:
            E.append(e); O.append(o)
            e = o = 0.0
    if E:
        E[-1] += e; O[-1] += o                                           # the rest joins the last bin
    else:
        E, O = [e], [o]
    E, O = np.array(E), np.array(O)
    assert len(E) >= 2 and abs(E.sum() - DRAWS) < 1e-6 * DRAWS and O.sum() == DRAWS
    chi2 = float(((O - E) ** 2 / E).sum())
    pv = float(stats.chi2.sf(chi2, len(E) - 1))
    print(f"binomial({n}, inv_logit({eta})): mean {x.mean():.4f} (n p = {n * p:.4f}), {len(E)} bins, chi2 = {chi2:.1f}, p = {pv:.4f}")
    assert pv >= 1e-4


def test_saturated_cells_give_all_or_nothing(cell_draws):
    assert (cell_draws[(300, 40.0)] == 300).all() and (cell_draws[(300, -40.0)] == 0).all()
