"""Mean-field ADVI on the MI355X (potus_advi: k_vi_sga, k_vi_elbo, k_vi_draws and Laplace's k_lap_lp) against tests/advi_ref.py (numpy over
the CPU oracle's log_prob_grad, the library's normals restated with the oracle's Philox), against potus_log_prob_grad / potus_constrain of the
same handle, and against stand-alone handles for the data sets of a potus_set_datasets_ex handle.  Designs: synthetic.small of both variants.

Bounds.  e_ref is the reference's own error: the reference run twice, with the oracle's plain and its fast gradient, measured by the test at
every t it compares and printed.  The device is held to 2 x e_ref -- one share for each side of the comparison, DESIGN.md section 4n's
convention -- plus ONE derived term:
  iterates   a step moves a coordinate by (eta / sqrt(t)) g / (1 + sqrt(s)), so a gradient that is off by dg moves it by at most
             (eta / sqrt(t)) |dg| / (1 + sqrt(s)) more; the map is contractive on these designs, so the terms add up and do not grow:
             sum_t (eta / sqrt(t)) max_i |dg_i| / (1 + sqrt(s_i)), with dg what potus_log_prob_grad and the oracle differ by at the
             reference's own zeta_t, measured in the test (no a-priori constant).  For omega the gradient is g o eps o exp(omega) + 1, so its dg
             is that of g times |eps| exp(omega), and s is omega's.
  ELBO       the mean of what potus_log_prob_grad and the oracle differ by at the reference's own zeta_k, measured, plus DEPTH eps sum|omega| for
             the entropy, a sum of D terms whose partial sums pass through DEPTH = ceil(D / 512) + 14 additions on the device (a thread's
             strided share, six DPP steps, eight waves).
  trace      the ELBO's bound plus what the iterates' own difference moves it by, to first order: max over the reference's draws of
             sum_i |g_i| (1 + |eps_i| exp(omega_i)) times the largest difference between the device's and the reference's (mu, omega) at the
             end of the run, measured.
  delta      |(e - p) / e| with e and p off by at most b: (2 + delta) b / |e| to first order.
The whole call: the test first asserts ON THE REFERENCE that the chosen candidate's ELBO is further from its neighbours than 10 x the ELBO's bound
and every buffer mean and median further from tol_rel_obj than 10 x delta's bound; then eta*, the stop, the code and the trace on the device.
The library's stream with seed 1843 has those margins on both variants and both starts (eta* = 1, 0.1 and 1; stop at t = 300, MEAN_CONVERGED),
so the seed is the suite's usual one.  Measured on one MI355X: see DESIGN.md section 4p."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import advi_ref as ref
import outcomes_ref
import timeline_ref
from oracle_lib import OracleModel, lib as oracle_lib
from us_potus_model_amd import _abi, synthetic, timeline
from us_potus_model_amd.outcomes import outcomes_of_block
from us_potus_model_amd.sampler import Handle, PotusError, PotusModel

pytestmark = pytest.mark.gpu
SEED = 1843
OPTS = dict(seed=SEED, cus_per_chain=1, twin=0)
VARIANTS = ("full", "no_mode_adjustment")
EV = np.array([100, 90, 80, 70, 60, 138])
EPS = 2.0 ** -52
M = 37
KEYS = ("mu", "omega", "elbo", "adapt_elbo", "q", "lp", "lq", "return_code", "flags", "iterations", "eta_index", "model_passes", "evaluations")
QUICK = dict(iter=200, eval_elbo=100, elbo_samples=5, adapt_iter=10, output_samples=M)     # the settings of the byte comparisons
TS = (1, 2, 10, 50)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def raw(res, keys=KEYS):
    return b"".join(np.ascontiguousarray(res[k]).tobytes() for k in keys)


def status_of(fn):
    try:
        fn()
    except PotusError as e:
        return int(re.search(r"error (\d+)", str(e)).group(1))
    return 0


@pytest.fixture(scope="module")
def small():
    """Per variant: a plain handle, two starts, the oracle, and ONE quick call from the two starts that the byte comparisons share."""
    out = {}
    for v in VARIANTS:
        data = synthetic.small(v)
        h = Handle(data, v, chains=1, **OPTS)
        q0 = np.random.default_rng(1).uniform(-1, 1, (2, h.D))
        res = h.variational(q0, **QUICK)
        for a in res.values():
            a.setflags(write=False)
        m = OracleModel(data, v)
        out[v] = dict(data=data, h=h, q0=q0, res=res, oracle=m, lpg=lambda q, m=m: m.log_prob_grad(np.ascontiguousarray(q)),
                      lpg_fast=lambda q, m=m: m.log_prob_grad(np.ascontiguousarray(q), fast=True))
    yield out
    for v in VARIANTS:
        out[v]["h"].close()


# ------------------------------------------------------------------------------------------------ 1. the iterates
def _reference_steps(s, r, grad_samples, n):
    """The reference's n steps from start r at eta = 1, with the plain and the fast gradient: snapshots of (mu, omega) per t, and per step the
    points, the step size and the step-size memories the step used."""
    D = s["h"].D
    nm = ref.library_normals(SEED, r)
    snap, fast, steps = {}, {}, []

    def rec(t, zetas, step, s_before, s_mu, mu, om):
        snap[t] = (mu, om)
        steps.append(dict(t=t, zetas=zetas, step=step))
    st = ref.sga(s["lpg"], s["q0"][r], np.zeros(D), 1.0, n, nm, grad_samples=grad_samples, record=rec)
    ref.sga(s["lpg_fast"], s["q0"][r], np.zeros(D), 1.0, n, nm, grad_samples=grad_samples, record=lambda t, z, st_, s0, s1, mu, om: fast.__setitem__(t, (mu, om)))
    assert st["code"] == 0
    return snap, fast, steps, nm


def _derived_terms(s, r, steps, nm, grad_samples):
    """sum_t (eta / sqrt(t)) max_i |dg_i| / (1 + sqrt(s_i)) for mu and for omega, cumulative per t, from the gradient difference measured at the
    reference's own points.  The step-size memories are recomputed here from the oracle's gradients, as the reference computed them."""
    h, D = s["h"], s["h"].D
    pts = np.array([z for st in steps for z in st["zetas"]])
    g_dev = h.log_prob_grad(np.ascontiguousarray(pts))[1]
    g_ora = np.array([s["lpg"](z)[1] for z in pts])
    dg = np.abs(g_dev - g_ora).reshape(len(steps), grad_samples, D)
    g_ora = g_ora.reshape(len(steps), grad_samples, D)
    om, mu = np.zeros(D), np.array(s["q0"][r])
    s_mu = s_om = np.zeros(D)
    cum_mu, cum_om, tm, to = {}, {}, 0.0, 0.0
    for k, st in enumerate(steps):
        t = st["t"]
        eps = np.array([nm(0, m, t, D) for m in range(grad_samples)])
        g_mu, g_om = g_ora[k].mean(0), (g_ora[k] * eps).mean(0) * np.exp(om) + 1.0
        d_mu, d_om = dg[k].mean(0), (dg[k] * np.abs(eps)).mean(0) * np.exp(om)
        mu, s_mu = ref._update(g_mu, st["step"], t, mu, s_mu)
        om_new, s_om = ref._update(g_om, st["step"], t, om, s_om)
        tm += st["step"] * float((d_mu / (1.0 + np.sqrt(s_mu))).max())
        to += st["step"] * float((d_om / (1.0 + np.sqrt(s_om))).max())
        om = om_new
        cum_mu[t], cum_om[t] = tm, to
    return cum_mu, cum_om, float(dg.max())


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("grad_samples,ts", [(1, TS), (3, (1, 2))])
def test_iterates(small, variant, grad_samples, ts):
    s = small[variant]
    h = s["h"]
    worst = 0.0
    for r in range(2):
        snap, fast, steps, nm = _reference_steps(s, r, grad_samples, max(ts))
        cum_mu, cum_om, dg = _derived_terms(s, r, steps, nm, grad_samples)
        for t in ts:
            dev = h.variational(s["q0"][r:r + 1], adapt_engaged=0, eta=1.0, iter=t, eval_elbo=t + 1, elbo_samples=1, grad_samples=grad_samples,
                                output_samples=0, run_offset=r)
            assert dev["return_code"].tolist() == [ref.MAXIT] and dev["iterations"].tolist() == [t] and dev["evaluations"].tolist() == [0]
            for name, got, k, term in (("mu", dev["mu"][0], 0, cum_mu[t]), ("omega", dev["omega"][0], 1, cum_om[t])):
                e_ref, err = float(np.abs(snap[t][k] - fast[t][k]).max()), float(np.abs(got - snap[t][k]).max())
                print(f"{variant} M={grad_samples} run {r} t={t} {name}: e_ref {e_ref:.2e} device {err:.2e} derived term {term:.2e} (max |dg| {dg:.2e})")
                assert err <= 2.0 * e_ref + term, (name, t, err, e_ref, term)
                worst = max(worst, err)
    print(f"{variant} M={grad_samples}: the largest difference {worst:.2e}")


def test_library_start_and_nonfinite(small):
    """The library's start is U(-r, r) from its own counters: with a step that cannot move it (eta = 1e-300) mu after one iteration is the
    start itself.  And a run that meets a non-finite pass stops at its last finished iterate, as the reference's does: eta = 100 on the full design."""
    s = small["full"]
    h, D = s["h"], s["h"].D
    dev = h.variational(None, 1, adapt_engaged=0, eta=1e-300, iter=1, eval_elbo=2, elbo_samples=1, output_samples=0, run_offset=3)
    Lo = oracle_lib()
    want = np.array([2.0 * (2.0 * Lo.oracle_rng_uniform(SEED, 4, 0, ref.RNG_ADVI, 14, i) - 1.0) for i in range(D)])
    assert np.array_equal(dev["mu"][0], want)
    for r in range(2):
        rf = ref.sga(s["lpg"], s["q0"][r], np.zeros(D), 100.0, 50, ref.library_normals(SEED, r))
        assert rf["code"] == ref.NONFINITE and rf["t"] == 1
        dev = h.variational(s["q0"][r:r + 1], adapt_engaged=0, eta=100.0, iter=50, eval_elbo=100, elbo_samples=1, output_samples=3, run_offset=r)
        assert dev["return_code"].tolist() == [ref.NONFINITE] and dev["iterations"].tolist() == [1]
        assert np.abs(dev["mu"][0] - rf["mu"]).max() <= 1e-9 * np.abs(rf["mu"]).max() and np.isfinite(dev["q"]).all()   # it keeps its approximation


# ------------------------------------------------------------------------------------------------ 2. the ELBO
def _elbo_bound(s, pts, om):
    """What potus_log_prob_grad and the oracle differ by at the points (their mean is what the ELBO's mean can differ by: the largest is used),
    plus the entropy's rounding."""
    h, D = s["h"], s["h"].D
    lp_dev = h.log_prob_grad(np.ascontiguousarray(np.array(pts)))[0]
    lp_ora = np.array([s["lpg"](z)[0] for z in pts])
    depth = -(-D // 512) + 14
    return float(np.abs(lp_dev - lp_ora).max()), depth * EPS * float(np.abs(om).sum())


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K", [1, 5])
def test_elbo(small, variant, K):
    s = small[variant]
    h, D = s["h"], s["h"].D
    for r in range(2):
        nm = ref.library_normals(SEED, r)
        dev = h.variational(s["q0"][r:r + 1], adapt_engaged=0, eta=1.0, iter=10, eval_elbo=10, elbo_samples=K, output_samples=0, run_offset=r)
        assert dev["evaluations"].tolist() == [1] and dev["iterations"].tolist() == [10]
        # the initial ELBO at the start itself; the later one at the DEVICE's own (mu, omega), so that only the ELBO is compared
        for j, (mu, om, t) in enumerate(((s["q0"][r], np.zeros(D), 0), (dev["mu"][0], dev["omega"][0], 10))):
            pts = []
            want = ref.elbo(s["lpg"], np.array(mu), np.array(om), nm, 0, t, K, points=pts)
            lp_share, ent = _elbo_bound(s, pts, om)
            err = abs(dev["elbo"][0, j] - want)
            print(f"{variant} K={K} run {r} t={t}: ELBO {want:.6f} device off by {err:.2e}; lp share {lp_share:.2e}, entropy term {ent:.2e}")
            assert err <= lp_share + ent


# ------------------------------------------------------------------------------------------------ 3. the whole call
@pytest.mark.parametrize("variant", VARIANTS)
def test_the_whole_call(small, variant):
    s = small[variant]
    h, D = s["h"], s["h"].D
    K, tol = 20, 0.01
    kw = dict(iter=2000, eval_elbo=100, elbo_samples=K, output_samples=0)
    dev = h.variational(s["q0"], **kw)
    for r in range(2):
        nm = ref.library_normals(SEED, r)
        rf = ref.run(s["lpg"], s["q0"][r], nm, iter=2000, eval_elbo=100, elbo_samples=K)
        n_ev = rf["iterations"] // 100
        # the ELBO's bound at the reference's own points: the initial one, the chosen candidate's and its neighbours', every one of the trace
        pts, grads = [], []
        ref.elbo(s["lpg"], s["q0"][r], np.zeros(D), nm, 0, 0, K, points=pts)
        ks = [k for k in (rf["eta_index"] - 1, rf["eta_index"], rf["eta_index"] + 1) if 0 <= k < 5 and math.isfinite(rf["adapt_elbo"][k])]
        for k in ks:
            c = ref.sga(s["lpg"], s["q0"][r], np.zeros(D), ref.ETAS[k], 50, nm, stage=1 + k)
            ref.elbo(s["lpg"], c["mu"], c["omega"], nm, 1 + k, 50, K, points=pts)
        st, om_max, g1 = dict(mu=s["q0"][r], omega=np.zeros(D), s=None, t=0), 0.0, 0.0
        for j in range(1, n_ev + 1):
            st = ref.sga(s["lpg"], st["mu"], st["omega"], rf["eta"], 100, nm, t0=st["t"], s=st["s"])
            mine = []
            ref.elbo(s["lpg"], st["mu"], st["omega"], nm, 0, st["t"], K, points=mine)
            for k, z in enumerate(mine):                  # first-order sensitivity of lp(zeta_k) to the iterate
                eps = nm(ref.STAGE_ELBO, k, st["t"], D)
                g1 = max(g1, float((np.abs(s["lpg"](z)[1]) * (1.0 + np.abs(eps) * np.exp(st["omega"]))).sum()))
            pts += mine
            om_max = max(om_max, float(np.abs(st["omega"]).sum()))
        lp_share, ent = _elbo_bound(s, pts, np.full(1, om_max))
        b = lp_share + ent
        e_min = float(np.abs(rf["elbo"][:n_ev + 1]).min())
        b_delta = max((2.0 + d) * b / e_min for d in rf["deltas"])
        # ---- the margins, on the reference
        k = rf["eta_index"]
        gaps = [abs(rf["adapt_elbo"][k] - rf["adapt_elbo"][j]) for j in (k - 1, k + 1) if 0 <= j < 5] + [abs(rf["adapt_elbo"][k] - rf["elbo"][0])]
        print(f"{variant} run {r}: ELBO bound {b:.2e} (lp share {lp_share:.2e}), delta bound {b_delta:.2e}; eta* {rf['eta']} candidates {rf['adapt_elbo']}, "
              f"stop at {rf['iterations']} code {rf['code']}, deltas {rf['deltas']}")
        assert rf["code"] == ref.MEAN_CONVERGED and rf["iterations"] == 300 and rf["deltas"][0] == 1.0
        assert min(gaps) > 10.0 * b
        assert all(abs(v - tol) > 10.0 * b_delta for v in rf["means"] + rf["medians"])
        # ---- the device
        assert dev["eta_index"][r] == k and dev["eta"][r] == rf["eta"]
        assert dev["iterations"][r] == rf["iterations"] and dev["return_code"][r] == rf["code"] and dev["flags"][r] == rf["flags"]
        assert dev["evaluations"][r] == n_ev and np.isnan(dev["elbo"][r, n_ev + 1:]).all() and dev["elbo"].shape[1] == 21
        d_theta = max(float(np.abs(dev["mu"][r] - rf["mu"]).max()), float(np.abs(dev["omega"][r] - rf["omega"]).max()))
        err = float(np.abs(dev["elbo"][r, :n_ev + 1] - rf["elbo"][:n_ev + 1]).max())
        print(f"  trace: device off by {err:.2e}; iterates differ by {d_theta:.2e} at the end, sensitivity {g1:.2e}: bound {b + g1 * d_theta:.2e}")
        assert abs(dev["elbo"][r, 0] - rf["elbo"][0]) <= b and err <= b + g1 * d_theta
        assert abs(dev["adapt_elbo"][r, k] - rf["adapt_elbo"][k]) <= 1e-6 * abs(rf["adapt_elbo"][k])
        assert np.isneginf(dev["adapt_elbo"][r][np.isneginf(rf["adapt_elbo"])]).all()


# ------------------------------------------------------------------------------------------------ 4. equal bytes
@pytest.mark.parametrize("variant", VARIANTS)
def test_equal_bytes(small, variant, monkeypatch):
    s = small[variant]
    h, res = s["h"], s["res"]
    assert raw(h.variational(s["q0"], **QUICK)) == raw(res)                                    # the same call twice
    for G in ("1", "7", "300"):
        monkeypatch.setenv("POTUS_ADVI_G", G)
        assert raw(h.variational(s["q0"], **QUICK)) == raw(res), G
    monkeypatch.delenv("POTUS_ADVI_G")
    # three library runs in one call against three calls with run_offset 0, 1, 2
    three = h.variational(None, 3, **QUICK)
    assert len({three["mu"][p].tobytes() for p in range(3)}) == 3
    for p in range(3):
        one = h.variational(None, 1, run_offset=p, **QUICK)
        assert raw(one) == raw({k: three[k][p:p + 1] for k in KEYS}), p
    # 37 draws in one call against draw_offset 0 / 12 / 24, and against no draws at all
    rest = tuple(k for k in KEYS if k not in ("q", "lp", "lq", "model_passes"))
    for a, b in ((0, 12), (12, 24), (24, M)):
        part = h.variational(s["q0"], **{**QUICK, "output_samples": b - a, "draw_offset": a})
        for k in ("q", "lp", "lq"):
            assert part[k].tobytes() == np.ascontiguousarray(res[k][:, a:b]).tobytes(), (k, a)
        assert raw(part, rest) == raw(res, rest)
    none = h.variational(s["q0"], **{**QUICK, "output_samples": 0})
    assert raw(none, rest) == raw(res, rest) and none["q"].shape == (2, 0, h.D)


def three_dates():
    """tests/test_gpu_laplace.py's design: synthetic.small with three run dates that keep different polls and have different priors."""
    data = synthetic.small("full")
    Ns, Nn, S = int(data["N_state_polls"]), int(data["N_national_polls"]), int(data["S"])
    rng = np.random.default_rng(3)
    keep_s = np.stack([rng.uniform(size=Ns) < 0.5, rng.uniform(size=Ns) < 0.8, np.ones(Ns, bool)])
    keep_n = np.stack([rng.uniform(size=Nn) < 0.5, rng.uniform(size=Nn) < 0.8, np.ones(Nn, bool)])
    prior = np.tile(np.asarray(data["mu_b_prior"], dtype=np.float64), (3, 1))
    prior[0] += np.linspace(-0.3, 0.4, S)
    prior[1] -= 0.1
    return timeline.design_of(data, keep_s, keep_n, prior, np.full(3, float(data["mu_b_T_scale"])))


def test_data_sets_equal_stand_alone_handles():
    design = three_dates()
    h = Handle(design["data"], "full", chains=3, **OPTS)
    timeline.set_design(h, design)
    kw = {**QUICK, "output_samples": 9}
    q0 = np.zeros((3, h.D))
    many = h.variational(q0, **kw)
    rows, scores = h.variational_rows_device().cpu().numpy().reshape(3, 9, -1), h.variational_scores((0, 3)).cpu().numpy()
    assert not np.isin(many["return_code"], (5, 6)).any() and status_of(lambda: h.variational(q0[:2], **kw)) == 1
    for d in range(3):
        g = Handle(timeline.data_of(design, d), "full", chains=1, **OPTS)
        one = g.variational(q0[:1], run_offset=d, **kw)
        assert raw(one) == raw({k: many[k][d:d + 1] for k in KEYS}), d
        assert g.variational_rows_device().cpu().numpy().tobytes() == np.ascontiguousarray(rows[d]).tobytes()
        assert g.variational_scores((0, 3)).cpu().numpy().tobytes() == np.ascontiguousarray(scores[d:d + 1]).tobytes()
        g.close()
    assert np.abs(many["mu"][0] - many["mu"][2]).max() > 1e-3
    # timeline.variational is that call with the library's starts, and the summary per run
    lib = h.variational(None, 3, **kw)
    sm = h.variational_summary(EV)
    h.close()
    tl = timeline.variational(design, "full", draws=9, ev=EV, seed=SEED, **{k: v for k, v in kw.items() if k != "output_samples"})
    assert tl["lp"].tobytes() == lib["lp"].tobytes() and tl["lq"].tobytes() == lib["lq"].tobytes()
    assert tl["iterations"].ravel().tolist() == lib["iterations"].tolist() and tl["state"].shape == (3, 1) + sm["state"].shape[1:]
    assert tl["state"].tobytes() == sm["state"].tobytes() and tl["n_draws"].ravel().tolist() == [9, 9, 9]


def test_r_entry_point(small):
    s = small["full"]
    h, res = s["h"], s["res"]
    n, D, trace = 2, h.D, QUICK["iter"] // QUICK["eval_elbo"] + 1
    info, mu, om, elbo, ad = np.zeros((n, 6), np.int32), np.zeros((n, D)), np.zeros((n, D)), np.zeros((n, trace)), np.zeros((n, 5))
    q, lp, lq, st = np.zeros((n, M, D)), np.zeros((n, M)), np.zeros((n, M)), (C.c_int * 1)(-1)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int))
    h.L.potus_R_variational((C.c_int * 1)(h.h), (C.c_int * 11)(QUICK["iter"], 1, QUICK["elbo_samples"], QUICK["eval_elbo"], 1, QUICK["adapt_iter"], M, 0, 0, n, 1),
                            (C.c_double * 3)(1.0, 0.01, 0.0), dp(np.ascontiguousarray(s["q0"])), ip(info), dp(mu), dp(om), dp(elbo), dp(ad), dp(q), dp(lp), dp(lq), st)
    assert st[0] == 0
    got = dict(mu=mu, omega=om, elbo=elbo, adapt_elbo=ad, q=q, lp=lp, lq=lq, return_code=info[:, 0], flags=info[:, 1], iterations=info[:, 2],
               eta_index=info[:, 3], model_passes=info[:, 4], evaluations=info[:, 5])
    assert raw(got) == raw(res)


# ------------------------------------------------------------------------------------------------ 5. edges, refusals, an undisturbed run
def test_edges(small):
    s = small["full"]
    h, D, res = s["h"], s["h"].D, s["res"]
    # a start with a NaN: INIT for that run alone, NaN rows, the other run's bytes unchanged
    bad = np.array(s["q0"])
    bad[0, 5] = np.nan
    both = h.variational(bad, **QUICK)
    ms = h.variational_timing()
    assert all(ms[k] > 0 for k in ("adapt_ms", "grad_ms", "elbo_ms", "draws_ms"))
    assert both["return_code"][0] == ref.INIT and both["iterations"][0] == 0 and both["eta_index"][0] == -1
    assert np.isnan(both["q"][0]).all() and np.isnan(both["lp"][0]).all() and np.isnan(both["lq"][0]).all()
    assert np.isnan(both["mu"][0]).all() and np.isnan(both["omega"][0]).all() and np.isneginf(both["elbo"][0, 0]) and np.isnan(both["elbo"][0, 1:]).all()
    assert raw({k: both[k][1:2] for k in KEYS}) == raw({k: res[k][1:2] for k in KEYS})
    sm = h.variational_summary(EV)
    assert sm["n_draws"].tolist() == [0, M] and np.isnan(sm["state"][0]).all() and np.isfinite(sm["state"][1]).all()
    rows = h.variational_rows_device().cpu().numpy()
    assert np.isnan(rows[:M]).all() and np.isfinite(rows[M:, 7:]).all()
    # iter < eval_elbo: no evaluation, MAXIT; iter no multiple of eval_elbo: the tail has none
    short = h.variational(s["q0"], adapt_engaged=0, iter=7, eval_elbo=10, elbo_samples=2, output_samples=2)
    assert short["return_code"].tolist() == [ref.MAXIT] * 2 and short["iterations"].tolist() == [7, 7] and short["evaluations"].tolist() == [0, 0]
    assert short["elbo"].shape == (2, 1) and np.isfinite(short["elbo"]).all() and np.isnan(short["adapt_elbo"]).all() and short["eta"].tolist() == [1.0, 1.0]
    tail = h.variational(s["q0"], adapt_engaged=0, iter=25, eval_elbo=10, elbo_samples=2, output_samples=0, tol_rel_obj=0.0)
    assert tail["return_code"].tolist() == [ref.MAXIT] * 2 and tail["iterations"].tolist() == [25, 25] and tail["evaluations"].tolist() == [2, 2]
    # lq is the normal's log density at the draw, and lp the library's log density of it
    z = (res["q"] - res["mu"][:, None, :]) / np.exp(res["omega"])[:, None, :]
    lq = -0.5 * (z * z).sum(2) - res["omega"].sum(1)[:, None] - 0.5 * D * ref.LOG_2PI
    assert np.abs(res["lq"] - lq).max() <= 1e-10 * np.abs(lq).max()
    assert res["lp"].tobytes() == h.log_prob_grad(np.ascontiguousarray(res["q"].reshape(-1, D)))[0].tobytes()


def test_refusals_and_an_undisturbed_run(small):
    s = small["full"]
    h, data, q0 = s["h"], s["data"], s["q0"]
    ARG, STATE, UNSUP = 1, 4, 6
    for bad in (dict(iter=0), dict(grad_samples=0), dict(grad_samples=1 << 20), dict(elbo_samples=0), dict(elbo_samples=1 << 20), dict(eval_elbo=0),
                dict(adapt_engaged=2), dict(adapt_iter=0), dict(output_samples=-1), dict(eta=0.0), dict(eta=math.inf), dict(tol_rel_obj=-1.0),
                dict(elbo_offset=math.nan), dict(draw_offset=-1), dict(run_offset=-1), dict(algorithm=2)):
        assert status_of(lambda: h.variational(q0, **{**QUICK, **bad})) == ARG, bad
    assert status_of(lambda: h.variational(q0, **{**QUICK, "algorithm": "fullrank"})) == UNSUP
    assert status_of(lambda: h.variational(None, 0)) == ARG
    assert h.L.potus_advi_timing(None) == ARG
    assert h.L.potus_advi(12345, None, None, 1, None, None, None, None, None, None, None, None) == STATE
    assert h.L.potus_advi(h.h, None, None, 1, None, None, None, None, None, None, None, None) == ARG            # null info_out
    hk = Handle(data, "full", chains=1, seed=SEED, cus_per_chain=2, twin=0)
    assert hk.cus_per_chain == 2 and status_of(lambda: hk.variational(q0, **QUICK)) == UNSUP
    hk.close()
    hd = Handle(data, "full", chains=1, seed=SEED, cus_per_chain=1, twin=0, metric=_abi.METRICS["dense_e"])
    assert status_of(lambda: hd.variational(q0, **QUICK)) == UNSUP
    hd.close()
    f = Handle(data, "full", chains=1, **OPTS)
    with pytest.raises(PotusError):
        f.variational_scores()
    import torch
    buf = torch.empty(4096, dtype=torch.float64, device="cuda:0")
    assert f.L.potus_advi_write_array_device(f.h, 0, 8, C.c_void_p(buf.data_ptr())) == STATE
    f.variational(q0[:1], **{**QUICK, "output_samples": 0})
    assert f.L.potus_advi_write_array_device(f.h, 0, 8, C.c_void_p(buf.data_ptr())) == STATE   # a call without draws keeps no rows
    f.variational(q0[:1], **{**QUICK, "output_samples": 3})
    assert status_of(lambda: f.variational(q0[:1], **{**QUICK, "iter": 0})) == ARG
    assert f.L.potus_advi_write_array_device(f.h, 0, 8, C.c_void_p(buf.data_ptr())) == 0       # a refused call leaves the last rows alone
    assert status_of(lambda: f.variational_rows_device((5, 5))) == ARG and status_of(lambda: f.variational_scores((3, 3))) == ARG
    f.close()
    # a sampling run with a refused and a successful call in its middle gives the bytes of an uninterrupted one
    run = dict(chains=2, num_warmup=20, num_samples=20, **OPTS)
    a, b = Handle(data, "full", **run), Handle(data, "full", **run)
    before = b.variational(q0, **QUICK)
    for x_ in (a, b):
        x_.init()
    a.run(40)
    b.run(20)
    assert status_of(lambda: b.variational(q0, **{**QUICK, "elbo_samples": 0})) == ARG
    mid = b.variational(q0, **QUICK)
    b.run(20)
    assert raw(before) == raw(mid) == raw(s["res"])
    assert a.draws().tobytes() == b.draws().tobytes() and a.chain_status() == b.chain_status()
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 6. downstream
@pytest.mark.parametrize("variant", VARIANTS)
def test_downstream_blocks(small, variant):
    s = small[variant]
    h, data = s["h"], s["data"]
    T, S = int(data["T"]), int(data["S"])
    res = h.variational(s["q0"], **QUICK)
    rows = h.variational_rows_device().cpu().numpy()
    assert rows.shape == (2 * M, h.n_cols)
    assert rows[:, 0].tobytes() == res["lp"].tobytes() and np.isnan(rows[:, 1:7]).all()
    assert np.ascontiguousarray(rows[:, 7:]).tobytes() == h.constrain(res["q"].reshape(2 * M, -1)).tobytes()
    a, b, _ = h.layout["predicted_score"]
    ps = rows[:, a:b].reshape(2, M, S, T).transpose(0, 1, 3, 2)                        # predicted_score is T x S column-major
    for days in ((0, T), (T - 1, T), (3, 7)):
        x = h.variational_scores(days).cpu().numpy()
        assert x.shape == (2, M, days[1] - days[0], S)
        assert x.tobytes() == np.ascontiguousarray(ps[:, :, days[0]:days[1]]).tobytes(), days
    out = h.variational_summary(EV, (T - 3, T), ev_to_win=200)
    assert out["n_draws"].tolist() == [M, M]
    for p in range(2):
        want = timeline_ref.summary(ps[p][:, T - 3:], data["state_weights"], EV, ev_to_win=200)
        for key, mean_col in (("state", 2), ("national", 2), ("electoral_votes", None)):  # test_gpu_timeline._compare's tolerances
            err = np.abs(out[key][p] - np.asarray(want[key]))
            for j in range(err.shape[-1]):
                assert err[..., j].max() <= (1e-12 if j == mean_col else 1e-15), (key, j, err[..., j].max())
    blk = h.variational_scores((0, T)).reshape(2 * M, T, S).contiguous()
    o = outcomes_of_block(blk, data["state_weights"], EV)
    w = outcomes_ref.outcomes_vectorised(ps.reshape(2 * M, T, S), outcomes_ref.normalised_weights(data["state_weights"]), EV)
    assert o.n_draws == 2 * M
    for k in ("ev_hist", "tipping", "joint"):
        assert np.array_equal(getattr(o, k), w[k]), k


def test_the_model_s_surface_and_inits():
    """PotusModel.variational on the no-mode small design: the Variational result's surface, and .inits(4): distinct draws, one per run, that
    sample(inits=...) accepts -- its first saved warm-up rows are the oracle's transitions from exactly those rows."""
    v = "no_mode_adjustment"
    data = synthetic.small(v)
    vi = PotusModel(v).variational(data, runs=4, iter=2000, elbo_samples=20, output_samples=250)
    try:
        D = vi.draws.shape[1]
        assert vi.draws.shape[0] == 1000 and vi.ok.all() and np.isfinite(vi.log_ratio).all() and np.isfinite(vi.elbo).all()
        assert vi.mean.shape == vi.sd.shape == (4, D) and (vi.sd > 0).all() and vi.elbo_path.shape == (4, 21)
        print("codes", vi.return_code.tolist(), "iterations", vi.iterations.tolist(), "eta", vi.eta.tolist(), "elbo", vi.elbo.tolist(),
              "k-hat", vi.pareto_k, "sd log ratio", vi.log_ratio.std())
        assert vi.scores().shape[0] == 1000 and vi.summary(EV)["n_draws"].tolist() == [250] * 4 and vi.outcomes(EV).n_draws == 1000
        init = vi.inits(4, seed=0)
        assert init.shape == (4, D) and len({r.tobytes() for r in init}) == 4
        for c in range(4):
            assert (vi.draws[c * 250:(c + 1) * 250] == init[c]).all(1).sum() == 1        # chain c starts from a draw of run c
        fit = PotusModel(v).sample(data, seed=SEED, chains=4, iter_warmup=20, iter_sampling=5, refresh=25, save_warmup=True, inits=init, cus_per_chain=1, twin=0)
        d = fit._hs[0].draws()
        m = OracleModel(data, v)
        o = m.default_opts(num_warmup=20, num_samples=5, seed=SEED, fast_grad=0, save_warmup=1)
        for c in range(4):
            rf = m.sample_chain(c + 1, o, q0=init[c])[0]
            assert np.array_equal(d[c, :3, 3:6], rf[:3, 3:6]) and d[c, 0, 2] == rf[0, 2], c
            assert np.allclose(d[c, :3, 7:], rf[:3, 7:], rtol=1e-6, atol=1e-7), c
        for hh in fit._hs:
            hh.close()
    finally:
        vi.close()
