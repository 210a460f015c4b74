"""k_opt_lbfgs step by step on the MI355X: every iteration of the device's own trajectory against one iteration of tests/lbfgs_ref.py (numpy,
written from the header's and DESIGN.md section 4k's text) from the same state, the five stop rules recomputed at every accepted iterate, and
the discrete outcome -- code, iterations, evaluations -- of whole runs.  The objective of the reference is the handle's own potus_log_prob_grad
(the bytes the kernel's pass computes: tests/test_gpu_pathfinder.py::test_trajectory), with optimize_ref.remove_jacobian around it for
jacobian = 0, so what is compared is the optimiser; the pass is held to the oracle elsewhere.

Designs (lbfgs_ref.designs): synthetic.small of both variants (D = 292 / 260: one trip of every thread-strided loop) and a `wide` design with
D = 805 / 697, more than the 512 threads of the workgroup and no multiple of them: two trips, the second ragged.  Two starts each, U(-1, 1) and
U(-2, 2).  tests/test_optimize_host.py runs the same inputs on the CPU oracle and asserts there which branches they reach (first-trial accept,
expansion, both ways into the bracket, secant zoom, far-end updates, the non-finite trial and bisection, the near-end update that flips the
bracket), that every comparison stays 1e-4 and more (relative) from its threshold, and that each of the codes 1-7 ends a path.

Never reached, by these inputs or by 2 592 further runs on the oracle (72 starts x 3 radii x 2 histories x 3 first steps, both small designs):
  zoom_near without the flip   a zoom trial BETWEEN the ends that rises above the near end with a derivative still above 0.9 g'd: the
                               derivative would have to fall by less than a tenth over the near part of a bracket whose far end already
                               failed -- the log density is close to concave along an ascent direction;
  retry_gradient               needs 20 trials without a Wolfe point along a direction with a history; no search here took more than 8;
  skipped_pair                 a Wolfe step has s'y >= 0.1 alpha g'd > 0;
  history_reset                g'Hg > 0 whenever every kept pair has s'y > 0, up to rounding.
The reference implements the four (from the text), the device's are unexercised; no probe or build switch forces them.

Bounds.  e_ref is the reference's own error, the spread between its float64 and its longdouble dot products from the same state; a compared
vector is held to 2 e_ref plus one rounding term for the device's other summation order:
  x_{l+1}     alpha (2 m + 4) DEPTH eps max_i T_i, with T_i the sum of the absolute values of the 2 m + 1 terms of entry i of the direction
              (every coefficient taken as the sum of the absolute terms of its dot product: lbfgs_ref.two_loop) and DEPTH = ceil(D / 512) + 14
              as tests/test_gpu_pathfinder.py derives it; plus eps |x| for the fused x + alpha d; plus, where alpha came out of a secant,
              |d| times alpha's own bound:
  alpha       the secant's value over the corners of its derivatives +- (2 m + 5) DEPTH eps sum_i |g_i| T_i (lbfgs_ref._spread), carried
              from trial to trial.
A comparison of the state machine is skipped only where the reference's clearance is below 1e-9; for these inputs there is none (asserted).
Measured on one MI355X: DESIGN.md section 4k."""
import numpy as np
import pytest

import lbfgs_ref as lb
import optimize_ref as oref
from us_potus_model_amd.sampler import Handle

pytestmark = pytest.mark.gpu
OPTS = dict(seed=1843, cus_per_chain=1, twin=0)
DESIGNS = ("small_full", "small_nomode", "wide_full", "wide_nomode")
EPS = lb.EPS
PF = dict(num_elbo_draws=1, num_draws=0)
MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


class Device:
    """A design on the device: the handle, the two starts and the objective q -> (lp, g) of either Jacobian setting."""

    def __init__(self, name):
        data, variant = lb.designs()[name]
        self.h = Handle(data, variant, chains=1, **OPTS)
        self.D, self.irho = self.h.D, oref.rho_index(data, variant)
        self.q0 = lb.starts(self.D)

    def fun(self, jacobian=1):
        def f(q):
            lp, g = self.h.log_prob_grad(q)
            with np.errstate(all="ignore"):
                return (float(lp[0]), g[0]) if jacobian else oref.remove_jacobian(float(lp[0]), g[0], q, self.irho)
        return f


@pytest.fixture(scope="module")
def devices():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Device(name)
        return made[name]
    yield get
    for d in made.values():
        d.h.close()
    if MEASURED:
        print("\nlargest measured / bound:", {k: f"{v:.3g}" for k, v in sorted(MEASURED.items())})


def _note(key, value):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(value))


def _trajectory(dev, q0, **opts):
    """potus_pathfinder's record of k_opt_lbfgs per path: (x, lp, g)[0..L], code, L; and potus_optimize's evaluations of the same run."""
    pf = {("max_lbfgs_iters" if k == "iter" else "lbfgs_history_size" if k == "history_size" else k): v for k, v in opts.items()}
    res = dev.h.pathfinder(q0, trajectory=True, **PF, **pf)
    opt = dev.h.optimize(q0, jacobian=1, **opts)
    assert res["optimize_code"].tolist() == opt["return_code"].tolist() and res["iterations"].tolist() == opt["iterations"].tolist()
    out = []
    for p in range(q0.shape[0]):
        L = int(res["iterations"][p])
        x, g = np.ascontiguousarray(res["x"][p][:L + 1]), np.ascontiguousarray(res["g"][p][:L + 1])
        lp, gr = dev.h.log_prob_grad(x)
        assert g.tobytes() == gr.tobytes() and x[0].tobytes() == q0[p].tobytes() and x[L].tobytes() == opt["q"][p].tobytes() and lp[L] == opt["lp"][p]
        out.append(dict(x=x, lp=lp, g=g, L=L, code=int(opt["return_code"][p]), evals=int(opt["grad_evals"][p])))
    return out


# ------------------------------------------------------------------------------------------------ a. every iteration, replayed
def _replay_path(dev, t, tag, **opts):
    m, D = opts["history_size"], dev.D
    r64 = lb.replay(dev.fun(), t["x"], t["lp"], t["g"], t["L"], long=False, **opts)
    rld = lb.replay(dev.fun(), t["x"], t["lp"], t["g"], t["L"], long=True, **opts)
    k = (2 * m + 4) * lb.depth(D) * EPS
    searched = 0
    for l, (a, b) in enumerate(zip(r64, rld)):
        s, sl = a["step"], b["step"]
        where = (tag, l, s["rec"].branches)
        assert s["rec"].clearance >= lb.CLEAR_MIN and a["accept_rec"].clearance >= lb.CLEAR_MIN, where + (s["rec"].closest, s["rec"].clearance)
        assert s["ok"] and not s["retried"] and s["rec"].branches == sl["rec"].branches, where
        assert s["first_trial"] == (opts["init_alpha"] if l == 0 else 1.0)
        x0, x1, d = t["x"][l], t["x"][l + 1], s["d"]
        # the step length the device took, from its own two points
        alpha_dev = float(d @ (x1 - x0)) / float(d @ d)
        # (a projection on the reference's d: the rounding of x_{l+1} and of the two sums, and the direction's own bound along d)
        e_alpha = (2.0 * abs(s["alpha"] - sl["alpha"]) + s["alpha_err"] + 4.0 * EPS * (abs(s["alpha"]) + float(np.abs(d) @ np.abs(x0)) / float(d @ d))
                   + s["alpha"] * k * float(np.abs(d) @ s["T"]) / float(d @ d))
        _note("alpha", abs(alpha_dev - s["alpha"]) / e_alpha)
        assert abs(alpha_dev - s["alpha"]) <= e_alpha, where + (alpha_dev, s["alpha"], e_alpha)
        if s["search_evals"] == 1:                         # the device's first trial itself
            assert abs(alpha_dev - s["first_trial"]) <= e_alpha, where
        e_ref = float(np.abs(s["x"] - sl["x"]).max())
        term = s["alpha"] * k * float(s["T"].max()) + s["alpha_err"] * float(np.abs(d).max()) + EPS * float(np.abs(x1).max())
        err = float(np.abs(x1 - s["x"]).max())
        _note("x", err / (2.0 * e_ref + term))
        _note("x error", err)
        assert err <= 2.0 * e_ref + term, where + (err, e_ref, term)
        # both Wolfe conditions on the device's own values
        gd0, dh = lb.dot(t["g"][l], d, long=True), lb.dot(t["g"][l + 1], d, long=True)
        assert gd0 > 0 and lb.wolfe(t["lp"][l], gd0, s["alpha"], t["lp"][l + 1], dh) == (True, True), where
        searched += s["search_evals"]
    assert t["code"] != lb.LSFAIL and searched == t["evals"] - 1, (tag, searched, t["evals"])
    return r64


@pytest.mark.parametrize("m", lb.HISTORIES)
@pytest.mark.parametrize("design", DESIGNS)
def test_every_iteration_is_the_reference_iteration(devices, design, m):
    dev = devices(design)
    seen = set()
    for ia in lb.INIT_ALPHAS:
        opts = dict(history_size=m, init_alpha=ia, iter=lb.ITER)
        for p, t in enumerate(_trajectory(dev, dev.q0, **opts)):
            assert t["L"] >= min(m + 9, 29)                # the ring wraps within the compared range
            for r in _replay_path(dev, t, (design, m, ia, p), **opts):
                seen.update(r["step"]["rec"].branches)
    print(design, "history", m, "branches", sorted(seen), "measured / bound", {k: f"{v:.3g}" for k, v in MEASURED.items()})
    assert {"accept_first", "bracket_armijo", "secant", "zoom_far"} <= seen


def test_the_bracket_flips(devices):
    """lbfgs_ref.FLIP: the zoom trial that becomes the near end and turns the old near end into the far end (iteration 0 on the oracle)."""
    dev = devices(lb.FLIP["design"])
    opts = dict(history_size=lb.FLIP["history_size"], init_alpha=lb.FLIP["init_alpha"], iter=lb.ITER)
    t, = _trajectory(dev, lb.flip_start(dev.D)[None], **opts)
    r = _replay_path(dev, t, "flip", **opts)
    assert any("zoom_near_flip" in a["step"]["rec"].branches for a in r)


# ------------------------------------------------------------------------------------------------ b. the stop rules, from the trajectory
@pytest.mark.parametrize("design", DESIGNS)
def test_stop_rules(devices, design):
    dev = devices(design)
    for name, kw in [("defaults", {})] + [(k, dict(lb.OFF, **t)) for k, t in lb.SINGLE.items()]:
        opts = dict(kw, iter=100)
        thr = lb.LBFGS(None, **opts).thresholds()
        for p, t in enumerate(_trajectory(dev, dev.q0, **opts)):
            L = t["L"]
            r = lb.replay(None, t["x"], t["lp"], t["g"], L, searches=False, **opts)
            fired = [a["code"] for a in r]
            q = r[-1]["rules"]
            print(f"{design} {name} path {p}: code {t['code']} at L = {L}; quantities / thresholds there " +
                  " ".join(f"{k}={q[k] / thr[k]:.3g}" for k in lb.RULES if thr[k] > 0))
            assert all(a["accept_rec"].clearance >= lb.CLEAR_MIN for a in r), (name, p)
            assert 1 <= t["code"] <= 5 and fired[-1] == t["code"] and not any(fired[:-1]), (name, p, t["code"], fired)
            if name != "defaults":
                assert t["code"] == 1 + lb.RULES.index(name)
            # the rule's quantity where only one is on: the first below, every earlier one above
            only = [k for k in lb.RULES if thr[k] > 0]
            if len(only) == 1:
                v = [a["rules"][only[0]] for a in r]
                assert v[-1] < thr[only[0]] and min(v[:-1]) >= thr[only[0]]


# ------------------------------------------------------------------------------------------------ c. whole runs, discrete outcomes
@pytest.mark.parametrize("jacobian", [0, 1])
@pytest.mark.parametrize("design", DESIGNS)
def test_whole_runs(devices, design, jacobian):
    dev = devices(design)
    fun = dev.fun(jacobian)
    for name, kw, code in (("defaults", {}, lb.RELGRAD), ("maxit", dict(iter=lb.ITER), lb.MAXIT), ("lsfail", dict(init_alpha=1e300), lb.LSFAIL)):
        res = dev.h.optimize(dev.q0, jacobian=jacobian, **kw)
        for p in range(2):
            ref = lb.LBFGS(fun, **kw).run(dev.q0[p])
            got = (int(res["return_code"][p]), int(res["iterations"][p]), int(res["grad_evals"][p]))
            print(f"{design} jacobian={jacobian} {name} path {p}: device (code, iterations, evaluations) {got}, reference {(ref['code'], ref['iterations'], ref['evals'])}")
            assert all(s["rec"].clearance >= lb.CLEAR_MIN for s in ref["steps"])
            assert got == (ref["code"], ref["iterations"], ref["evals"]) and got[0] == code, (name, p)
            if name == "lsfail":
                assert got[1:] == (0, 21) and res["q"][p].tobytes() == dev.q0[p].tobytes()
    # the first three iterations: q_out under the bound of (a), summed over the steps taken, before anything can be amplified
    m = lb.DEFAULTS["history_size"]
    k = (2 * m + 4) * lb.depth(dev.D) * EPS
    for it in (1, 2, 3):
        res = dev.h.optimize(dev.q0, jacobian=jacobian, iter=it)
        for p in range(2):
            r64, rld = lb.LBFGS(fun, iter=it).run(dev.q0[p], errors=True), lb.LBFGS(fun, long=True, iter=it).run(dev.q0[p], errors=True)
            assert (int(res["return_code"][p]), int(res["iterations"][p]), int(res["grad_evals"][p])) == (lb.MAXIT, it, r64["evals"])
            x = r64["x"][-1]
            e_ref = float(np.abs(x - rld["x"][-1]).max())
            term = sum(s["alpha"] * k * float(s["T"].max()) + s["alpha_err"] * float(np.abs(s["d"]).max()) for s in r64["steps"]) + it * EPS * float(np.abs(x).max())
            err = float(np.abs(res["q"][p] - x).max())
            _note(f"q_out jacobian={jacobian}", err / (2.0 * e_ref + term))
            assert err <= 2.0 * e_ref + term, (it, p, err, e_ref, term)
