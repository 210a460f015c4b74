"""The state machine of k_opt_lbfgs in numpy, iteration by iteration (tests/test_optimize_host.py, tests/test_gpu_lbfgs.py).

Written from the potus_optimize block of include/potus_hmc.h and DESIGN.md section 4k: L-BFGS with a ring of history_size pairs, the two-loop
recursion scaled by s'y / y'y of the newest pair, a strong-Wolfe search on directional derivatives (c1 = 1e-4, c2 = 0.9), CmdStan 2.24's
five rules in code order with strict <.  The objective is any callable q -> (lp, g): the CPU oracle in the host tests, the handle's own
potus_log_prob_grad in the GPU tests, so that what is compared there is the optimiser and not the model pass.

Every dot product goes through `dot`, float64 by default and numpy's longdouble with long = True; the spread between the two runs of the same
state is the reference's own error e_ref, in the convention of tests/test_gpu_pathfinder.py.  `dense_h` is a second, independent form of the
direction: H built as a D x D matrix from gamma I by the BFGS product formula over the same pairs.

A record per iteration names the branches the search took and keeps the `clearance`: the smallest relative distance of any comparison the
iteration made from its threshold (|a - b| / max(|a|, |b|); for the sign of a dot product |sum| / sum |terms|; for two values of the
objective, relative to the larger of their gains over the search's starting value).  A comparison closer to its
threshold than rounding can decide either way, so the GPU tests only compare iterations whose clearance is at least CLEAR_MIN -- and the host
tests assert that, for the inputs the GPU tests use, there is no other kind.

Branch names: accept_first (the first trial satisfies both conditions), expansion, bracket_armijo (sufficient increase fails, or the value is
not above the near end's), bracket_derivative (the derivative has changed sign), secant (zoom on the secant of the end derivatives), bisection,
nonfinite (a non-finite trial becomes the far end), zoom_far / zoom_near (a zoom trial replaces the far / the near end; zoom_near_flip: the old
near end becomes the far end first), retry_gradient, skipped_pair, history_reset."""
from __future__ import annotations

import itertools
import math

import numpy as np

EPS = 2.0 ** -52
C1, C2, LS_MAX, INIT_ATTEMPTS = 1e-4, 0.9, 20, 100
ABSF, RELF, ABSGRAD, RELGRAD, ABSX, MAXIT, LSFAIL, INIT = range(1, 9)
RULES = ("absf", "relf", "absgrad", "relgrad", "absx")
DEFAULTS = dict(history_size=5, iter=2000, init_alpha=1e-3, tol_obj=1e-12, tol_rel_obj=1e4, tol_grad=1e-8, tol_rel_grad=1e7, tol_param=1e-8)
OFF = dict(tol_obj=0.0, tol_rel_obj=0.0, tol_grad=0.0, tol_rel_grad=0.0, tol_param=0.0)
CLEAR_MIN = 1e-9
REACHABLE = ("accept_first", "expansion", "bracket_armijo", "bracket_derivative", "secant", "bisection", "nonfinite", "zoom_far")


def dot(a, b, long=False):
    if long:
        return float(np.dot(a.astype(np.longdouble), b.astype(np.longdouble)))
    return float(np.dot(a, b))


def depth(D):
    """Additions a partial sum passes through on the device: a thread's strided share, six DPP steps, eight waves (test_gpu_pathfinder.py)."""
    return -(-D // 512) + 14


class Rec:
    """What one iteration did: branch names in order, and the comparison that came closest to its threshold."""

    def __init__(self):
        self.branches, self.clearance, self.closest = [], math.inf, None

    def _note(self, c, name):
        if c < self.clearance:
            self.clearance, self.closest = c, name

    def less(self, a, b, name, strict=True):
        """a < b (or a <= b), recorded with its relative distance."""
        s = max(abs(a), abs(b))
        self._note(abs(a - b) / s if s > 0 and math.isfinite(s) else math.inf, name)
        return a < b if strict else a <= b

    def gain(self, a, b, f0, name, strict=True):
        """a < b (or a <= b) for two values of the objective along a search from f0: the distance is relative to the larger of the two GAINS
        a - f0 and b - f0, which is what the search compares -- relative to |f| every step near the mode would count as undecided."""
        s = max(abs(a - f0), abs(b - f0))
        self._note(abs(a - b) / s if s > 0 and math.isfinite(s) else math.inf, name)
        return a < b if strict else a <= b

    def positive(self, v, scale, name):
        """v > 0 for a sum v whose absolute terms add up to `scale`."""
        self._note(abs(v) / scale if scale > 0 and math.isfinite(scale) else math.inf, name)
        return v > 0.0


# ------------------------------------------------------------------------------------------------ the direction, twice
def two_loop(g, S, Y, gamma, long=False, absolute=False):
    """H g over the pairs S[k], Y[k] (oldest first), H0 = gamma I.  With absolute = True also T: per entry, the sum of the absolute values of
    the 2 m + 1 terms the entry is made of, every coefficient taken as the sum of the absolute terms of its dot product."""
    q = g.copy()
    T = np.abs(g)
    n = len(S)
    rho = [1.0 / dot(S[k], Y[k], long) for k in range(n)]
    a, a_abs = [0.0] * n, [0.0] * n
    for k in reversed(range(n)):
        a[k] = rho[k] * dot(S[k], q, long)
        a_abs[k] = abs(rho[k]) * float(np.abs(S[k]) @ T)
        q = q - a[k] * Y[k]
        T = T + a_abs[k] * np.abs(Y[k])
    if n:
        q, T = gamma * q, abs(gamma) * T
    for k in range(n):
        b = rho[k] * dot(Y[k], q, long)
        b_abs = abs(rho[k]) * float(np.abs(Y[k]) @ T)
        q = q + (a[k] - b) * S[k]
        T = T + (a_abs[k] + b_abs) * np.abs(S[k])
    return (q, T) if absolute else q


def dense_h(S, Y, gamma, D):
    """The same H as a matrix: H <- (I - rho s y') H (I - rho y s') + rho s s', oldest pair first.  Returns (H, A): A is the same product
    formula on absolute values, A >= |H| entry by entry, which is what the rounding of the two matrix products of every update scales with."""
    H = (gamma if len(S) else 1.0) * np.eye(D)
    A = np.abs(H)
    I = np.eye(D)
    for s, y in zip(S, Y):
        rho = 1.0 / float(s @ y)
        V = I - rho * np.outer(y, s)
        H = V.T @ H @ V + rho * np.outer(s, s)
        A = np.abs(V).T @ A @ np.abs(V) + abs(rho) * np.outer(np.abs(s), np.abs(s))
    return H, A


# ------------------------------------------------------------------------------------------------ the line search
def _expand_to(alpha, a_lo, d_lo, dh):
    an = alpha + (alpha - a_lo) * dh / (d_lo - dh) if d_lo > dh else 10.0 * alpha
    return min(max(an, 1.1 * alpha), 10.0 * alpha)


def _inside(a_lo, d_lo, a_hi, d_hi, hi_ok):
    """The next trial inside the bracket and whether it is the secant's."""
    w, t, sec = a_hi - a_lo, 0.5, False
    if hi_ok and (d_lo - d_hi) * w > 0.0:
        ts = d_lo / (d_lo - d_hi)
        if ts > 0.0:
            t, sec = min(max(ts, 0.1), 0.9), True
    return a_lo + t * w, sec


def _spread(fn, args, errs):
    """Largest change of fn over the corners of args +- errs: a first-order bound on what the errors of the arguments do to its value."""
    base = fn(*args)
    worst = 0.0
    idx = [i for i, e in enumerate(errs) if e > 0.0]
    for signs in itertools.product((-1.0, 1.0), repeat=len(idx)):
        p = list(args)
        for i, sg in zip(idx, signs):
            p[i] = args[i] + sg * errs[i]
        v = fn(*p)
        if math.isfinite(v):
            worst = max(worst, abs(v - base))
    return worst


def search(fun, x, f0, d, gd0, alpha0, rec, long=False, dd=None):
    """A strong-Wolfe search from x along d (gd0 = g'd > 0).  dd(g_t): the absolute error assumed in a derivative g_t'd, carried to the step
    lengths that are secants of derivatives (the returned `alpha_err`).  Returns a dict; `ok` is False after LS_MAX trials without a step."""
    a_lo, h_lo, d_lo, e_alo, e_dlo = 0.0, f0, gd0, 0.0, 0.0
    a_hi, h_hi, d_hi, e_ahi, e_dhi = 0.0, 0.0, 0.0, 0.0, 0.0
    hi_ok, zoom = False, False
    alpha, e_alpha = alpha0, 0.0
    trials = []
    for ev in range(LS_MAX):
        xt = x + alpha * d
        ft, gt = fun(xt)
        dh = dot(gt, d, long)
        e_dh = dd(gt) if dd is not None else 0.0
        trials.append(alpha)
        fin = bool(np.isfinite(ft) and np.isfinite(gt).all() and np.isfinite(dh))
        expand = False
        if not fin:
            rec.branches.append("nonfinite")
            a_hi, e_ahi, hi_ok, zoom = alpha, e_alpha, False, True
        else:
            worse = rec.gain(ft, f0 + C1 * alpha * gd0, f0, "sufficient increase") or ((zoom or ev > 0) and rec.gain(ft, h_lo, f0, "value against the near end", strict=False))
            if worse:
                rec.branches.append("zoom_far" if zoom else "bracket_armijo")
                a_hi, h_hi, d_hi, e_ahi, e_dhi, hi_ok, zoom = alpha, ft, dh, e_alpha, e_dh, True, True
            elif rec.less(abs(dh), C2 * gd0, "curvature", strict=False):
                if ev == 0:
                    rec.branches.append("accept_first")
                return dict(ok=True, alpha=alpha, alpha_err=e_alpha, x=xt, f=ft, g=gt, dh=dh, evals=ev + 1, trials=trials)
            elif not zoom:
                if not rec.positive(dh, float(np.abs(gt) @ np.abs(d)), "sign of the trial's derivative"):
                    rec.branches.append("bracket_derivative")
                    a_hi, h_hi, d_hi, e_ahi, e_dhi, hi_ok = a_lo, h_lo, d_lo, e_alo, e_dlo, True
                    a_lo, h_lo, d_lo, e_alo, e_dlo, zoom = alpha, ft, dh, e_alpha, e_dh, True
                else:
                    rec.branches.append("expansion")
                    rec.less(dh, d_lo, "derivative still falling")
                    e_new = _spread(_expand_to, (alpha, a_lo, d_lo, dh), (e_alpha, e_alo, e_dlo, e_dh))
                    an = _expand_to(alpha, a_lo, d_lo, dh)
                    a_lo, h_lo, d_lo, e_alo, e_dlo = alpha, ft, dh, e_alpha, e_dh
                    alpha, e_alpha, expand = an, e_new, True
            else:
                if not rec.positive(dh * (a_hi - a_lo), float(np.abs(gt) @ np.abs(d)) * abs(a_hi - a_lo), "side of the zoom trial"):
                    rec.branches.append("zoom_near_flip")
                    a_hi, h_hi, d_hi, e_ahi, e_dhi, hi_ok = a_lo, h_lo, d_lo, e_alo, e_dlo, True
                else:
                    rec.branches.append("zoom_near")
                a_lo, h_lo, d_lo, e_alo, e_dlo = alpha, ft, dh, e_alpha, e_dh
        if ev + 1 < LS_MAX and not expand:
            fn = lambda al, dl, ah, dhh: _inside(al, dl, ah, dhh, hi_ok)[0]
            e_new = _spread(fn, (a_lo, d_lo, a_hi, d_hi), (e_alo, e_dlo, e_ahi, e_dhi if hi_ok else 0.0))
            alpha, sec = _inside(a_lo, d_lo, a_hi, d_hi, hi_ok)
            e_alpha = e_new
            rec.branches.append("secant" if sec else "bisection")
    return dict(ok=False, evals=LS_MAX, trials=trials)


# ------------------------------------------------------------------------------------------------ the iteration
class State:
    """What the optimiser carries from one accepted point to the next."""

    def __init__(self, x, f, g, opts):
        self.x, self.f, self.g = np.array(x, dtype=np.float64), float(f), np.array(g, dtype=np.float64)
        self.S, self.Y, self.gamma, self.it = [], [], 1.0, 0
        self.d, self.T, self.gd = self.g.copy(), np.abs(self.g), None
        self.o = opts

    def history(self):
        return len(self.S)


class LBFGS:
    def __init__(self, fun, long=False, **opts):
        unknown = set(opts) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"unknown options {sorted(unknown)}")
        self.fun, self.long = fun, long
        self.o = dict(DEFAULTS, **opts)
        self.m = int(self.o["history_size"])

    def thresholds(self):
        o = self.o
        return dict(absf=o["tol_obj"], relf=o["tol_rel_obj"] * EPS, absgrad=o["tol_grad"], relgrad=o["tol_rel_grad"] * EPS, absx=o["tol_param"])

    def start(self, x0, f0=None, g0=None):
        """The state at the start; (f0, g0) given: no evaluation."""
        if f0 is None:
            f0, g0 = self.fun(np.asarray(x0, dtype=np.float64))
        st = State(x0, f0, g0, self.o)
        st.gd = dot(st.g, st.g, self.long)
        return st

    def accept(self, st, x, f, g, rec):
        """The point (x, f, g) is accepted from st: the pair, the new direction, the rules.  Returns (code or 0, the five quantities)."""
        L = self.long
        s, y = x - st.x, st.g - g
        sy, yy, ss = dot(s, y, L), dot(y, y, L), dot(s, s, L)
        if rec.positive(sy, float(np.abs(s) @ np.abs(y)), "s'y"):
            st.S.append(s)
            st.Y.append(y)
            if len(st.S) > self.m:                          # the ring wraps: the oldest pair leaves
                st.S.pop(0)
                st.Y.pop(0)
            st.gamma = sy / yy
        else:
            rec.branches.append("skipped_pair")
        df, fprev = abs(f - st.f), st.f
        st.x, st.f, st.g, st.it = np.array(x), float(f), np.array(g), st.it + 1
        gg = dot(st.g, st.g, L)
        st.d, st.T = two_loop(st.g, st.S, st.Y, st.gamma, L, absolute=True)
        gd = dot(st.g, st.d, L)
        if not (rec.positive(gd, float(np.abs(st.g) @ np.abs(st.d)), "g'Hg") and math.isfinite(gd)):
            rec.branches.append("history_reset")
            st.S, st.Y = [], []
            st.d, st.T, gd = st.g.copy(), np.abs(st.g), gg
        st.gd = gd
        tol_obj = self.o["tol_obj"]
        q = dict(absf=df, relf=df / max(abs(st.f), abs(fprev), tol_obj), absgrad=math.sqrt(gg), relgrad=gd / max(abs(st.f), tol_obj), absx=math.sqrt(ss))
        code = 0
        for c, name in enumerate(RULES, start=1):
            thr = self.thresholds()[name]
            if thr > 0.0 and rec.less(q[name], thr, name):
                code = c
                break
        if not code and st.it >= self.o["iter"]:
            code = MAXIT
        return code, q

    def derivative_error(self, st):
        """dd for `search`: (2 m + 5) DEPTH eps sum |g_t,i| T_i -- the dot product's own rounding and that of the direction's entries."""
        k = (2 * self.m + 5) * depth(st.x.size) * EPS
        return lambda gt: k * float(np.abs(gt) @ st.T)

    def iterate(self, st, errors=False):
        """One iteration from st: the search (twice where it is repeated along the gradient).  Does not change st.  Returns the record."""
        rec = Rec()
        out = dict(rec=rec, evals=0, history=st.history())
        d, T, gd0 = st.d, st.T, st.gd
        first = self.o["init_alpha"] if st.it == 0 else 1.0
        retried = False
        while True:
            ls = search(self.fun, st.x, st.f, d, gd0, first, rec, self.long, self.derivative_error(st) if errors else None)
            out["evals"] += ls["evals"]
            out.setdefault("first_trial", ls["trials"][0])
            if ls["ok"]:
                break
            if st.history() and not retried:               # once more, along the gradient, with an empty history
                rec.branches.append("retry_gradient")
                retried = True
                st = _without_history(st)
                d, T, gd0 = st.g, np.abs(st.g), dot(st.g, st.g, self.long)
                continue
            out.update(ok=False, retried=retried)
            return out
        out.update(ok=True, retried=retried, alpha=ls["alpha"], alpha_err=ls["alpha_err"], x=ls["x"], f=ls["f"], g=ls["g"], dh=ls["dh"], d=d, T=T,
                   gd0=gd0, search_evals=ls["evals"])
        return out

    def run(self, x0, errors=False):
        """The whole path.  Returns code, iterations, evals, the accepted x, f, g and one record per iteration."""
        x0 = np.asarray(x0, dtype=np.float64)
        f0, g0 = self.fun(x0)
        if not (np.isfinite(f0) and np.isfinite(g0).all()):
            return dict(code=INIT, iterations=0, evals=1, x=[x0], f=[f0], g=[g0], steps=[])
        st = self.start(x0, f0, g0)
        res = dict(x=[st.x], f=[st.f], g=[st.g], steps=[], evals=1)
        if st.gd == 0.0:
            return dict(res, code=ABSGRAD, iterations=0)
        budget = INIT_ATTEMPTS + (LS_MAX + 1) * int(self.o["iter"])     # passes of the launch, whatever the data
        while True:
            step = self.iterate(st, errors)
            res["evals"] += step["evals"]
            res["steps"].append(step)
            if not step["ok"]:
                return dict(res, code=LSFAIL, iterations=st.it)
            if step["retried"]:
                st = _without_history(st)
            code, q = self.accept(st, step["x"], step["f"], step["g"], step["rec"])
            step.update(rules=q, code=code)
            res["x"].append(st.x)
            res["f"].append(st.f)
            res["g"].append(st.g)
            if code:
                return dict(res, code=code, iterations=st.it)
            if res["evals"] >= budget:
                return dict(res, code=MAXIT, iterations=st.it)


def _without_history(st):
    s2 = State(st.x, st.f, st.g, st.o)
    s2.gamma, s2.it = st.gamma, st.it
    return s2


def replay(fun, xs, fs, gs, L, long=False, searches=True, **opts):
    """One reference iteration from each state of a recorded trajectory: for l < L the state is what x_0..x_l, g_0..g_l define (the pairs
    that were kept, the newest history_size of them), the reference performs iteration l from it and the next state is again taken from the
    record, not from the reference.  Returns a list of dicts: the record of iteration l (`step`, with the predicted x), and the rule quantities
    and the code of accepting the RECORDED point l + 1 (`rules`, `code`, `accept_rec`).  searches = False: the rules alone, no evaluation
    (a search repeated along the gradient, which empties the history, would then go unnoticed: the replay with searches is where it shows)."""
    ref = LBFGS(fun, long, **opts)
    st = ref.start(xs[0], fs[0], gs[0])
    out = []
    for l in range(L):
        step = ref.iterate(st, errors=True) if searches else dict(d=st.d, gd0=st.gd, history=st.history())
        if step.get("retried"):
            st = _without_history(st)
        rec = Rec()
        code, q = ref.accept(st, xs[l + 1], fs[l + 1], gs[l + 1], rec)
        out.append(dict(step=step, rules=q, code=code, accept_rec=rec))
    return out


def wolfe(f0, gd0, alpha, f1, dh):
    """(sufficient increase, curvature) of a step of length alpha with value f1 and derivative dh along the direction."""
    return f1 >= f0 + C1 * alpha * gd0, abs(dh) <= C2 * gd0


# ------------------------------------------------------------------------------------------------ the inputs both test modules use
ITER = 40
HISTORIES = (1, 2, 5, 20)
INIT_ALPHAS = (1e-3, 1.0, 100.0)
SINGLE = dict(absf=dict(tol_obj=0.1), relf=dict(tol_rel_obj=1e10), absgrad=dict(tol_grad=2.0), relgrad=dict(tol_rel_grad=1e10), absx=dict(tol_param=0.05))


def designs():
    """name -> (data, variant).  `wide`: the smallest shape whose D (805 full, 697 no-mode) exceeds the 512 threads of the workgroup and is no
    multiple of them, so every strided loop of the optimiser makes two trips, the second with a ragged tail."""
    from us_potus_model_amd import synthetic
    out = {}
    for v, tag in (("full", "full"), ("no_mode_adjustment", "nomode")):
        out[f"small_{tag}"] = (synthetic.small(v), v)
        out[f"wide_{tag}"] = (synthetic.make(seed=3, S=6, T=100, N_state=60, N_national=20, P=5, variant=v), v)
    return out


def default_starts(D):
    """The four starts of tests/test_gpu_optimize.py's `small` fixture, whose run under the defaults is held to the reference's code and count."""
    return np.vstack([np.zeros(D), np.random.default_rng(20161108).uniform(-2, 2, (3, D))])


FLIP = dict(design="small_nomode", history_size=5, init_alpha=1.0)      # with flip_start: zoom_near_flip in iteration 0 (found by a search of
                                                                        # 72 starts x 3 radii on the CPU oracle; the first of 15 that reach it)

def flip_start(D):
    return np.random.default_rng(114).uniform(-2, 2, D)


def starts(D):
    """Two starts per design: U(-1, 1) and U(-2, 2)."""
    q = np.stack([np.random.default_rng(1).uniform(-1, 1, D), np.random.default_rng(2).uniform(-2, 2, D)])
    q.setflags(write=False)
    return q
