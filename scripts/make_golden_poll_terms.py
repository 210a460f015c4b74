#!/usr/bin/env python3
"""Generate tests/golden/poll_terms.npz: the binomial-logit term of a poll over its whole domain, by mpmath at 40 - 60 digits.

Run by hand (needs mpmath):  python scripts/make_golden_poll_terms.py

Two parts (tests/test_poll_terms_host.py pins the oracle to them and recomputes a sample; tests/test_gpu_poll_terms.py holds the kernels to them):

  ll grid       log p(y | n, eta, sigma) without log C(n, y): the noise coordinate integrated over its N(0, 1) prior, and the plain value at
                z in LL_Z, over sigma x n x y x (eta - empirical logit); plain-only tail cells at |eta| up to 800.  The integral's mode comes from
                bisection on the strictly decreasing f'; the quadrature (tanh-sinh) is split at the mode, at +-3, +-10, +-40 around it (f is
                below f(mode) - (z - mode)^2 / 2, so +-40 leaves e^-800) and at +-3, +-10, +-40 standard deviations of the integrand.
  tail designs  two small synthetic designs in both variants with sigma_measure_noise_* = 25, counts edited to y = 0, y = n, n = 0,
                n = 2 000 000 and n = 61 771 on day 1 and day T among state and national polls, and six points each whose noise
                coordinates put |eta| anywhere from 0 to 800: log density and gradient (central differences at 60 digits, h = 1e-25),
                and the magnitudes A_lp = sum |terms|, A_i = sum |contributions to g_i| that rounding errors scale with.

The mpmath model is written statement by statement from poll_model_2020.stan / its no_mode_adjustment variant, like tests/stan_transcription.py;
`~` statements drop constants, Jacobians follow the Stan reference manual (lower = 0, upper = 1: log_inv_logit(x) + log_inv_logit(-x)).
mpmath is imported lazily: the design builders are used by tests that run without it.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "poll_terms.npz"

LL_SIGMA = (0.0, 0.02, 0.04, 0.1, 0.3)
LL_N = (0, 3, 100, 1000, 5000, 61771, 100000)
LL_OFF = (0.0, 0.3, -1.0, 2.5, 3.0, -6.0)
LL_Z = (-3.0, 0.0, 2.0)
TAIL_ETA = (36.0, 37.5, 40.0, 700.0, 745.2, 746.0, 800.0)
TAIL_N = (100, 100000)
NOISE_T = (0.0, 1e-3, -1e-3, .5, -.5, 5.0, -5.0, 17.0, -17.0, 36.0, -36.0, 37.5, -37.5, 40.0, -40.0, 700.0, -700.0, 745.2, -745.2, 746.0, -746.0,
           800.0, -800.0)
NOISE_SIGMA = 25.0
N_POINTS = 6
BUCKETS = ((0.0, 1.0), (15.0, 20.0), (30.0, 40.0), (40.0, 100.0), (600.0, 745.0), (746.0, np.inf))
DESIGNS = {"s6_full": (6, "full"), "s6_nomode": (6, "no_mode_adjustment"), "s1_full": (1, "full"), "s1_nomode": (1, "no_mode_adjustment")}
EDIT_COUNTS = ("y0", "yn", "n0", "n2e6", "n61771")


# ------------------------------------------------------------------------------------------------ inputs (no mpmath)
def ll_cells():
    """(sigma, n, y, eta, off) of every cell of the grid, as float64 arrays."""
    rows = []
    for sigma in LL_SIGMA:
        for n in LL_N:
            for y in sorted({0, int(round(.03 * n)), int(round(n / 2)), n}):
                for off in LL_OFF:
                    rows.append((sigma, float(n), float(y), float(np.log((y + .5) / (n - y + .5)) + off), off))
    return [np.array(c) for c in zip(*rows)]


def tail_cells():
    """(n, y, eta) of the plain-only tail cells."""
    rows = [(float(n), float(y), s * e) for n in TAIL_N for y in (0, n // 2, n) for e in TAIL_ETA for s in (1.0, -1.0)]
    return [np.array(c) for c in zip(*rows)]


def edit_counts(counts, n, y, day, T):
    """Edit the first 2 * len(counts) polls of one kind in place: each count once on day 1 and once on day T."""
    for k, what in enumerate(counts):
        for j, d in enumerate((1, T)):
            i = 2 * k + j
            day[i] = d
            if what == "y0": y[i] = 0
            elif what == "yn": y[i] = n[i]
            elif what == "n0": n[i] = 0; y[i] = 0
            elif what == "n2e6": n[i] = 2_000_000; y[i] = 1_037_311
            elif what == "n61771": n[i] = 61_771; y[i] = 29_403
    return 2 * len(counts)


def tail_design(name):
    """(data, variant) of a tail design: synthetic.make(seed = 3) with sigma_measure_noise_* = 25 and the edited counts."""
    from us_potus_model_amd import synthetic
    S, variant = DESIGNS[name]
    data = synthetic.make(seed=3, S=S, T=24, N_state=70, N_national=25, P=9, variant=variant)
    data["sigma_measure_noise_state"] = data["sigma_measure_noise_national"] = NOISE_SIGMA
    for kind in ("state", "national"):
        n, y, day = (np.array(data[f"{k}_{kind}"]) for k in ("n_two_share", "n_democrat", "day"))
        edit_counts(EDIT_COUNTS, n, y, day, int(data["T"]))
        data[f"n_two_share_{kind}"], data[f"n_democrat_{kind}"], data[f"day_{kind}"] = n, y, day
    return data, variant


def noise_cycle(n_noise, point, stride=1):
    """raw_measure_noise_* of one point: t_i / 25 with t_i cycling through NOISE_T, shifted by the point."""
    k = (stride * np.arange(n_noise) + 4 * point) % len(NOISE_T)
    return np.asarray(NOISE_T)[k] / NOISE_SIGMA


def layout(data, variant):
    """Offsets of the parameter blocks in declaration order (stan:56-69)."""
    full = variant == "full"
    S, T, P = int(data["S"]), int(data["T"]), int(data["P"])
    sizes = [("raw_mu_b_T", S), ("raw_mu_b", S * T), ("raw_mu_c", P)]
    if full:
        sizes += [("raw_mu_m", int(data["M"])), ("raw_mu_pop", int(data["Pop"])), ("mu_e_bias", 1), ("rho_e_bias", 1), ("raw_e_bias", T)]
    sizes += [("raw_measure_noise_national", int(data["N_national_polls"])), ("raw_measure_noise_state", int(data["N_state_polls"])), ("raw_polling_bias", S)]
    out, o = {}, 0
    for k, n in sizes:
        out[k] = (o, o + n)
        o += n
    return out, o


def tail_points(data, variant, seed=13):
    """[N_POINTS, D]: noise coordinates from noise_cycle, rho_e_bias's coordinate uniform(-5, 5), everything else uniform(-2, 2).  (The seed is the
    first from 11 on with which check_buckets holds for all four designs: eta's other terms decide on which side of 40 a poll with t = +-40 falls.)"""
    lay, D = layout(data, variant)
    rng = np.random.default_rng(seed)
    q = rng.uniform(-2, 2, (N_POINTS, D))
    a, b = lay["raw_measure_noise_national"][0], lay["raw_measure_noise_state"][1]
    for i in range(N_POINTS):
        q[i, a:b] = noise_cycle(b - a, i)
        if "rho_e_bias" in lay:
            q[i, lay["rho_e_bias"][0]] = rng.uniform(-5, 5)
    return q


# ------------------------------------------------------------------------------------------------ mpmath
def _mp(dps):
    import mpmath
    mpmath.mp.dps = dps
    return mpmath


def mp_plain(y, n, x, dps=40):
    """y x - n softplus(x)."""
    mp = _mp(dps)
    y, n, x = mp.mpf(y), mp.mpf(n), mp.mpf(x)
    return y * x - n * (max(x, mp.mpf(0)) + mp.log1p(mp.exp(-abs(x))))


def mp_mode(y, n, eta, sigma, dps=40):
    """Root of the strictly decreasing f'(z) = sigma (y - n inv_logit(eta + sigma z)) - z by bisection on [sigma (y - n), sigma y]."""
    mp = _mp(dps)
    y, n, eta, sigma = mp.mpf(y), mp.mpf(n), mp.mpf(eta), mp.mpf(sigma)
    df = lambda z: sigma * (y - n / (1 + mp.exp(-(eta + sigma * z)))) - z
    a, b = sigma * (y - n), sigma * y
    for _ in range(int(3.33 * dps) + 70):
        m = (a + b) / 2
        if df(m) > 0: a = m
        else: b = m
    return (a + b) / 2


def mp_integrated(y, n, eta, sigma, dps=40):
    """log int exp(y x - n softplus(x)) phi(z) dz, x = eta + sigma z."""
    mp = _mp(dps)
    if sigma == 0:
        return mp_plain(y, n, eta, dps)
    m = mp_mode(y, n, eta, sigma, dps)
    ys, ns, es, ss = mp.mpf(y), mp.mpf(n), mp.mpf(eta), mp.mpf(sigma)
    f = lambda z: mp_plain(ys, ns, es + ss * z, dps) - z * z / 2
    f0 = f(m)
    p = 1 / (1 + mp.exp(-(es + ss * m)))
    sd = 1 / mp.sqrt(ss * ss * ns * p * (1 - p) + 1)
    pts = {m} | {m + s * k for k in (3, 10, 40) for s in (1, -1)} | {m + s * k * sd for k in (3, 10, 40) for s in (1, -1)}
    v = mp.quad(lambda z: mp.exp(f(z) - f0), sorted(pts))
    return f0 + mp.log(v) - mp.log(2 * mp.pi) / 2


class MpModel:
    """The Stan program on mpmath numbers: transformed data once, log_prob(q) per point."""

    def __init__(self, data, variant, dps=60):
        mp = self.mp = _mp(dps)
        self.dps = dps
        f = self.f = lambda v: mp.mpf(float(v))
        self.full = variant == "full"
        d = self.d = data
        S = self.S = int(d["S"]); self.T = int(d["T"]); self.P = int(d["P"])
        self.Nn, self.Ns = int(d["N_national_polls"]), int(d["N_state_polls"])
        self.M, self.Pop = (int(d["M"]), int(d["Pop"])) if self.full else (0, 0)
        w = self.w = [f(v) for v in np.asarray(d["state_weights"]).reshape(-1)]
        cov = [[f(v) for v in row] for row in np.asarray(d["state_covariance_0"], dtype=float).reshape(S, S)]
        nsd = mp.sqrt(sum(w[i] * cov[i][j] * w[j] for i in range(S) for j in range(S)))            # stan:42-55

        def chol(scale):
            c = (f(scale) / nsd) ** 2
            L = [[mp.mpf(0)] * S for _ in range(S)]
            for i in range(S):
                for j in range(i + 1):
                    s = cov[i][j] * c - sum(L[i][k] * L[j][k] for k in range(j))
                    L[i][j] = mp.sqrt(s) if i == j else s / L[j][j]
            return L
        self.L_pb, self.L_T, self.L_W = chol(d["polling_bias_scale"]), chol(d["mu_b_T_scale"]), chol(d["random_walk_scale"])
        self.prior = [f(v) for v in d["mu_b_prior"]]

    def _mv(self, L, x):
        return [sum(L[i][k] * x[k] for k in range(i + 1)) for i in range(self.S)]

    def eta(self, q):
        """(eta_state, eta_national, rho_e_bias, mu_e_bias) at the mpf list q (stan:70-113)."""
        mp, d, f, S, T = self.mp, self.d, self.f, self.S, self.T
        o = [0]

        def take(n):
            v = q[o[0]:o[0] + n]
            o[0] += n
            return v
        zT, Z, zc = take(S), take(S * T), take(self.P)
        rho = mue = None
        if self.full:
            zm, zpop = take(self.M), take(self.Pop)
            mue, xr, ze = mp.mpf("0.02") * take(1)[0], take(1)[0], take(T)
            rho = 1 / (1 + mp.exp(-xr))
        znn, zns, zpb = take(self.Nn), take(self.Ns), take(S)
        assert o[0] == len(q)
        pb = self._mv(self.L_pb, zpb)
        nat_pb = sum(a * b for a, b in zip(pb, self.w))
        mu_b = [None] * T
        mu_b[T - 1] = [a + b for a, b in zip(self._mv(self.L_T, zT), self.prior)]
        for i in range(1, T):
            t = T - 1 - i
            mu_b[t] = [a + b for a, b in zip(self._mv(self.L_W, Z[S * t:S * t + S]), mu_b[t + 1])]   # raw_mu_b is column-major S x T
        nat_avg = [sum(a * b for a, b in zip(col, self.w)) for col in mu_b]
        mu_c = [v * f(d["sigma_c"]) for v in zc]
        if self.full:
            mu_m, mu_pop = [v * f(d["sigma_m"]) for v in zm], [v * f(d["sigma_pop"]) for v in zpop]
            se = f(d["sigma_e_bias"])
            sr = mp.sqrt(1 - rho ** 2) * se
            e = [ze[0] * se]
            for t in range(1, T):
                e.append(mue + rho * (e[t - 1] - mue) + ze[t] * sr)
        out = []
        for kind, z, sig in (("state", zns, d["sigma_measure_noise_state"]), ("national", znn, d["sigma_measure_noise_national"])):
            ev = []
            for j in range(len(z)):
                t = int(d[f"day_{kind}"][j]) - 1
                if kind == "state":
                    s = int(d["state"][j]) - 1
                    x = mu_b[t][s]
                else:
                    x = nat_avg[t]
                x = x + mu_c[int(d[f"poll_{kind}"][j]) - 1]
                if self.full:
                    x = x + mu_m[int(d[f"poll_mode_{kind}"][j]) - 1] + mu_pop[int(d[f"poll_pop_{kind}"][j]) - 1] + f(d[f"unadjusted_{kind}"][j]) * e[t]
                x = x + z[j] * f(sig) + (pb[s] if kind == "state" else nat_pb)
                ev.append(x)
            out.append(ev)
        return out[0], out[1], rho, mue

    def terms(self, q):
        """Every additive term of the log density at q (floats or mpf), in no particular order (stan:115-132 and the Jacobians)."""
        mp = self.mp
        q = [mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v for v in q]
        es, en, rho, mue = self.eta(q)
        lay, D = layout(self.d, "full" if self.full else "no_mode_adjustment")
        skip = {lay[k][0] for k in ("mu_e_bias", "rho_e_bias")} if self.full else set()
        t = [-v * v / 2 for i, v in enumerate(q) if i not in skip]
        if self.full:
            xr = q[lay["rho_e_bias"][0]]
            lil = lambda x: -mp.log1p(mp.exp(-x))
            t += [mp.log(mp.mpf("0.02")), lil(xr) + lil(-xr), -((mue / mp.mpf("0.02")) ** 2) / 2, -(((rho - mp.mpf("0.7")) / mp.mpf("0.1")) ** 2) / 2]
        for kind, ev in (("state", es), ("national", en)):
            for j, x in enumerate(ev):
                t.append(mp_plain(int(self.d[f"n_democrat_{kind}"][j]), int(self.d[f"n_two_share_{kind}"][j]), x, self.dps))
        return t

    def log_prob(self, q):
        return self.mp.fsum(self.terms(q))

    def grad(self, q, h="1e-25", coords=None):
        """Central differences at the working precision."""
        mp = self.mp
        q = [mp.mpf(float(v)) for v in q]
        h = mp.mpf(h)
        g = []
        for i in (range(len(q)) if coords is None else coords):
            qi = q[i]
            q[i] = qi + h; a = self.log_prob(q)
            q[i] = qi - h; b = self.log_prob(q)
            q[i] = qi
            g.append((a - b) / (2 * h))
        return g


def magnitudes(data, variant, q):
    """A_lp = sum |terms| and A_i = sum of the magnitudes of every contribution to g_i: |q_i| of the coordinate's own normal term, |r_p| |d eta_p / d q_i| of
    every poll, and for mu_e_bias / rho_e_bias the magnitudes of their prior and Jacobian terms.  Bounds, not values: double precision, the
    Jacobian of eta by autograd on tests/stan_transcription.py."""
    import torch
    sys.path.insert(0, str(ROOT / "tests"))
    import stan_transcription
    qt = torch.tensor(np.asarray(q, dtype=np.float64), requires_grad=True)
    lay, D = layout(data, variant)
    eta = lambda x: torch.cat([stan_transcription.log_prob(data, x, variant)[1][k] for k in ("eta_s", "eta_n")])
    J = torch.autograd.functional.jacobian(eta, qt).numpy()
    e = eta(qt).detach().numpy()
    y = np.concatenate([np.asarray(data["n_democrat_state"], float), np.asarray(data["n_democrat_national"], float)])
    n = np.concatenate([np.asarray(data["n_two_share_state"], float), np.asarray(data["n_two_share_national"], float)])
    ex = np.exp(-np.abs(e))
    r = y - n * np.where(e >= 0, 1.0, ex) / (1.0 + ex)
    A = np.abs(r) @ np.abs(J) + np.abs(q)
    l1 = np.log1p(ex)
    A_lp = np.sum(np.abs(y * (np.minimum(e, 0) - l1)) + np.abs((n - y) * (np.minimum(-e, 0) - l1))) + np.sum(0.5 * np.asarray(q) ** 2)
    if variant == "full":
        x = q[lay["rho_e_bias"][0]]
        rho = 1.0 / (1.0 + np.exp(-x))
        A[lay["rho_e_bias"][0]] += abs(1 - 2 * rho) + abs((rho - 0.7) / 0.01 * rho * (1 - rho)) - abs(x)
        A_lp += abs(np.log(0.02)) + abs(np.log(rho) + np.log1p(-rho)) + 0.5 * ((rho - 0.7) / 0.1) ** 2 - 0.5 * x * x
    return float(A_lp), A, e, y, n


def check_buckets(name, etas, y, n):
    """Every bucket of |eta| is hit by a poll with y = 0, one with 0 < y < n and one with y = n (n > 0), over the points of a design."""
    a = np.abs(etas)
    for cls, sel in (("y = 0", (y == 0) & (n > 0)), ("0 < y < n", (y > 0) & (y < n)), ("y = n", (y == n) & (n > 0))):
        for lo, hi in BUCKETS:
            assert ((a[:, sel] > lo) & (a[:, sel] < hi)).any(), f"{name}: no poll with {cls} has |eta| in ({lo}, {hi})"


def _ll_job(c):
    sigma, n, y, eta = c
    return float(mp_integrated(y, n, eta, sigma)), [float(mp_plain(y, n, _mp(40).mpf(eta) + _mp(40).mpf(sigma) * _mp(40).mpf(z))) for z in LL_Z]


def _point_job(a):
    name, i = a
    data, variant = tail_design(name)
    q = tail_points(data, variant)[i]
    m = MpModel(data, variant)
    return name, i, float(m.log_prob(q)), np.array([float(v) for v in m.grad(q)])


def main():
    import multiprocessing as mpc
    out = {}
    sigma, n, y, eta, off = ll_cells()
    with mpc.Pool() as pool:
        res = pool.map(_ll_job, list(zip(sigma, n, y, eta)), chunksize=8)
        out.update(ll_sigma=sigma, ll_n=n, ll_y=y, ll_eta=eta, ll_off=off, ll_z=np.array(LL_Z),
                   ll_integrated=np.array([r[0] for r in res]), ll_plain=np.array([r[1] for r in res]))
        tn, ty, te = tail_cells()
        out.update(tail_n=tn, tail_y=ty, tail_eta=te, tail_plain=np.array([float(mp_plain(a, b, c)) for a, b, c in zip(ty, tn, te)]))
        print(f"ll grid: {len(sigma)} cells, {len(tn)} tail cells", flush=True)
        jobs = [(name, i) for name in DESIGNS for i in range(N_POINTS)]
        pts = {(name, i): (lp, g) for name, i, lp, g in pool.map(_point_job, jobs, chunksize=1)}
    for name in DESIGNS:
        data, variant = tail_design(name)
        q = tail_points(data, variant)
        mags = [magnitudes(data, variant, q[i]) for i in range(N_POINTS)]
        check_buckets(name, np.array([m[2] for m in mags]), mags[0][3], mags[0][4])
        out[f"{name}_q"] = q
        out[f"{name}_lp"] = np.array([pts[name, i][0] for i in range(N_POINTS)])
        out[f"{name}_g"] = np.array([pts[name, i][1] for i in range(N_POINTS)])
        out[f"{name}_A_lp"] = np.array([m[0] for m in mags])
        out[f"{name}_A"] = np.array([m[1] for m in mags])
        for kind in ("state", "national"):                       # the edited counts, so that a test can tell a design that moved
            for k in ("n_two_share", "n_democrat", "day"):
                out[f"{name}_{k}_{kind}"] = np.asarray(data[f"{k}_{kind}"], dtype=np.int32)
        print(name, "D", q.shape[1], "lp", out[f"{name}_lp"], flush=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    main()
