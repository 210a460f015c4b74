"""tests/pathfinder_ref.py against itself, without a GPU: the dense and the low-rank form of Pathfinder's normal approximation agree on paths
over a strongly concave quadratic, Sigma_l satisfies the secant equations of its history, and where the ELBO's argmax lies on such a path.

Bounds.  Both forms are backward-stable dense algebra on the same inputs; they differ by the conditioning of what each inverts.  The dense
form solves with Sigma (kappa(Sigma) <= kappa(H) * kappa(alpha) here, H of condition 100): relative forward error of order D eps kappa.  The
tests use D = 40, kappa <= 1e4 in the worst case built here, so D eps kappa = 1e-10 relative; the asserted 1e-8 leaves two digits for the
constants of the two factorisations (QR + Cholesky against slogdet + solve)."""
import numpy as np
import pytest

import pathfinder_ref as pref

D, L, J = 40, 9, 4
RTOL = 1e-8


def _scale(v):
    return max(1.0, float(np.abs(v).max()))


def compare_forms(p, l, u):
    ak = pref.alphas(p["x"], p["g"])
    a, b = pref.dense(p["x"], p["g"], l, J, u=u, al_kept=ak), pref.low_rank(p["x"], p["g"], l, J, u=u, al_kept=ak)
    assert a["hist"] == b["hist"]
    for k in ("mu", "phi", "lq"):
        assert np.abs(a[k] - b[k]).max() <= RTOL * _scale(a[k]), (k, l, np.abs(a[k] - b[k]).max())
    assert abs(a["log_det"] - b["log_det"]) <= RTOL * _scale(np.array([a["log_det"]])), (l, a["log_det"], b["log_det"])
    return a


@pytest.mark.parametrize("case", ["plain", "rejected", "repeated"])
def test_the_two_forms_agree(case):
    rng = np.random.default_rng(5)
    p = pref.quadratic_path(rng, D, L, reject=4 if case == "rejected" else None, repeat=5 if case == "repeated" else None)
    _, kept, _ = pref.alphas(p["x"], p["g"])
    if case == "rejected":
        assert not kept[4]
    if case == "repeated":
        assert not kept[5]                                          # s = 0: s'z > 0 fails
    u = rng.standard_normal((3, D))
    sizes = set()
    for l in range(1, L + 1):
        sizes.add(len(compare_forms(p, l, u)["hist"]))
    assert {1, 2, 3, J} <= sizes                                    # j < J on the way up, then the oldest pair drops out


def test_no_kept_pair_is_the_diagonal():
    rng = np.random.default_rng(6)
    p = pref.quadratic_path(rng, D, 2)
    p["g"][1] = p["g"][0] + (p["g"][0] - p["g"][1])                 # the only pair up to l = 1 has s'z < 0
    u = rng.standard_normal((2, D))
    a = compare_forms(p, 1, u)
    assert a["hist"] == [] and np.array_equal(a["alpha"], np.ones(D))
    assert np.array_equal(a["Sigma"], np.eye(D)) and np.allclose(a["phi"], p["x"][1] + p["g"][1] + u, rtol=0, atol=1e-13 * _scale(a["phi"]))


def test_secant_equations():
    """Sigma_l z_i = s_i for the NEWEST pair i of the history, to rounding at kappa(Sigma): the defining property of the inverse BFGS update,
    whatever the diagonal.  For the older pairs of the history the equation is no property of BFGS (a later update keeps an earlier secant
    equation only under exact line searches on a quadratic, which these paths do not make): their residual is printed, of order |s|."""
    rng = np.random.default_rng(7)
    p = pref.quadratic_path(rng, D, L)
    for l in (1, 3, L):
        r = pref.dense(p["x"], p["g"], l, J)
        for i in r["hist"]:
            s, z = p["x"][i] - p["x"][i - 1], p["g"][i - 1] - p["g"][i]
            res = np.abs(r["Sigma"] @ z - s).max()
            print(f"l = {l}, pair {i}: |Sigma z - s| = {res:.3g}, |s| = {np.abs(s).max():.3g}")
            if i == r["hist"][-1]:
                assert res <= RTOL * _scale(s), (l, i)
        assert np.array_equal(r["Sigma"], r["Sigma"].T) and np.linalg.eigvalsh(r["Sigma"]).min() > 0.0


def test_where_the_elbo_peaks_on_a_quadratic():
    """On a quadratic the target IS normal, so the expectation was an ELBO that rises to the end of the path.  What the test finds (D = 12,
    J = 6, 60 steps, K = 200 draws, the same u at every iterate): the ELBO climbs by ~57 nats over the first ~10 iterates and then sits on
    a plateau within ~1.5 nats of the optimum log Z -- a history of J = 6 pairs cannot hold the 12 x 12 Hessian, so each iterate's
    Sigma is good in the last six directions searched only -- and the argmax is SOMEWHERE on the plateau (iterate 49 of 60 with this
    seed), not at the end.  So the assertion is the plateau: past the climb every ELBO, the last one included, is within 3 nats of the maximum
    and no ELBO exceeds log Z = D/2 log 2 pi - 1/2 log det H by more than the Monte Carlo error."""
    rng = np.random.default_rng(8)
    d, steps, K = 12, 60, 200
    p = pref.quadratic_path(rng, d, steps, cond=20.0)
    u = np.broadcast_to(rng.standard_normal((K, d)), (steps, K, d))
    e = pref.elbo(pref.low_rank, p["log_p"], p["x"], p["g"], 6, u)
    lstar = pref.best(e)
    log_z = 0.5 * d * pref.LOG_2PI - 0.5 * np.linalg.slogdet(p["H"])[1]
    print("ELBO along the path:", np.array2string(e[1:], precision=2), "argmax", lstar, "log Z", log_z)
    assert np.isfinite(e[1:]).all()
    assert e[1] < e[lstar] - 10.0 and lstar > 5
    assert (e[steps // 2:] >= e[lstar] - 3.0).all()
    assert e[lstar] <= log_z + 1.0
