"""What tests/test_poll_terms_host.py and tests/test_gpu_poll_terms.py share: the committed 40 - 60 digit results of the per-poll binomial terms
(tests/golden/poll_terms.npz), the generator that wrote them (scripts/make_golden_poll_terms.py, which also builds the tail designs), and the
rounding level of a straightforward double evaluation against them."""
import importlib.util
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent

# e_orc: the largest |g_oracle,i - g_ref,i| / A_i (|lp_oracle - lp_ref| / A_lp) over the 24 tail points, oracle in its literal and its fast form
# against the 60-digit values; measured on the CPU (test_poll_terms_host.py asserts it): gradient 6.45e-12, log density 5.74e-16.  The gradient's
# figure is one cancellation, not a sum's length: the residual r = y - n p of a saturated poll with y = n (eta = +37.5: 1 - p = 5e-17 is below the
# spacing of p at 1) is formed as n - n = 0 where it is 3.6e-14, and sigma r = 9e-13 stands against A_i = |q_i| + sigma |r| = 1.5.  A_i counts |r|,
# not y + n p, so this loss shows; every form that computes r by that subtraction shares it.  The device is allowed 16 e_orc: four bits for
# its other summation orders (sixteen members, DPP trees, L (a z) for (a L) z).  A wrong or dropped term is of order A_i.
E_ORC_GRAD = 6.5e-12
E_ORC_LP = 5.8e-16
DEVICE_FACTOR = 16.0

_GEN = None


def gen():
    """scripts/make_golden_poll_terms.py as a module (mpmath is imported only by the functions that compute)."""
    global _GEN
    if _GEN is None:
        spec = importlib.util.spec_from_file_location("make_golden_poll_terms", ROOT / "scripts" / "make_golden_poll_terms.py")
        _GEN = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_GEN)
    return _GEN


_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        with np.load(ROOT / "tests" / "golden" / "poll_terms.npz") as f:
            _FIX = {k: f[k] for k in f.files}
    return _FIX


def design_names():
    return list(gen().DESIGNS)


def design(name):
    """(data, variant, q [6, D], lp [6], g [6, D], A_lp [6], A [6, D]) of a tail design; the design is rebuilt and must be the one the fixture was
    computed on."""
    F = fixture()
    data, variant = gen().tail_design(name)
    for kind in ("state", "national"):
        for k in ("n_two_share", "n_democrat", "day"):
            assert np.array_equal(np.asarray(data[f"{k}_{kind}"]), F[f"{name}_{k}_{kind}"]), (name, k, kind)
    q = gen().tail_points(data, variant)
    assert np.array_equal(q, F[f"{name}_q"]), name
    return data, variant, q, F[f"{name}_lp"], F[f"{name}_g"], F[f"{name}_A_lp"], F[f"{name}_A"]


def scaled_errors(lp, g, ref_lp, ref_g, A_lp, A):
    """(|lp - ref| / A_lp, max_i |g_i - ref_i| / A_i); a coordinate with A_i = 0 (its poll has n = 0 and its own value is 0) must be exact."""
    d = np.abs(np.asarray(g) - ref_g)
    assert np.isfinite(lp) and np.isfinite(g).all()
    assert (d[A == 0] == 0).all()
    return abs(lp - ref_lp) / A_lp, float((d[A > 0] / A[A > 0]).max())
