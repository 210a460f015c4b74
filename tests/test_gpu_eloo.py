"""E_loo on the MI355X (potus_eloo.hpp) against its numpy restatement (tests/eloo_ref.py): the pointwise form on every
branch of its PSIS, diagnostic and quantile code, the shared form (the product on the matrix cores) at the edges of its tiles and chunks, the
bytes either form promises, and the refusals.  The bar is test_gpu_loo._close: relative 1e-8, infinities in the same places, no NaN."""
import ctypes as C

import numpy as np
import pytest

import eloo_ref as ref
from loo_mm_ref import psis_general
from test_gpu_loo import _close
from us_potus_model_amd import loo as loo_mod
from us_potus_model_amd.sampler import PotusError, load_library

pytestmark = pytest.mark.gpu
DP = C.POINTER(C.c_double)
PROBS = (0.05, 0.5, 0.95)
EL_CHUNK = 1024          # potus_eloo.hpp


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


def _ratios(rng, shape):
    """raw log ratios = minus the log-likelihoods of test_psis_branches_on_built_blocks"""
    return -(rng.normal(-3, 0.7, shape) + 0.3 * rng.standard_t(3, shape))


def _quantities(rng, shape, kind):
    if kind == "continuous":
        return rng.normal(0.3, 1.0, shape) + np.arange(shape[0])[:, None, None]
    if kind == "constant":
        return np.full(shape, 0.37)
    return (rng.random(shape) < 0.4).astype(float)


def _close_k(a, b):
    """_close, which has nothing to take a maximum of when every k is infinite"""
    if np.isfinite(b).any():
        _close(a, b)
    else:
        assert np.array_equal(a, b)


def _all(e):
    return np.concatenate([e.mean[:, None], e.variance[:, None], e.sd[:, None], e.quantiles], axis=1)


def _check_pointwise(x, r, r_eff):
    got = loo_mod.e_loo(_dev(x), _dev(r), "quantile", PROBS, r_eff)
    out, kh = ref.e_loo(x, r, PROBS, r_eff)
    _close(_all(got), out)
    _close_k(got.khat, kh)
    return got


@pytest.fixture(scope="module")
def built():
    """the six polls of test_psis_branches_on_built_blocks as ratios: poll 4's largest ratios are one value, poll 5's are identical"""
    rng = np.random.default_rng(3)
    ll = -_ratios(rng, (6, 4, 250))
    v = ll[4].reshape(-1)
    v[v < np.quantile(v, 0.3)] = np.quantile(v, 0.3)
    ll[5] = -1.25
    return -ll


@pytest.mark.parametrize("kind", ["continuous", "constant", "zero_one"])
@pytest.mark.parametrize("r_eff", [None, 1e-6, 1000.0], ids=["computed", "tail_0.2S", "tail_below_5"])
def test_pointwise_form_on_built_blocks(built, kind, r_eff):
    r = built
    x = _quantities(np.random.default_rng(21), r.shape, kind)
    re = None if r_eff is None else np.full(6, r_eff)
    got = _check_pointwise(x, r, re)
    if r_eff == 1e-6:
        assert ref.tail_length(r_eff, 1000) == 200 and np.isfinite(got.khat[:4]).all()
    if r_eff == 1000.0:
        assert np.isinf(got.khat).all()
    assert np.isinf(got.khat[4:]).all()
    if kind != "continuous":
        assert np.array_equal(got.khat[:, 0], got.khat[:, 2]) and np.array_equal(got.khat[:, 1], got.khat[:, 2])
    else:
        assert (got.khat[:4, 0] >= got.khat[:4, 2]).all()
    # poll 5 has equal weights: numpy's own quantile, mean and variance
    _close(got.quantiles[5], np.quantile(x[5].reshape(-1), PROBS))
    _close([got.mean[5], got.variance[5]], [x[5].mean(), x[5].var()])
    # the k of the ratios is potus_loo's pareto_k of the poll
    lo = loo_mod.loo_of_block(_dev(-r), r_eff=re)
    _close_k(got.khat[:, 2], lo.pareto_k)
    for t, col in (("mean", 0), ("variance", 1), ("sd", 1)):
        e = loo_mod.e_loo(_dev(x), _dev(r), t, None, re)
        assert e.pareto_k.tobytes() == got.khat[:, col].tobytes() and e.value.tobytes() == getattr(got, t).tobytes()


def test_pointwise_form_odd_size_zero_weights_and_more_than_one_sorted_run():
    rng = np.random.default_rng(4)
    r = _ratios(rng, (5, 3, 37))                           # S = 111: no multiple of 64 or of 4
    x = _quantities(rng, r.shape, "continuous")
    x[1] = np.round(x[1], 1)                               # ties in x
    _check_pointwise(x, r, None)
    r[2].reshape(-1)[rng.choice(111, 30, replace=False)] = -np.inf   # draws of weight 0 (a given r_eff: exp(-r) has none)
    got = _check_pointwise(x, r, np.full(5, 0.8))
    assert np.isfinite(_all(got)).all()
    r[3, 0, 5] = np.nan                                    # a poll that cannot be weighted: NaN, the others untouched
    bad = loo_mod.e_loo(_dev(x), _dev(r), "quantile", PROBS, np.full(5, 0.8))
    assert np.isnan(_all(bad)[3]).all() and np.isnan(bad.khat[3]).all()
    keep = [0, 1, 2, 4]
    assert _all(bad)[keep].tobytes() == _all(got)[keep].tobytes() and bad.khat[keep].tobytes() == got.khat[keep].tobytes()
    big = _ratios(rng, (3, 16, 1000))                      # 16 000 draws: two sorted runs
    _check_pointwise(_quantities(rng, big.shape, "continuous"), big, None)


def test_pointwise_form_repeats_its_bytes_and_a_poll_alone_has_its_bytes_of_the_batch(built):
    r = built
    x = _quantities(np.random.default_rng(22), r.shape, "continuous")
    a = loo_mod.e_loo(_dev(x), _dev(r), "quantile", PROBS)
    b = loo_mod.e_loo(_dev(x), _dev(r), "quantile", PROBS)
    assert _all(a).tobytes() == _all(b).tobytes() and a.khat.tobytes() == b.khat.tobytes()
    for i in (0, 3, 4, 5):
        one = loo_mod.e_loo(_dev(x[i:i + 1]), _dev(r[i:i + 1]), "quantile", PROBS)
        assert _all(one).tobytes() == _all(a)[i:i + 1].tobytes() and one.khat.tobytes() == a.khat[i:i + 1].tobytes()


# ---- the shared form
POLLS, COLS = (1, 15, 16, 17), (1, 15, 16, 17, 105)


def _shared_case(seed, chains, n, NP, NC):
    rng = np.random.default_rng(seed)
    r = _ratios(rng, (NP, chains, n))
    X = rng.normal(0.0, 1.0, (NC, chains, n)) * rng.uniform(0.1, 3.0, (NC, 1, 1)) + rng.normal(0, 2.0, (NC, 1, 1))
    X[min(2, NC - 1)] = 1e6 + rng.normal(0, 1.0, (chains, n))          # a huge offset: the uncentred variance has no digits left here
    if NC > 3:
        X[3] = (rng.random((chains, n)) < 0.3).astype(float)          # an indicator: its k is the k of the ratios
    re = np.array([ref.r_eff_of(r[i]) for i in range(NP)])
    lw = np.stack([psis_general(r[i], re[i])[0].reshape(chains, n) for i in range(NP)])
    return X, r, re, lw, ref.e_loo_shared(X, lw, r, re, diag=True)


@pytest.fixture(scope="module", params=[(3, 37), (4, 250)], ids=["S111", "S1000"])
def shared(request):
    return _shared_case(31 + request.param[1], *request.param, 17, 105)


def test_shared_form_at_the_edges_of_its_tiles(shared):
    X, r, re, lw, (mean, var, ess, kh) = shared
    Xd, rd, lwd = _dev(X), _dev(r), _dev(lw)
    worst = 0.0
    for NP in POLLS:
        for NC in COLS:
            g = loo_mod.e_loo_shared(Xd[:NC].contiguous(), lwd[:NP].contiguous(), rd[:NP].contiguous(), re[:NP], diag=True)
            worst = max(worst, float(np.abs(g.variance[:, 2] / var[:NP, 2] - 1).max()) if NC > 2 else 0.0)
            _close(g.mean, mean[:NP, :NC])
            _close(g.variance, var[:NP, :NC])
            _close(g.ess, ess[:NP])
            _close(g.pareto_k, kh[:NP, :NC])
    print(f"variance of the column at 1e6: largest relative error {worst:.2e}")
    full = loo_mod.e_loo_shared(Xd, lwd, rd, re, diag=True)
    err = np.abs(full.variance[:, 2] - var[:, 2]) / var[:, 2]
    assert err.max() <= 1e-8, float(err.max())
    # what the second pass is for: E[x^2] - E[x]^2 of the same column misses the bar
    W, x2 = np.exp(lw.reshape(17, -1)), X[2].reshape(-1)
    assert (np.abs((W @ (x2 * x2) - (W @ x2) ** 2) - var[:, 2]) / var[:, 2]).max() > 1e-8
    # diag = 0: the k of the ratios per poll, equal to potus_loo's pareto_k; without ratios no k
    g0 = loo_mod.e_loo_shared(Xd, lwd, rd, re, diag=False)
    _close(g0.pareto_k, loo_mod.loo_of_block(_dev(-r), r_eff=re).pareto_k)
    assert g0.mean.tobytes() == full.mean.tobytes() and g0.variance.tobytes() == full.variance.tobytes()
    assert full.pareto_k[:, 3].tobytes() == g0.pareto_k.tobytes()                           # the indicator column: k_r
    assert loo_mod.e_loo_shared(Xd, lwd).pareto_k is None
    # r_eff computed on the device
    gc = loo_mod.e_loo_shared(Xd[:16].contiguous(), lwd, rd, None, diag=True)
    _close(gc.pareto_k, kh[:, :16])


def test_shared_form_entry_has_the_same_bytes_alone_and_in_the_largest_call(shared):
    X, r, re, lw, _ = shared
    Xd, rd, lwd = _dev(X), _dev(r), _dev(lw)
    full = loo_mod.e_loo_shared(Xd, lwd, rd, re, diag=True)
    again = loo_mod.e_loo_shared(Xd, lwd, rd, re, diag=True)
    for k in ("mean", "variance", "ess", "pareto_k"):
        assert getattr(full, k).tobytes() == getattr(again, k).tobytes()
    for p, c in ((0, 0), (16, 104), (5, 70)):
        one = loo_mod.e_loo_shared(Xd[c:c + 1].contiguous(), lwd[p:p + 1].contiguous(), rd[p:p + 1].contiguous(), re[p:p + 1], diag=True)
        for k in ("mean", "variance", "pareto_k"):
            assert getattr(one, k)[0, 0].tobytes() == getattr(full, k)[p, c].tobytes(), (k, p, c)
        assert one.ess[0].tobytes() == full.ess[p].tobytes()


def test_shared_form_over_more_than_two_chunks_of_draws():
    chains, n = 3, 700
    assert chains * n > 2 * EL_CHUNK and (chains * n) % EL_CHUNK not in (0,)
    X, r, re, lw, (mean, var, ess, kh) = _shared_case(77, chains, n, 17, 20)
    g = loo_mod.e_loo_shared(_dev(X), _dev(lw), _dev(r), re, diag=True)
    _close(g.mean, mean)
    _close(g.variance, var)
    _close(g.ess, ess)
    _close(g.pareto_k, kh)
    assert (np.abs(g.variance[:, 2] - var[:, 2]) / var[:, 2]).max() <= 1e-8
    assert g.ms.shape == (4,) and g.ms[1] > 0 and g.ms[3] > 0


def test_the_device_weights_feed_the_shared_form(built):
    """potus_psis_device -> potus_e_loo_shared_device is the chain a fit's call makes: its means are the pointwise form's."""
    r = built[:4]
    rng = np.random.default_rng(9)
    X = rng.normal(size=(5, 4, 250))
    re = np.array([ref.r_eff_of(r[i]) for i in range(4)])
    lw, k = loo_mod.psis_weights(_dev(r), re)
    g = loo_mod.e_loo_shared(_dev(X), lw, _dev(r), re, diag=True)
    for j in range(5):
        e = loo_mod.e_loo(_dev(np.broadcast_to(X[j], r.shape)), _dev(r), "mean", None, re)
        _close(g.mean[:, j], e.mean)
        _close(g.variance[:, j], e.variance)
        _close(g.pareto_k[:, j], e.pareto_k)
    _close(k, loo_mod.e_loo_shared(_dev(X), lw, _dev(r), re).pareto_k)


def test_refusals_come_before_any_kernel():
    import torch
    L = load_library()
    x, r = torch.zeros((2, 2, 8), dtype=torch.float64, device="cuda:0"), torch.zeros((2, 2, 8), dtype=torch.float64, device="cuda:0")
    out, kh, pr = np.full((2, 4), 7.0), np.full((2, 3), 7.0), np.array([0.5])
    xp, rp = C.c_void_p(x.data_ptr()), C.c_void_p(r.data_ptr())

    def pw(xp_=xp, rp_=rp, n=8, re=None, probs=pr):
        return L.potus_e_loo_device(0, xp_, rp_, 2, 2, n, None if re is None else re.ctypes.data_as(DP), probs.ctypes.data_as(DP), probs.size,
                                    out.ctypes.data_as(DP), kh.ctypes.data_as(DP))
    assert pw() == 0
    out[:], kh[:] = 7.0, 7.0
    assert pw(n=3) == 1                                                    # fewer than four draws per chain
    for bad in (0.0, 1.0, -0.1, 1.5, np.nan):
        assert pw(probs=np.array([0.5, bad])) == 1
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert pw(re=np.array([1.0, bad])) == 1
    host = np.zeros((2, 2, 8))
    assert pw(xp_=C.c_void_p(host.ctypes.data)) == 1 and pw(rp_=C.c_void_p(host.ctypes.data)) == 1   # a block that is not this GPU's memory
    assert L.potus_e_loo_device(99, xp, rp, 2, 2, 8, None, pr.ctypes.data_as(DP), 1, out.ctypes.data_as(DP), kh.ctypes.data_as(DP)) != 0
    assert (out == 7.0).all() and (kh == 7.0).all()
    with pytest.raises(PotusError, match="inside"):
        loo_mod.e_loo(x, r, "quantile", [1.2])
    with pytest.raises(ValueError):
        loo_mod.e_loo(x, r, "median")
    mean, var, ess, k = np.full((2, 2), 7.0), np.full((2, 2), 7.0), np.full(2, 7.0), np.full((2, 2), 7.0)

    def sh(xp_=xp, wp_=rp, rp_=rp, n=8, diag=1, re=None):
        return L.potus_e_loo_shared_device(0, xp_, 2, wp_, 2, 2, n, rp_, None if re is None else re.ctypes.data_as(DP), diag, mean.ctypes.data_as(DP),
                                           var.ctypes.data_as(DP), ess.ctypes.data_as(DP), k.ctypes.data_as(DP))
    assert sh(n=3) == 1 and sh(diag=2) == 1 and sh(rp_=None, diag=1) == 1 and sh(re=np.array([1.0, 0.0])) == 1
    hp = C.c_void_p(host.ctypes.data)
    assert sh(xp_=hp) == 1 and sh(wp_=hp) == 1 and sh(rp_=hp) == 1
    assert (mean == 7.0).all() and (var == 7.0).all() and (ess == 7.0).all() and (k == 7.0).all()
    # blocks on two devices: the same check as the host pointer above (hipPointerGetAttributes: not memory of the named GPU), which is what
    # exercises it on a machine with one GPU; with a second GPU the very case runs as well
    if torch.cuda.device_count() > 1:
        other = torch.zeros((2, 2, 8), dtype=torch.float64, device="cuda:1")
        assert pw(rp_=C.c_void_p(other.data_ptr())) == 1 and sh(wp_=C.c_void_p(other.data_ptr())) == 1
    with pytest.raises(TypeError):
        loo_mod.e_loo(x.float(), r)
    with pytest.raises(ValueError):
        loo_mod.e_loo_shared(x, r, diag=True)
