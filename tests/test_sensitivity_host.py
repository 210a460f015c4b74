"""Prior sensitivity by refit, the parts that need no GPU: the numpy restatement of the three distances (tests/sens_ref.py), the designs
sensitivity.grid builds, the flags, and the entry points' declarations and argument refusals."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import sens_ref
from us_potus_model_amd import sampler, sensitivity, synthetic, timeline
from us_potus_model_amd.sampler import N_SCALES, SCALE_NAMES

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------ the restatement
def test_distances_of_identical_samples_are_zero():
    x = np.random.default_rng(0).standard_normal(50)
    assert sens_ref.distance(x, x) == (0.0, 0.0, 0.0)
    assert sens_ref.distance(x, x[::-1]) == (0.0, 0.0, 0.0)
    assert sens_ref.distance([2.0], [2.0, 2.0]) == (0.0, 0.0, 0.0)                # m = 1
    assert sens_ref.distance(np.tile(x, 2), x) == (0.0, 0.0, 0.0)                 # the same distribution function at another size


@pytest.mark.parametrize("na,nb", [(1, 1), (7, 12), (200, 200), (64, 65)])
def test_distances_are_symmetric_and_bounded(na, nb):
    rng = np.random.default_rng(na * 1000 + nb)
    for a, b in ((rng.standard_normal(na), 0.5 + rng.standard_normal(nb)), (rng.integers(0, 4, na).astype(float), rng.integers(1, 5, nb).astype(float))):
        w1, ks, c2 = sens_ref.distance(a, b)
        w1r, ksr, c2r = sens_ref.distance(b, a)
        assert abs(w1 - w1r) <= 1e-13 * max(np.ptp(np.concatenate([a, b])), 1.0) and ks == ksr and abs(c2 - c2r) <= 1e-13
        assert 0.0 <= ks <= 1.0 and 0.0 <= c2 <= 1.0 and w1 >= 0.0
        # cjs takes the larger of the two orientations, so negating both samples leaves it alone
        assert abs(sens_ref.distance(-a, -b)[2] - c2) <= 1e-15


def test_w1_of_a_shifted_sample_is_the_shift_and_disjoint_samples_are_at_distance_one():
    x = np.random.default_rng(1).standard_normal(300)
    for shift in (0.25, 3.0, 1e6):
        w1, ks, c2 = sens_ref.distance(x + shift, x)
        assert abs(w1 - shift) <= 1e-12 * shift * 300
    w1, ks, c2 = sens_ref.distance(x + 100.0, x)                                  # no overlap
    assert ks == 1.0 and 0.0 < c2 <= 1.0
    assert sens_ref.distance([1.0, 1.0], [3.0]) == (2.0, 1.0, 1.0)                 # one constant against another
    # w1 against the sorted-sample form for equal sizes, ks against a brute-force maximum
    a, b = np.random.default_rng(2).standard_normal(40), np.random.default_rng(3).standard_normal(40) * 2
    w1, ks, _ = sens_ref.distance(a, b)
    assert abs(w1 - np.abs(np.sort(a) - np.sort(b)).mean()) <= 1e-13
    grid = np.concatenate([a, b])
    assert ks == max(abs((a <= t).mean() - (b <= t).mean()) for t in grid)


def test_a_non_finite_value_makes_its_column_nan_alone():
    a, b = np.random.default_rng(4).standard_normal((10, 3)), np.random.default_rng(5).standard_normal((12, 3))
    a[3, 1] = np.inf
    out = sens_ref.distance_columns(a, b)
    assert np.isnan(out[1]).all() and np.isfinite(out[[0, 2]]).all()


# ------------------------------------------------------------------------------------------------ designs
def test_grid_one_at_a_time():
    data = synthetic.small("full")
    d = sensitivity.grid(data, {"sigma_c": [0.5, 2], "mu_b_T_scale": [3]})
    assert d["labels"] == ["baseline", "null copy", "sigma_c x 0.5", "sigma_c x 2", "mu_b_T_scale x 3"] and d["null"] == 1
    assert d["scales"].shape == d["factors"].shape == (5, N_SCALES) and d["varied"].tolist() == [-1, -1, 0, 0, 7]
    base = sensitivity.scales_of(data)
    assert base.tolist() == [float(data[nm]) for nm in SCALE_NAMES]
    assert d["scales"][0].tobytes() == base.tobytes() == d["scales"][1].tobytes()
    assert d["scales"][3, 0] == 2 * data["sigma_c"] and d["scales"][4, 7] == 3 * data["mu_b_T_scale"] and (d["factors"][2] == [0.5] + [1.0] * 8).all()
    assert d["keep_state"].shape == (5, data["N_state_polls"]) and d["keep_state"].all() and d["keep_national"].all()
    assert d["mu_b_prior"] is None and d["mu_b_T_scale"] is None                  # the scale travels in scales alone
    one = timeline.data_of(d, 4)                                                  # what a stand-alone handle of the setting takes
    assert one["mu_b_T_scale"] == 3 * data["mu_b_T_scale"] and one["sigma_c"] == data["sigma_c"]
    assert (one["n_two_share_state"] == np.asarray(data["n_two_share_state"])).all()
    assert timeline.data_of(d, 0)["sigma_c"] == data["sigma_c"]
    no_null = sensitivity.grid(data, {"sigma_pop": [2]}, null=False)
    assert no_null["labels"] == ["baseline", "sigma_pop x 2"] and no_null["null"] is None
    with pytest.raises(ValueError, match="not a prior scale"):
        sensitivity.grid(data, {"sigma": [2]})
    with pytest.raises(ValueError, match="positive and finite"):
        sensitivity.grid(data, {"sigma_c": [0.0]})
    with pytest.raises(ValueError, match="no scales"):
        sensitivity.fit(timeline.design_of(data, d["keep_state"], d["keep_national"]))


def test_grid_product_is_the_full_factorial():
    data = synthetic.small("full")
    d = sensitivity.grid(data, {"sigma_measure_noise_state": [0.5, 1, 2], "sigma_measure_noise_national": [0.5, 1, 2]}, product=True)   # the reference's 3 x 3
    assert d["scales"].shape == (2 + 9, N_SCALES)
    got = {(f[4], f[3]) for f in d["factors"][2:]}
    assert got == {(a, b) for a in (0.5, 1.0, 2.0) for b in (0.5, 1.0, 2.0)}
    assert d["labels"][2] == "sigma_measure_noise_state x 0.5, sigma_measure_noise_national x 0.5"
    assert d["varied"][2] == -1 and d["varied"][3] == 4                           # (0.5, 1) changes one scale


def test_no_mode_data_has_no_mode_scales():
    data = synthetic.small("no_mode_adjustment")
    base = sensitivity.scales_of(data)
    assert base[[1, 2, 5]].tolist() == [0.0, 0.0, 0.0] and (base[[0, 3, 4, 6, 7, 8]] > 0).all()


def test_sensitivity_and_flags():
    """Two days, S = 2 (columns: two states, national, electoral votes); baseline, null copy, one scale x 4, two scales changed."""
    factors = np.ones((4, N_SCALES))
    factors[2, 7], factors[3, 0], factors[3, 1] = 4.0, 2.0, 2.0
    varied = np.array([-1, -1, 7, -1])
    cjs = np.zeros((4, 2, 4))
    cjs[1] = [[0.02, 0.04, 0.03, 0.20], [0.01, 0.01, 0.01, 0.01]]                 # the floor: noisy electoral votes on day 0
    cjs[2] = [[0.30, 0.03, 0.12, 0.15], [0.09, 0.30, 0.02, np.nan]]
    cjs[3] = [[0.06, 0.04, 0.01, 0.30], [0.0, 0.0, 0.0, 0.0]]
    s = sensitivity.sensitivity_of(cjs, factors, varied)
    assert np.isnan(s[[0, 1, 3]]).all() and np.array_equal(s[2], cjs[2] / 2.0, equal_nan=True)
    design = dict(factors=factors, varied=varied, null=1, labels=["baseline", "null copy", "mu_b_T_scale x 4", "two"])
    c = sensitivity.Comparison(np.stack([cjs, cjs, cjs], -1), np.full(4, 10), design, (0, 2), 0)
    assert c.floor.shape == (3, 2, 4) and c.floor_of_kind().tolist() == [[0.04, 0.03, 0.20], [0.01, 0.01, 0.01]]
    fl = c.flag()
    assert not fl[0].any() and not fl[1].any()
    # x 4: sensitivity = cjs / 2 >= 0.05 and cjs above the largest floor of its kind; 0.03 is below the states' floor, 0.15 below the EV floor
    assert fl[2].tolist() == [[True, False, True, False], [False, True, False, False]]
    # several scales changed: cjs itself is the measure; 0.04 is not above the states' floor of 0.04
    assert fl[3].tolist() == [[True, False, False, True], [False, False, False, False]]
    assert c.flag(threshold=0.2)[2].tolist() == [[False, False, False, False], [False, False, False, False]]
    t = c.table(day=0)
    assert "mu_b_T_scale x 4" in t and "state, national" in t and len(t.splitlines()) == 5


# ------------------------------------------------------------------------------------------------ declarations and refusals without a device
NEW = {"potus_set_datasets_grid", "potus_ecdf_distance_device", "potus_grid_compare", "potus_grid_timing", "potus_R_set_datasets_grid", "potus_R_grid_compare"}


def test_entry_points_are_declared_everywhere():
    hdr = (ROOT / "include" / "potus_hmc.h").read_text()
    assert NEW <= set(re.findall(r"\b(potus_[A-Za-z_0-9]+)\s*\(", hdr)) and NEW <= set(sampler.EXPORTS)
    assert "#define POTUS_N_SCALES 9" in hdr
    for line in ("x_1 < ... < x_m are the distinct values of the union of the two samples.", "ks  = max_j |P_j - Q_j|.", "c = 0 when m = 1."):
        assert line in hdr and line in (ROOT / "us_potus_model_amd" / "csrc" / "potus_sens.hpp").read_text()
    for name in ("set_datasets_grid", "grid_compare", "grid_timing"):
        assert callable(getattr(sampler.Handle, name))
    import us_potus_model_amd as pkg
    assert pkg.sensitivity is sensitivity and pkg.SCALE_NAMES == SCALE_NAMES and callable(pkg.ecdf_distance_device)
    r = (ROOT / "R" / "potus_sampling.R").read_text()
    assert '.C("potus_R_set_datasets_grid"' in r and '.C("potus_R_grid_compare"' in r and re.search(r"^potus_prior_grid <- function\(", r, re.M)
    L = sampler.load_library()
    for name in NEW:
        assert hasattr(L, name), name


def test_refusals_and_dot_c_marshalling_need_no_device():
    L = sampler.load_library()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    buf = C.create_string_buffer(512)

    def err():
        L.potus_last_error(buf, 512)
        return buf.value.decode()
    assert L.potus_grid_timing(None) == 1                                        # POTUS_ERR_ARG
    out = np.zeros(3)
    x = np.zeros(4)
    p = C.c_void_p(x.ctypes.data)
    # sizes are refused before the pointers are looked at: more than 16 384 draws, none
    assert L.potus_ecdf_distance_device(0, p, 8192, p, 8193, 1, out.ctypes.data_as(dp)) == 6 and "at most 16384" in err()      # POTUS_ERR_UNSUPPORTED
    assert L.potus_ecdf_distance_device(0, p, 0, p, 4, 1, out.ctypes.data_as(dp)) == 1 and "at least one draw" in err()
    assert L.potus_ecdf_distance_device(0, None, 4, p, 4, 1, out.ctypes.data_as(dp)) == 1
    assert L.potus_ecdf_distance_device(0, p, 4, p, 4, 0, out.ctypes.data_as(dp)) == 1
    assert L.potus_grid_compare(12345, 0, 0, 1, out.ctypes.data_as(dp), 270, out.ctypes.data_as(dp), None) == 4 and "handle" in err()   # POTUS_ERR_STATE
    assert L.potus_set_datasets_grid(12345, 1, None, None, None, None, None, None, out.ctypes.data_as(dp)) == 4
    # the .C() entries take every argument by pointer and hand the status back through the last one
    st = (C.c_int * 1)(-1)
    sc = np.ones((2, N_SCALES))
    L.potus_R_set_datasets_grid((C.c_int * 1)(12345), (C.c_int * 1)(2), None, None, None, None, (C.c_int * 3)(0, 0, 1), x.ctypes.data_as(dp), x.ctypes.data_as(dp),
                                sc.ctypes.data_as(dp), st)
    assert st[0] == 4 and "handle" in err()
    st[0] = -1
    cnt = np.zeros(2, np.int32)
    L.potus_R_grid_compare((C.c_int * 1)(12345), (C.c_int * 4)(0, 0, 1, 270), x.ctypes.data_as(dp), out.ctypes.data_as(dp), cnt.ctypes.data_as(ip), st)
    assert st[0] == 4 and "handle" in err()
