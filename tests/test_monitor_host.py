"""CPU tests of the summary-table layer: the numpy restatement (diagnostics.py) on cases worked by hand, the Monitor object on a built table, the
refusals that need no device, and the names of the new entry points in the header, the R shim and sampler.EXPORTS."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from us_potus_model_amd import diagnostics as dg, monitor as mn, sampler

ROOT = Path(__file__).resolve().parent.parent


def test_new_names_are_declared_exported_and_wrapped():
    new = {"potus_monitor", "potus_monitor_device", "potus_R_monitor"}
    hdr = (ROOT / "include" / "potus_hmc.h").read_text()
    assert new <= set(re.findall(r"\b(potus_[A-Za-z_0-9]+)\s*\(", hdr))
    assert re.search(r"#define\s+POTUS_MONITOR_NSTATS\s+8\b", hdr) and mn.N_STATS == 8 == len(dg.MONITOR_STATS)
    assert new <= set(sampler.EXPORTS)
    r = (ROOT / "R" / "potus_sampling.R").read_text()
    assert '"potus_R_monitor"' in r and "potus_monitor <- function(fit, pars = NULL, probs = c(.025, .25, .5, .75, .975))" in r
    L = sampler.load_library()
    assert all(hasattr(L, nm) for nm in new)
    import us_potus_model_amd as pkg
    # (the package attribute `monitor` stays the module; its function is re-exported as monitor_table)
    assert pkg.monitor is mn and pkg.monitor_table is mn.monitor and pkg.monitor_of_block is mn.monitor_of_block and pkg.Monitor is mn.Monitor
    assert hasattr(sampler.Handle, "monitor") and hasattr(sampler.StanFit, "monitor")
    # potus_set_datasets' list of pooled calls that refuse names the new one
    assert re.search(r"calls that pool all chains \([^)]*potus_monitor[^)]*\) refuse", hdr.replace("\n *", ""))


# ---- the restatement, by hand
def test_quantile_and_mad_by_hand():
    assert dg.quantile7([1, 2, 3, 4], 0.25) == 1.75                 # h = 0.75: 1 + 0.75 (2 - 1)
    assert dg.quantile7([4, 1, 3, 2], 0.0) == 1.0 and dg.quantile7([4, 1, 3, 2], 1.0) == 4.0 and dg.quantile7([1, 2, 3, 4], 0.5) == 2.5
    assert dg.mad([1, 2, 3, 4, 100]) == 1.4826                      # median 3, |x - 3| = 2 1 0 1 97, median 1
    assert dg.mad([[1, 2], [3, 4]]) == 1.4826                       # median 2.5, deviations 1.5 0.5 0.5 1.5: median 1
    x = np.random.default_rng(5).standard_normal((3, 41))
    for p in (0.05, 0.5, 0.95, 0.975):
        assert dg.quantile7(x, p) == pytest.approx(np.quantile(x, p), rel=1e-14)


def test_constant_and_non_finite_columns():
    c = np.full((4, 100), 2.5)
    assert np.isnan(dg.ess_tail(c))
    row = dg.monitor_row(c, (0.1, 0.9))
    assert row[:3].tolist() == [2.5, 0.0, 0.0] and np.isnan(row[3:8]).all() and row[8:].tolist() == [2.5, 2.5]
    bad = np.random.default_rng(0).standard_normal((4, 100))
    bad[1, 7] = np.inf
    assert np.isnan(dg.monitor_row(bad, (0.5,))).all()
    few = dg.monitor_row(np.arange(12.0).reshape(2, 6), (0.5,))      # three draws per half: R-hat, no ESS
    assert np.isfinite(few[[0, 1, 2, 4, 8]]).all() and np.isnan(few[[3, 5, 6, 7]]).all()


def test_ess_of_independent_and_autocorrelated_draws():
    rng = np.random.default_rng(0)
    N = 4000
    x = rng.standard_normal((4, 1000))
    assert 0.5 * N <= dg.ess_tail(x) <= 1.5 * N and 0.5 * N <= dg.ess_mean(x) <= 1.5 * N
    rho = 0.9
    e = rng.standard_normal((4, 1000))
    y = np.zeros((4, 1000))
    y[:, 0] = e[:, 0]
    for t in range(1, 1000):
        y[:, t] = rho * y[:, t - 1] + np.sqrt(1 - rho * rho) * e[:, t]
    want = N * (1 - rho) / (1 + rho)
    assert abs(dg.ess_mean(y) / want - 1) <= 0.30, dg.ess_mean(y) / want
    assert dg.mcse_mean(y) == pytest.approx(y.std(ddof=1) / np.sqrt(dg.ess_mean(y)), rel=1e-15)
    assert dg.ess_tail(y) == min(dg.ess_quantile(y, 0.05), dg.ess_quantile(y, 0.95))


def test_summarise_keeps_its_keys_and_adds_the_rest_of_the_row():
    d = np.random.default_rng(2).standard_normal((3, 40, 2))
    s = dg.summarise(d, probs=(0.25, 0.75))
    assert {"rhat", "ess_bulk", "ess_mean", "mean", "sd", "mcse"} <= set(s) and {"mad", "ess_tail", "mcse_mean", "quantiles"} <= set(s)
    for j in range(2):
        row = dg.monitor_row(d[:, :, j], (0.25, 0.75))
        got = [s[k][j] for k in dg.MONITOR_STATS] + list(s["quantiles"][j])
        assert got == row.tolist()
    assert "quantiles" not in dg.summarise(d)


# ---- Monitor on a built table
def _built():
    rng = np.random.default_rng(9)
    P_, S, T = 3, 2, 4
    draws = {"lp__": rng.standard_normal((2, 30)) - 50, "mu_c": rng.standard_normal((2, 30, P_)), "mu_b": rng.standard_normal((2, 30, S * T))}
    probs = (0.025, 0.5, 0.975)
    rows = [dg.monitor_row(draws["lp__"], probs)] + [dg.monitor_row(draws["mu_c"][:, :, j], probs) for j in range(P_)] + \
           [dg.monitor_row(draws["mu_b"][:, :, j], probs) for j in range(S * T)]
    names = ["lp__"] + [f"mu_c.{i + 1}" for i in range(P_)] + [f"mu_b.{s + 1}.{t + 1}" for t in range(T) for s in range(S)]
    blocks = {"lp__": (0, 1, ()), "mu_c": (1, 1 + P_, (P_,)), "mu_b": (1 + P_, 1 + P_ + S * T, (S, T))}
    return draws, mn.Monitor(np.array(rows), names, probs, blocks, n_chains=2, n_draws=30)


def test_monitor_object_on_a_built_table():
    draws, m = _built()
    assert len(m) == 12 and m.stats == dg.MONITOR_STATS + ("2.5%", "50%", "97.5%")
    assert m.par("lp__").shape == (11,) and m.par("mu_c").shape == (3, 11) and m.par("mu_b").shape == (2, 4, 11)
    # column-major: mu_b[s, t] is row s + S t of the block
    assert m.par("mu_b")[1, 2, 0] == draws["mu_b"][:, :, 1 + 2 * 2].mean() and m.names[4 + 1 + 2 * 2] == "mu_b.2.3"
    mlh = m.mean_low_high("mu_c")
    mean, sd = draws["mu_c"].mean(axis=(0, 1)), draws["mu_c"].reshape(-1, 3).std(axis=0, ddof=1)
    assert mlh.shape == (3, 3) and np.allclose(mlh, np.stack([mean, mean - 1.96 * sd, mean + 1.96 * sd], axis=1), rtol=1e-14)
    assert m.mean_low_high("lp__", z=1.0).shape == (3,) and m.mean_low_high("mu_b").shape == (2, 4, 3)
    assert m.column("rhat").shape == (12,) and m.column("50%")[0] == pytest.approx(np.median(draws["lp__"]), rel=1e-14)
    with pytest.raises(KeyError, match="not in this table"):
        m.par("e_bias")
    text = str(m).splitlines()
    assert text[0] == "Inference for 12 columns: 2 chains, each with 30 post-warmup draws; total post-warmup draws=60."
    assert text[2].split() == ["mean", "se_mean", "sd", "2.5%", "50%", "97.5%", "n_eff", "Rhat", "tail_eff"]
    assert text[3].split()[0] == "lp__" and len(text[3].split()) == 10 and text[3 + 11].startswith("mu_b.2.4")
    with pytest.raises(ValueError, match="shape"):
        mn.Monitor(np.zeros((2, 8)), ["a"], ())


def test_pars_selection_needs_no_device():
    class H:                                                         # what _ranges reads of a Handle
        n_cols = 30
        layout = {"mu_c": (7, 10, (3,)), "mu_b": (10, 18, (2, 4)), "sigma_rho": (18, 19, ())}
    assert mn._ranges(H, ["lp__", "mu_b", "sigma_rho"], None) == [("lp__", 0, 1, ()), ("mu_b", 10, 18, (2, 4)), ("sigma_rho", 18, 19, ())]
    assert mn._ranges(H, "mu_c", None) == [("mu_c", 7, 10, (3,))]
    assert mn._ranges(H, None, None) == [(None, 0, 30, None)] and mn._ranges(H, None, (5, 9)) == [(None, 5, 9, None)]
    with pytest.raises(KeyError, match="unknown parameter"):
        mn._ranges(H, ["mu_x"], None)
    with pytest.raises(ValueError, match="columns"):
        mn._ranges(H, None, (5, 31))
    with pytest.raises(ValueError, match="not both"):
        mn._ranges(H, ["mu_c"], (0, 1))


# ---- refusals that need no device
def test_python_argument_refusals():
    with pytest.raises(ValueError, match="at most 16"):
        mn._probs(np.linspace(0, 1, 17))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        mn._probs([0.5, 1.5])
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        mn._probs([np.nan])
    assert mn._probs(()).size == 0 and mn._probs(None).size == 0 and mn._probs([0, 1]).tolist() == [0.0, 1.0]
    import torch
    with pytest.raises(TypeError, match="on the GPU"):
        mn.monitor_of_block(torch.zeros((8, 2, 3), dtype=torch.float64))
    with pytest.raises(TypeError, match="n_draws"):
        mn.monitor_of_block(4096)


def test_library_refuses_bad_arguments_before_touching_a_device():
    L = sampler.load_library()
    DP = C.POINTER(C.c_double)
    fake = C.c_void_p(4096)                                          # never dereferenced: every call below is refused first
    out = np.zeros(8 + 17)

    def dev(probs=(0.5,), n_probs=None, o=out, n_draws=10, n_chains=2, n_cols=1, block=fake):
        p = np.array(probs, dtype=np.float64)
        return L.potus_monitor_device(0, block, n_draws, n_chains, n_cols, p.ctypes.data_as(DP) if p.size else None,
                                      len(p) if n_probs is None else n_probs, None if o is None else o.ctypes.data_as(DP))

    def message():
        buf = C.create_string_buffer(512)
        L.potus_last_error(buf, 512)
        return buf.value.decode()
    assert dev(probs=np.linspace(0, 1, 17)) == 1 and "n_probs = 17" in message()
    assert dev(n_probs=-1) == 1
    assert dev(probs=(0.5, 1.5)) == 1 and "probs[1] = 1.5 outside [0, 1]" in message()
    assert dev(probs=(np.nan,)) == 1 and "outside [0, 1]" in message()
    assert dev(probs=(), n_probs=2) == 1 and "null probs" in message()
    assert dev(o=None) == 1 and "null out" in message()
    assert dev(n_cols=0) == 1 and dev(n_draws=0) == 1 and dev(block=None) == 1
    assert dev(n_chains=600) == 6 and "600 chains pooled (at most 512)" in message()
    ids = (C.c_int * 1)(-7)
    p = np.array([0.5])

    def pooled(cb=0, ce=1, n_probs=1, o=out, h=ids, probs=p):
        return L.potus_monitor(h, 1, cb, ce, probs.ctypes.data_as(DP), n_probs, None if o is None else o.ctypes.data_as(DP))
    assert pooled(n_probs=17) == 1 and "n_probs = 17" in message()
    assert pooled(probs=np.array([1.5])) == 1 and pooled(probs=np.array([np.nan])) == 1
    assert pooled(o=None) == 1 and "null out" in message()
    assert pooled(cb=3, ce=3) == 1 and "columns [3, 3)" in message()          # an empty range
    assert pooled(cb=-1) == 1
    assert pooled() == 4 and "bad handle" in message()
    assert L.potus_monitor(None, 0, 0, 1, p.ctypes.data_as(DP), 1, out.ctypes.data_as(DP)) == 1
    st = C.c_int(-1)
    cols = (C.c_int * 2)(0, 0)
    L.potus_R_monitor(ids, C.byref(C.c_int(1)), cols, p.ctypes.data_as(DP), C.byref(C.c_int(1)), out.ctypes.data_as(DP), C.byref(st))
    assert st.value == 1
