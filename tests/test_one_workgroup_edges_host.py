"""The designs of tests/test_gpu_one_workgroup_edges.py without a GPU (tests/one_workgroup_cases.py): the constants the restated schedule uses against the text of
csrc/potus_model.hpp and build_model; every design's stated structure against its own arrays; the oracle at every design -- shapes that are new to its
scan / sparse gradient too -- against the independent torch transcription (tests/stan_transcription.py) at the tolerance of test_oracle.py (1e-12 of the log
density, 1e-12 of the gradient's max-norm), its fast form against its literal form (1e-12, as there); and, on the oracle's rows alone, the precondition of the chain
comparison: a non-divergent transition of depth >= 5 among the twelve rows of each chain."""
import re

import numpy as np
import pytest

import one_workgroup_cases as cases
from conftest import ROOT

CSRC = ROOT / "us_potus_model_amd" / "csrc"


def test_the_constants_are_the_sources():
    hpp, hip = (CSRC / "potus_model.hpp").read_text(), (CSRC / "potus_hmc.hip").read_text()
    define = lambda name: re.search(rf"^#define {name}\s+(.+?)\s*(//.*)?$", hpp, re.M).group(1)
    assert int(define("PT_NW")) == cases.WAVES and define("PT_THREADS") == "(64 * PT_NW)" and cases.THREADS == 64 * cases.WAVES
    assert define("PT_CH") == "(256 / PT_NW)" and cases.DAYS_PER_WAVE == 256 // cases.WAVES
    assert int(define("PT_SUBLEN")) == cases.SUBLEN
    assert "const int per = (T + 63) / 64, ta = lane * per, tb = min(T, ta + per);" in hpp and hpp.count("const int per = (T + 63) / 64") == 2
    assert "constexpr int PER = 4;" in hpp
    assert "for (int i0 = PT_THREADS; i0 < nmid; i0 += PT_THREADS) {" in hpp and "for (int seg = tid + PT_THREADS; seg < nseg; seg += PT_THREADS) {" in hpp
    assert f"if (wt[wv].size() < {cases.WAVE_DAYS} && npolls_w[wv] + nt <= {cases.WAVE_POLLS} && (wmin < 0 || load[wv] < load[wmin])) wmin = wv;" in hip
    assert "load[wmin] += day_ptr[t + 1] - day_ptr[t] + 2;" in hip
    assert f"if (sp->lds_bytes > {cases.LDS_LIMIT // 1024} * 1024) k1_fail(" in hip


def test_every_edge_of_the_issue_has_its_design():
    st = {name: cases.structure(dz["data"], dz["variant"]) for name, dz in ((n, f()) for n, f in cases.DESIGNS.items())}
    assert {s["per"] for s in st.values()} == {1, 2, 3, 4}
    assert {(st[f"T{T}"]["per"], st[f"T{T}"]["lanes"]) for T in (64, 65, 129, 193)} == {(1, 64), (2, 33), (3, 43), (4, 49)}
    assert (st["capacity"]["per"], st["capacity"]["lanes"]) == (4, 64)
    assert max(s["nmid"] for s in st.values()) > cases.THREADS and st["many_days_few_pollsters"]["nmid"] == cases.THREADS + 1
    assert st["many_pollsters_short/nomode"]["nmid"] > cases.THREADS and st["capacity/nomode"]["nmid"] > cases.THREADS
    assert {tuple(s["beyond"]) for s in st.values()} == {(), (2,), (0, 1), (0, 1, 2)}
    assert st["capacity"]["waves"][-1] == (cases.WAVE_POLLS, cases.WAVE_DAYS) and st["capacity"]["polls"] == 2 * 2 * cases.THREADS
    assert st["day_of_256"]["waves"][0] == (cases.WAVE_POLLS, 1) and set(st["one_pollster_2048"]["waves"]) == {(cases.WAVE_POLLS, 16)}
    assert {int(n) for n in st["pollster_lists_0_1_16_17"]["pollster_lists"]} == {0, 1, cases.SUBLEN, cases.SUBLEN + 1, 2 * cases.SUBLEN, 2 * cases.SUBLEN + 1}
    assert int(st["one_pollster_2048"]["pollster_lists"][0]) == 128 * cases.SUBLEN
    empty_beyond = np.flatnonzero(st["capacity"]["pollster_lists"][cases.THREADS:] == 0)
    assert len(empty_beyond) and (st["capacity"]["pollster_lists"][cases.THREADS:] > 0).any()
    assert {int(cases.DESIGNS[f"S{S}"]()["data"]["S"]) for S in (8, 9, 16, 17)} == {8, 9, 16, 17}
    assert {int(cases.DESIGNS[f"T{T}"]()["data"]["T"]) for T in (32, 33, 225)} == {32, 33, 225}
    # the extra loop's day segments of many_days_few_pollsters: one without polls among them
    md = st["many_days_few_pollsters"]
    days_beyond = md["per_day"][cases.THREADS - md["nseg"]:]
    assert len(days_beyond) == md["nseg"] - cases.THREADS == 6 and (days_beyond == 0).sum() == 1 and (days_beyond > 0).sum() == 5


@pytest.mark.parametrize("name", list(cases.ALL))
def test_the_design_is_what_it_says(name):
    dz = cases.ALL[name]()
    st = cases.assert_preconditions(dz)
    assert (st["waves"] is None or st["per"] > 4 or "lds_more_than" in dz) == (name in cases.REFUSED)


@pytest.mark.parametrize("name", list(cases.ALL))
def test_the_oracle_matches_the_transcription_and_its_fast_form(name):
    import stan_transcription as st
    dz, q, lpg, _ = cases.reference(name)
    from oracle_lib import OracleModel
    m = OracleModel(dz["data"], dz["variant"])
    for i in (1, 2):
        lp, grad = lpg[i]
        lpt, gt, _ = st.log_prob_grad(dz["data"], q[i], dz["variant"])
        scale = np.abs(gt).max()
        lpf, gradf = m.log_prob_grad(q[i], fast=True)
        print(f"{name} point {i}: oracle - transcription lp {abs(lp - lpt) / abs(lpt):.1e}, grad {np.abs(grad - gt).max() / scale:.1e}; "
              f"fast - literal lp {abs(lpf - lp) / abs(lp):.1e}, grad {np.abs(gradf - grad).max() / scale:.1e}")
        assert abs(lp - lpt) <= 1e-12 * abs(lpt)
        assert np.abs(grad - gt).max() <= 1e-12 * scale
        assert abs(lpf - lp) <= 1e-12 * abs(lp) and np.abs(gradf - grad).max() <= 1e-12 * scale


@pytest.mark.parametrize("name", list(cases.DESIGNS))
def test_the_rows_compared_reach_real_trees(name):
    _, _, _, rows = cases.reference(name)
    assert len(rows) == 2 and all(r.shape[0] == cases.ROWS for r in rows)
    cases.assert_real_trees(name, rows)
