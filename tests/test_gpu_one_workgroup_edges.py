"""The one-workgroup model pass (csrc/potus_model.hpp, model_pass) and build_model's schedule at the edges of their layout: the designs of
tests/one_workgroup_cases.py, each with its structure stated as literals and asserted on its own arrays before the library sees them, all with cus_per_chain = 1.

  a. Handle.log_prob_grad (k_logprob_grad, PlainPolicy) against OracleModel.log_prob_grad (the literal form) at zeros, uniform(-2, 2) and 0.2 x normal: log density to
     1e-11 relative, gradient to 1e-10 of its max-norm and, block by block, to 1e-10 of the block's own max-norm;
  b. 12 warm-up transitions of two chains (k_init / k_run, LeapPolicy) against OracleModel.sample_chain: tree depth, leapfrogs and divergence equal, values to 1e-6 / 1e-7
     (a chain that leaves the oracle's on a 13th digit is replayed row by row from its own previous row, adaptation_replay.py, same tolerances); the oracle's rows reach
     a non-divergent tree of depth >= 5 in each chain (precondition, test_one_workgroup_edges_host.py holds it without a GPU as well);
  c. the same run on two workgroups per chain (k_run_twin): the bytes of b, draws and adaptation;
  d. the saved rows through write_array (wa_build_row) against OracleModel.write_array, rtol 1e-11 / atol 1e-12 as test_write_array_matches_oracle;
  e. every device call made twice: the same bytes.

Then what one workgroup per chain must refuse (T = 257, a day of 257 polls, a 65th four-poll day on top of `capacity`, S = 63 x T = 256 beyond 160 KiB of LDS): the
message as text, the same data on the cluster the library picks by itself (cus_per_chain = 0) through leg a, and Handle.optimize on the T = 257 model.

Measured on an MI355X, worst over the 21 designs: a. log density 1.7e-15, gradient 1.0e-15 of its max-norm (`one_pollster_2048`), worst block on its own scale 1.7e-13
(rho_e_bias at `T225`; 6.5e-15 elsewhere); `capacity` with its 2 048 polls: 1.7e-15 / 6.3e-16 / 4.3e-15.  b. every chain in step with the oracle's over the twelve rows
but chain 2 of `many_pollsters_short/nomode` and of `day_of_256`, which leave it at row 11 and pass the replay; the chains in step agree to 4.0e-7 of 0.1 + |value| (bound
1e-6), 1 510 to 9 624 leapfrogs per design.  c. and e. the same bytes.  d. 8.0e-15 of 0.1 + |value| (bound 1e-11).  The four refused designs on the 16 members the library
picks: 7.1e-16 / 9.6e-16 / 4.3e-15.  No defect was found in the pass or the schedule; potus_optimize and its kin named the handle's cluster size before the model's own
reason on a model beyond these kernels, which now comes first.

Wall time of this module on the MI355X: 11 s for its 46 cases, the oracle's share included (the slowest, `capacity`, 1.2 s)."""
import numpy as np
import pytest

import one_workgroup_cases as cases
from adaptation_replay import adaptation_replayed_from_the_device_rows
from oracle_lib import OracleModel
from test_gpu_parity import GRAD_RTOL, LP_RTOL, _worst_block
from us_potus_model_amd import Handle, sampler

pytestmark = pytest.mark.gpu

ROWS = cases.ROWS


def open_handle(dz, cus=1, **kw):
    return Handle(dz["data"], dz["variant"], chains=2, num_warmup=ROWS, num_samples=0, save_warmup=1, seed=dz["seed"], cus_per_chain=cus, **kw)


def leg_a(name, h):
    """Leg a (and e for this call) on an open handle; the worst deviations are printed before anything is asserted."""
    dz, q, lpg, _ = cases.reference(name)
    data, variant = dz["data"], dz["variant"]
    lp, grad = h.log_prob_grad(q)
    lp2, grad2 = h.log_prob_grad(q)
    dev = []
    for i, (lpo, go) in enumerate(lpg):
        err = np.abs(grad[i] - go)
        dev.append((abs(lp[i] - lpo) / abs(lpo), err.max() / np.abs(go).max(), _worst_block(data, variant, err, go)))
    print(f"{name} K={h.cus_per_chain}: lp {max(d[0] for d in dev):.2e}, grad / max-norm {max(d[1] for d in dev):.2e}, "
          f"worst block on its own scale {max((d[2] for d in dev), key=lambda t: t[1])}")
    for i, (dlp, dg, worst) in enumerate(dev):
        assert dlp <= LP_RTOL, (name, i, lp[i], lpg[i][0])
        assert dg <= GRAD_RTOL, (name, i, dg)
        assert worst[1] <= GRAD_RTOL, (name, i, worst)
    assert np.array_equal(lp, lp2) and np.array_equal(grad, grad2), "the call does not repeat its bytes"


def in_step(d, ref):
    return np.array_equal(d[:, 3:6], ref[:, 3:6]) and np.allclose(d[:, 7:], ref[:, 7:], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("name", list(cases.DESIGNS))
def test_log_density_and_gradient_match_the_oracle(name):
    dz = cases.reference(name)[0]
    cases.assert_preconditions(dz)
    h = open_handle(dz)
    assert h.cus_per_chain == 1 and h.clusters_per_chain == 1
    leg_a(name, h)
    h.close()


@pytest.mark.parametrize("name", list(cases.DESIGNS))
def test_chains_follow_the_oracle_on_one_workgroup_and_on_two(name):
    """Legs b to e."""
    dz, _, _, chains = cases.reference(name)
    cases.assert_preconditions(dz)
    cases.assert_real_trees(name, chains)
    data, variant = dz["data"], dz["variant"]
    m = OracleModel(data, variant)
    out = []
    for twin in (0, 0, 1):
        h = open_handle(dz, twin=twin)
        assert h.cus_per_chain == 1 and h.clusters_per_chain == 1 + twin
        h.init(); h.run(ROWS)
        d = h.draws().copy()
        assert d.shape == (2, ROWS, 7 + h.D)
        if not out:
            worst = 0.0
            for c, ref in enumerate(chains):
                if in_step(d[c], ref):
                    worst = max(worst, float(np.max(np.abs(d[c][:, 7:] - ref[:, 7:]) / (1e-7 / 1e-6 + np.abs(ref[:, 7:])))))
                    continue
                first = next(i for i in range(ROWS) if not in_step(d[c][i:i + 1], ref[i:i + 1]))
                print(f"{name} chain {c + 1}: out of step with the oracle's chain at row {first}; replaying every row from the device's previous one")
                adaptation_replayed_from_the_device_rows(data, variant, h, c, dz["seed"], [(0, ROWS)])
            print(f"{name}: the chains in step with the oracle's agree to {worst:.2e} (relative, atol / rtol = 0.1 added to the scale); {h.total_leapfrogs()} leapfrogs")
            # d. the rows the device builds from its draws
            full = h.write_array(0, h.n_cols, ROWS)
            assert np.array_equal(full, h.write_array(0, h.n_cols, ROWS))
            assert np.array_equal(full[:, :, :7], np.transpose(d[:, :, :7], (1, 0, 2)))
            wa = 0.0
            for it in (0, ROWS - 1):
                for c in (0, 1):
                    want = m.write_array(d[c, it, 7:])
                    wa = max(wa, float(np.max(np.abs(full[it, c, 7:] - want) / (1e-12 / 1e-11 + np.abs(want)))))
                    assert np.allclose(full[it, c, 7:], want, rtol=1e-11, atol=1e-12), (name, it, c)
            print(f"{name}: write_array to {wa:.2e}")
        out.append((d, h.adaptation()))
        h.close()
    (a, ada), (b, adb), (t, adt) = out
    assert np.isfinite(a).all()
    assert np.array_equal(a, b), ("the run does not repeat its bytes", np.argwhere(a != b)[:5])
    assert np.array_equal(a, t), ("two workgroups per chain", np.argwhere(a != t)[:5])
    for x in (adb, adt):
        assert np.array_equal(ada[0], x[0]) and np.array_equal(ada[1], x[1])


@pytest.mark.parametrize("name", list(cases.REFUSED))
def test_what_one_workgroup_cannot_hold_is_refused_and_a_cluster_runs_it(name):
    dz = cases.REFUSED[name]()
    cases.assert_preconditions(dz)
    for twin in (0, 1):
        with pytest.raises(sampler.PotusError, match="error 6: " + dz["refusal"] + r" \(the model is beyond the one-workgroup kernels"):
            open_handle(dz, twin=twin)
    h = open_handle(dz, cus=0)                      # the process is still usable: the library's own choice runs the same data
    assert h.cus_per_chain >= 8
    leg_a(name, h)
    if name == "T257":                              # a pooled entry point that needs the one-workgroup kernels says why it cannot run
        with pytest.raises(sampler.PotusError, match="error 6: potus_optimize: " + dz["refusal"]):
            h.optimize(paths=2)
        leg_a(name, h)                              # and leaves the handle as it was
    h.close()
