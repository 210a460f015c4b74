#!/usr/bin/env python3
"""Development (GPU box): sha256 of everything the kernels that rebuild an output row produce, with the library POTUS_LIB selects -- two
builds that claim the same row arithmetic must print the same lines (the fits are the sampler's kernels, so the draws are the same).

    POTUS_LIB=build/variants/libpotus_parent.so python scripts/dev/row_digest.py > parent.txt
    python scripts/dev/row_digest.py > new.txt && diff parent.txt new.txt

synthetic.small in both variants; 4 chains x 140 saved draws = 560 rows, so the grid-stride loops of the 512-workgroup grids wrap."""
import hashlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from us_potus_model_amd import Handle, _abi, synthetic  # noqa: E402

import torch  # noqa: E402
torch.cuda.init()          # torch's GPU runtime comes up before the library's first call, as in bench.py and the tests

NW, NS, SEED = 20, 140, 1843
OPTS = dict(chains=4, num_warmup=NW, num_samples=NS, seed=SEED, cus_per_chain=1, twin=0)


def show(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    print(f"{name} {h.hexdigest()}", flush=True)


def fitted(data, variant, prepare=None):
    h = Handle(data, variant, **OPTS)
    if prepare:
        prepare(h)
    h.init()
    h.run(NW + NS)
    assert h.chain_status()[0] == [0] * 4, h.chain_status()
    return h


def log_lik(h, p0, p1, integrate):
    t = torch.empty((p1 - p0, h.opts.chains, h.post_warmup_saved()), dtype=torch.float64, device=f"cuda:{h.opts.device}")
    return h.log_lik_device(p0, p1, t, integrate=integrate).cpu().numpy()


outcomes = {}
for variant in ("full", "no_mode_adjustment"):
    data = synthetic.small(variant)
    Ns, Nn, S = int(data["N_state_polls"]), int(data["N_national_polls"]), int(data["S"])
    # ---- a plain handle
    h = fitted(data, variant)
    lay, ncols = h.layout, h.n_cols
    show(f"{variant} draws", h.draws())
    show(f"{variant} write_array all", h.write_array(0, ncols, NS))
    a, b = lay["mu_b"][0] + 3, lay["predicted_score"][0] + 5                  # starts and ends inside blocks
    show(f"{variant} write_array [{a},{b})", h.write_array(a, b, NS))
    show(f"{variant} constrain", h.constrain(h.draws()[1, 5:12, 7:]))
    q_sim, ys, yn = h.simulate_prior(SEED, 3, sim_offset=5)
    outcomes[variant] = (ys, yn)
    show(f"{variant} simulate_prior q", q_sim)
    show(f"{variant} simulate_prior y_state", ys)
    show(f"{variant} simulate_prior y_national", yn)
    for integrate in (False, True):
        show(f"{variant} log_lik polls [{Ns - 3},{Ns + 2}) integrate={int(integrate)}", log_lik(h, Ns - 3, Ns + 2, integrate))
    show(f"{variant} optimize rows, one data set", h.optimize(paths=2, cols=(0, ncols), iter=40)["rows"])
    truth = h.constrain(q_sim[:2])                                            # [2, ncols - 7]
    h.close()
    # ---- potus_set_datasets: 2 data sets x 2 chains that differ in the outcomes
    g = fitted(data, variant, lambda g: g.set_datasets(ys[:2], yn[:2]))
    less, equal, L = g.sbc_ranks(truth, 7, ncols, thin=3)
    show(f"{variant} sbc_ranks thin=3 (L={L})", less, equal)
    show(f"{variant} optimize rows, set_datasets", g.optimize(paths=4, cols=(0, ncols), iter=40)["rows"])
    g.close()
    # ---- potus_set_datasets_ex: 2 data sets x 2 chains with priors of their own; the second has not seen every third poll
    prior = np.tile(np.asarray(data["mu_b_prior"], dtype=np.float64), (2, 1))
    prior[1] += np.linspace(-0.3, 0.4, S)
    keep_s, keep_n = np.ones((2, Ns), bool), np.ones((2, Nn), bool)
    keep_s[1, ::3] = False
    keep_n[1, ::3] = False
    n2s, n2n = np.asarray(data["n_two_share_state"], np.int32), np.asarray(data["n_two_share_national"], np.int32)
    nds, ndn = np.asarray(data["n_democrat_state"], np.int32), np.asarray(data["n_democrat_national"], np.int32)
    e = fitted(data, variant, lambda e: e.set_datasets_ex(np.where(keep_s, nds, 0), np.where(keep_n, ndn, 0), np.where(keep_s, n2s, 0),
                                                         np.where(keep_n, n2n, 0), prior, np.array([float(data["mu_b_T_scale"]), 0.2])))
    show(f"{variant} set_datasets_ex draws", e.draws())
    show(f"{variant} set_datasets_ex write_array all", e.write_array(0, ncols, NS))
    held_s, held_n = ~keep_s, ~keep_n
    held_s[0, [0, Ns - 1]] = True                                               # in-sample pairs too: a state poll and a national poll
    held_n[0, 0] = True
    assert held_s[1].any() and held_n[1].any()
    for integrate in (False, True):
        show(f"{variant} cv_log_lik integrate={int(integrate)}", e.cv_log_lik_device(held_s, held_n, integrate=integrate).cpu().numpy())
    show(f"{variant} optimize rows, set_datasets_ex", e.optimize(paths=4, cols=(a, b), iter=40)["rows"])
    e.close()

# ---- every sampler: draws and adaptation of a short warm-up that holds one window end (30 warm-up iterations: buffers 4 | 23 | 3)
data = synthetic.small("full")
SAMPLERS = [("one workgroup", dict(cus_per_chain=1, twin=0)), ("two workgroups", dict(cus_per_chain=1, twin=1)),
            ("cluster of 4", dict(cus_per_chain=4, twin=0)), ("two clusters of 4", dict(cus_per_chain=4, twin=1)),
            ("dense_e", dict(metric=_abi.METRICS["dense_e"], cus_per_chain=1)), ("set_datasets 2 x 1", dict(cus_per_chain=1, twin=0))]
for name, kw in SAMPLERS:
    h = Handle(data, "full", chains=2, num_warmup=30, num_samples=10, save_warmup=1, seed=SEED, **kw)
    if name.startswith("set_datasets"):
        h.set_datasets(outcomes["full"][0][:2], outcomes["full"][1][:2])
    h.init()
    h.run(40)
    assert h.chain_status()[0] == [0, 0], (name, h.chain_status())
    show(f"sampler {name} draws", h.draws())
    show(f"sampler {name} adaptation", *h.adaptation())
    h.close()
