"""potus_e_loo on a fit (loo.influence, loo.predict): what leaving each poll out does to the forecast and what the
model expected of each poll, against the numpy restatement (tests/eloo_ref.py) fed with the fit's own log-likelihood block and output
columns; the days form against the one-day form; two handles against one; exact refits; refusals; the .C() entries.  The fits are test_gpu_loo.py's: synthetic.small, both variants, 4 chains, 300 + 500, one workgroup per chain."""
import ctypes as C

import numpy as np
import pytest

import eloo_ref as ref
import psis_ref
from conftest import second_device
from loo_mm_ref import psis_general
from test_gpu_loo import NS, NW, SEED, VARIANTS, _close, _columns as _cols, _fit, _log_lik, _polls
from us_potus_model_amd import loo as loo_mod, synthetic
from us_potus_model_amd.sampler import Handle, PotusError, run_many

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def fits():
    out = {v: _fit(synthetic.small(v), v) for v in VARIANTS}
    yield out
    for h in out.values():
        h.close()


def _ev(S):
    ev = 3 + (7 * np.arange(S)) % 11
    return ev.astype(float), int(ev.sum()) // 2 + 1


def _columns(h, t, ev, ev_to_win):
    """the 2 S + 3 forecast columns of day t from the predicted_score columns of write_array: [2 S + 3, chains, draws]"""
    S, T = int(h.data["S"]), int(h.data["T"])
    a, b, _ = h.layout["predicted_score"]
    n = h.draws_saved()
    ps = h.write_array(a, b, n)[n - h.post_warmup_saved():].reshape(-1, h.opts.chains, S, T)[..., t].transpose(1, 0, 2)   # [chain, draw, S]
    w = np.asarray(h.data["state_weights"], dtype=float)
    w = w / w.sum()
    won = (ps > 0.5).astype(float)
    evs = won @ ev
    cols = [ps[..., s] for s in range(S)] + [ps @ w] + [won[..., s] for s in range(S)] + [(evs >= ev_to_win).astype(float), evs]
    return np.stack(cols)


@pytest.mark.parametrize("variant", VARIANTS)
def test_influence_equals_the_restatement_on_the_fits_own_blocks(fits, variant):
    h = fits[variant]
    S, T = int(h.data["S"]), int(h.data["T"])
    ev, win = _ev(S)
    inf = h.loo_influence(ev, ev_to_win=win)
    ll = _log_lik(h, True)
    r = -ll
    re = np.array([psis_ref.relative_eff(ll[i]) for i in range(ll.shape[0])])
    lw = np.stack([psis_general(r[i], re[i])[0].reshape(ll.shape[1:]) for i in range(ll.shape[0])])
    X = _columns(h, T - 1, ev, win)
    mean, var, ess, kh = ref.e_loo_shared(X, lw, r, re, diag=True)
    post = X.reshape(X.shape[0], -1).mean(axis=1)
    print(f"{variant}: {ll.shape[0]} polls, largest |delta| national {np.abs(inf.delta[:, S]).max():.2e}, ec_win {np.abs(inf.delta[:, 2 * S + 1]).max():.2e}; "
          f"k <= threshold for {(inf.pareto_k <= inf.k_threshold()).sum()} polls; stages {np.round(inf.ms, 3)} ms")
    _close(inf.loo_mean, mean)
    _close(inf.post_mean, post)
    _close(inf.delta, mean - post[None])
    _close(inf.sd, np.sqrt(var))
    _close(inf.ess, ess)
    _close(inf.khat, kh)
    lo = loo_mod.loo([h], integrate=True)
    assert inf.pareto_k.tobytes() == lo.pareto_k.tobytes()
    _close(inf.pareto_k, psis_ref.loo_pointwise(ll)[:, 3])
    assert len(inf.columns) == 2 * S + 3 and inf.columns[S] == "national" and inf.columns[-2:] == ["ec_win", "ev"]
    # the indicator columns take the k of the ratios; leaving a poll out does move the forecast
    assert np.array_equal(inf.khat[:, 2 * S + 1], inf.khat[:, S + 1]) and np.abs(inf.delta[:, S]).max() > 1e-5
    top = inf.top("national", 5)
    assert len(top) == 5 and all(k <= inf.k_threshold() for _, _, k in top)
    assert [abs(d) for _, d, _ in top] == sorted([abs(d) for _, d, _ in top], reverse=True)
    ok = inf.pareto_k <= inf.k_threshold()
    assert abs(top[0][1]) == np.abs(inf.delta[ok, S]).max()
    again = h.loo_influence(ev, ev_to_win=win)
    assert again.delta.tobytes() == inf.delta.tobytes() and again.khat.tobytes() == inf.khat.tobytes()
    plain = h.loo_influence(ev, ev_to_win=win, integrate=False, diag=False)
    assert plain.khat is None and plain.pareto_k.tobytes() == loo_mod.loo([h], integrate=False).pareto_k.tobytes()


def test_influence_over_days_agrees_with_the_one_day_call(fits):
    h = fits["full"]
    S, T = int(h.data["S"]), int(h.data["T"])
    ev, win = _ev(S)
    one = h.loo_influence(ev, ev_to_win=win, diag=False)
    many = h.loo_influence(ev, ev_to_win=win, days=(T - 3, T), diag=False)
    assert many.delta_days.shape == (h.n_polls, 3, S + 1)
    _close(many.delta_days[:, -1], one.delta[:, :S + 1])
    _close(many.loo_mean_days[:, -1], one.loo_mean[:, :S + 1])
    early = h.loo_influence(ev, ev_to_win=win, day=T - 3, diag=False)
    _close(many.delta_days[:, 0], early.delta[:, :S + 1])


def test_two_handles_of_two_chains_give_the_bytes_of_one_handle_of_four(fits):
    h = fits["full"]
    d = synthetic.small("full")
    a = Handle(d, "full", chains=2, num_warmup=NW, num_samples=NS, seed=SEED, cus_per_chain=1, twin=0)
    b = Handle(d, "full", chains=2, chain_id_offset=2, device=second_device(), num_warmup=NW, num_samples=NS, seed=SEED, cus_per_chain=1, twin=0)
    a.init()
    b.init()
    run_many([a, b], NW + NS)
    ev, win = _ev(int(d["S"]))
    one, two = loo_mod.influence([h], ev, ev_to_win=win), loo_mod.influence([a, b], ev, ev_to_win=win)
    for k in ("delta", "loo_mean", "post_mean", "pareto_k", "khat", "ess"):
        assert getattr(one, k).tobytes() == getattr(two, k).tobytes(), k
    a.close()
    b.close()


# ---- what the model expected of each poll
def _eta_z(h):
    """(eta without the noise term, sigma, z) per poll, chain, draw from the logit_pi_* and raw_measure_noise_* columns"""
    _, _, sig = _polls(h.data)
    n = h.draws_saved() - h.post_warmup_saved()
    z = _cols(h, "raw_measure_noise_state", "raw_measure_noise_national")[:, :, n:]
    lp = _cols(h, "logit_pi_democrat_state", "logit_pi_democrat_national")[:, :, n:]
    return lp - sig[:, None, None] * z, sig[:, None, None], z


@pytest.mark.parametrize("integrate", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_poll_share_equals_the_restatement_on_the_row_columns(fits, variant, integrate):
    h = fits[variant]
    eta, sig, z = _eta_z(h)
    a1, a2 = ref.poll_share(eta, sig, z, integrate)
    g1, g2 = (t.cpu().numpy() for t in h.poll_share_device(0, h.n_polls, integrate=integrate))
    e1, e2 = np.abs(g1 - a1).max(), np.abs(g2 - a2).max()
    print(f"{variant} integrate={integrate}: largest |device - restatement| a1 {e1:.2e}, a2 {e2:.2e}")
    assert e1 < 1e-12 and e2 < 1e-12          # shares in (0, 1): eta is rebuilt from the row to ~1e-13 (test_gpu_loo's 1e-9 on log-likelihoods of n ~ 1e3)
    b1, b2 = (t.cpu().numpy() for t in h.poll_share_device(3, 7, integrate=integrate))
    assert b1.tobytes() == g1[3:7].tobytes() and b2.tobytes() == g2[3:7].tobytes()
    if not integrate:
        assert np.array_equal(g2, g1 * g1)


@pytest.mark.parametrize("integrate", [False, True])
def test_predict_equals_the_restatement(fits, integrate):
    h = fits["full"]
    y, n, _ = _polls(h.data)
    eta, sig, z = _eta_z(h)
    a1, a2 = ref.poll_share(eta, sig, z, integrate)
    ll = _log_lik(h, integrate)
    re = np.array([psis_ref.relative_eff(ll[i]) for i in range(ll.shape[0])])
    o1, k1 = ref.e_loo(a1, -ll, (), re)
    o2, _ = ref.e_loo(a2, -ll, (), re)
    var = ref.predict_var(o1[:, 0], o2[:, 0], n)
    p = h.loo_predict(integrate=integrate)
    print(f"integrate={integrate}: sd of z {p.z.std():.2f}, largest |z| {np.abs(p.z).max():.2f}, largest |LOO mean - in-sample mean| {np.abs(p.mean - p.in_sample_mean).max():.2e}")
    _close(p.mean, o1[:, 0])
    _close(p.variance, var)
    _close(p.sd, np.sqrt(var))
    _close(p.pareto_k, k1[:, 0])
    _close(p.in_sample_mean, a1.reshape(a1.shape[0], -1).mean(axis=1))
    _close(p.residual, y / n - o1[:, 0])
    _close(p.z, (y / n - o1[:, 0]) / np.sqrt(var))
    mz, cnt = p.by_pollster()
    pol = np.concatenate([np.asarray(h.data["poll_state"]), np.asarray(h.data["poll_national"])]) - 1
    assert cnt.sum() == len(y) and np.array_equal(cnt, np.bincount(pol, minlength=cnt.size))
    j = int(np.argmax(cnt))
    assert abs(mz[j] - p.z[pol == j].mean()) < 1e-12


def test_pooling_in_several_blocks_gives_the_bytes_of_one_block(fits, monkeypatch):
    h = fits["full"]
    ev, win = _ev(int(h.data["S"]))
    T = int(h.data["T"])
    one, p1 = h.loo_influence(ev, ev_to_win=win, days=(T - 2, T)), h.loo_predict()
    monkeypatch.setenv("POTUS_ELOO_BLOCK_POLLS", "24")                     # 95 polls: four blocks, the last of 23
    many, p2 = h.loo_influence(ev, ev_to_win=win, days=(T - 2, T)), h.loo_predict()
    for k in ("delta", "variance", "pareto_k", "khat", "ess", "delta_days"):
        assert getattr(one, k).tobytes() == getattr(many, k).tobytes(), k
    for k in ("mean", "variance", "pareto_k", "in_sample_mean", "k_ratios"):
        assert getattr(p1, k).tobytes() == getattr(p2, k).tobytes(), k


def test_dot_c_entries_give_the_bytes_of_the_c_call(fits):
    h = fits["full"]
    S, N = int(h.data["S"]), h.n_polls
    ev, win = _ev(S)
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    p = lambda a: a.ctypes.data_as(DP)
    ids, one = (C.c_int * 1)(h.h), C.byref(C.c_int(1))
    for diag in (1, 0):
        inf = h.loo_influence(ev, ev_to_win=win, diag=bool(diag))
        NC = 2 * S + 3
        mean, var, post, k, ess, kh, st = np.zeros((N, NC)), np.zeros((N, NC)), np.zeros(NC), np.zeros(N), np.zeros(N), np.zeros((N, NC)), C.c_int(-1)
        h.L.potus_R_loo_influence(ids, one, (C.c_int * 4)(1, win, -1, diag), p(np.ascontiguousarray(ev)), p(mean), p(var), p(post), p(k), p(ess), p(kh), C.byref(st))
        assert st.value == 0
        assert mean.tobytes() == inf.loo_mean.tobytes() and var.tobytes() == inf.variance.tobytes() and post.tobytes() == inf.post_mean.tobytes()
        assert k.tobytes() == inf.pareto_k.tobytes() and ess.tobytes() == inf.ess.tobytes()
        assert kh.tobytes() == inf.khat.tobytes() if diag else not kh.any()
    for integrate in (1, 0):
        pr = h.loo_predict(integrate=bool(integrate))
        o, k, st = np.zeros((N, 5)), np.zeros(N), C.c_int(-1)
        h.L.potus_R_loo_predict(ids, one, C.byref(C.c_int(integrate)), p(o), p(k), C.byref(st))
        assert st.value == 0 and o[:, 0].tobytes() == pr.mean.tobytes() and o[:, 2].tobytes() == pr.sd.tobytes() and o[:, 3].tobytes() == pr.pareto_k.tobytes()
        assert k.tobytes() == pr.k_ratios.tobytes()
    st = C.c_int(0)
    h.L.potus_R_loo_predict(ids, one, C.byref(C.c_int(2)), p(o), p(k), C.byref(st))
    assert st.value == 1


def test_handle_level_refusals(fits):
    """handles with data sets, and fewer than four post-warm-up draws per chain: the library's codes (4: state, 1: argument), before any E_loo kernel"""
    data = synthetic.small("full")
    ev, win = _ev(int(data["S"]))
    m = Handle(data, "full", chains=2, num_warmup=5, num_samples=5, cus_per_chain=1, twin=0)
    ys, yn = np.asarray(data["n_democrat_state"])[None], np.asarray(data["n_democrat_national"])[None]
    m.set_datasets(np.repeat(ys, 2, 0), np.repeat(yn, 2, 0))
    m.init()
    m.run(10)
    for call in (lambda: m.loo_influence(ev, ev_to_win=win), lambda: m.loo_predict(), lambda: m.poll_share_device(0, 1)):
        with pytest.raises(PotusError, match="error 4.*slice the chains per data set"):
            call()
    e = Handle(data, "full", chains=2, num_warmup=5, num_samples=3, cus_per_chain=1, twin=0)
    e.init()
    e.run(8)
    for call in (lambda: e.loo_influence(ev, ev_to_win=win), lambda: e.loo_predict()):
        with pytest.raises(PotusError, match="error 4.*at least four"):
            call()
    h = fits["full"]
    import torch
    t = torch.zeros(8, dtype=torch.float64, device="cuda:0")
    p = C.c_void_p(t.data_ptr())
    for b0, b1, ig in ((-1, 3, 1), (0, h.n_polls + 1, 1), (3, 3, 1), (0, 1, 2)):
        assert h.L.potus_poll_share_device(h.h, b0, b1, ig, p, p) == 1
    with pytest.raises(PotusError, match="error 1.*listed twice"):
        loo_mod.influence([h, h], ev)
    with pytest.raises(PotusError, match="error 1.*another posterior"):
        loo_mod.predict([h, fits["no_mode_adjustment"]])
    o, k = np.zeros((h.n_polls, 5)), np.zeros(h.n_polls)
    DP = C.POINTER(C.c_double)
    for integrate, what in ((2, 0), (1, 2), (1, -1)):
        assert h.L.potus_e_loo((C.c_int * 1)(h.h), 1, integrate, what, None, 0, -1, 0, 0, 0, o.ctypes.data_as(DP), None, None, k.ctypes.data_as(DP), None, None, None, None) == 1
    assert h.L.potus_e_loo((C.c_int * 1)(h.h), 1, 1, 1, None, 0, -1, 0, 0, 0, o.ctypes.data_as(DP), None, None, k.ctypes.data_as(DP), None, None, None, None) == 1   # influence without ev
    assert not o.any() and not k.any()
    c = Handle(data, "full", chains=2, num_warmup=5, num_samples=5, cus_per_chain=4)      # a cluster-layout handle: refused before it is counted
    with pytest.raises(PotusError, match="one workgroup per chain"):
        c.loo_influence(ev, ev_to_win=win)
    c.close()
    m.close()
    e.close()


def test_influence_agrees_with_exact_refits_of_the_most_influential_polls(fits):
    """Among the polls with k <= 0.5 the four with the largest |delta| of the national vote are each held out of a refit (n_two_share = 0),
    four data sets of one handle in one launch (the machinery of crossval).  Each refit's election-day national mean against post_mean + delta
    within 5 combined standard errors: the refit's MCSE (potus_monitor) and the estimate's sd_loo / sqrt(ess), added in quadrature.
    Fewer than four such polls: a failure, not a pass."""
    import torch
    from us_potus_model_amd import timeline
    from us_potus_model_amd.monitor import monitor_of_block
    h = fits["full"]
    data = h.data
    S, Ns = int(data["S"]), int(data["N_state_polls"])
    ev, win = _ev(S)
    inf = h.loo_influence(ev, ev_to_win=win, diag=False)
    cand = np.flatnonzero(inf.pareto_k <= 0.5)
    assert cand.size >= 4, f"only {cand.size} polls with k <= 0.5"
    # the seed's suitability by the restatement on the dumped log-likelihood block: the same candidates, at least four of them
    k_ref = psis_ref.loo_pointwise(_log_lik(h, True))[:, 3]
    assert np.array_equal(np.flatnonzero(k_ref <= 0.5), cand) and np.abs(k_ref - 0.5).min() > 1e-6
    pick = cand[np.argsort(-np.abs(inf.delta[cand, S]), kind="stable")[:4]]
    keep = np.ones((4, h.n_polls), dtype=bool)
    keep[np.arange(4), pick] = False
    tl = timeline.fit(timeline.design_of(data, keep[:, :Ns], keep[:, Ns:]), "full", chains_per_date=4, num_warmup=NW, num_samples=NS, seed=SEED + 1)
    try:
        assert tl.handle.chain_status()[0] == [0] * 16
        x = tl.handle.timeline_scores_device()                            # [4, draws, 1, S], a data set's draws chain after chain
        w = np.asarray(data["state_weights"], dtype=float)
        w = torch.as_tensor(w / w.sum(), device=x.device)
        nat = (x[:, :, 0, :] @ w).reshape(4, 4, NS)                       # [data set, chain, draw]
        misses = []
        for d, i in enumerate(pick):
            mon = monitor_of_block(nat[d].T[:, :, None].contiguous())
            m, mcse = float(mon.column("mean")[0]), float(mon.column("mcse_mean")[0])
            est, se = inf.post_mean[S] + inf.delta[i, S], inf.sd[i, S] / np.sqrt(inf.ess[i])
            comb = np.sqrt(mcse ** 2 + se ** 2)
            print(f"poll {i}: k {inf.pareto_k[i]:.2f}, delta {inf.delta[i, S]:+.2e}, E_loo {est:.5f}, refit {m:.5f} (posterior {inf.post_mean[S]:.5f}), "
                  f"difference {abs(m - est) / comb:.2f} combined standard errors ({comb:.1e})")
            if not abs(m - est) <= 5 * comb:
                misses.append(int(i))
        assert not misses, misses
    finally:
        tl.close()
