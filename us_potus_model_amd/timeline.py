"""The forecast timeline: every run date of a campaign fitted as the data sets of ONE handle and summarised per date on the device.

The reference's run scripts take RUN_DATE as their first parameter (final_2016.R:66-67) and are rerun as the campaign goes on.  The data
of two run dates differ in which polls exist, in mu_b_prior (final_2016.R:401) and in mu_b_T_scale (:337).  A poll that a date has not
seen is kept in the design with n_two_share = 0: it adds 0 to the log density and to the residual, its noise coordinate keeps its N(0,1)
prior, and so does the house effect of a pollster without a poll left -- the posterior has the same marginal on everything the scripts
report.  So the design of the LAST run date serves every date (dataprep.build_timeline checks that it does), and the dates are chains of
one launch (potus_set_datasets_ex, k_init_ds / k_run_ds), summarised by potus_timeline without a draws x columns block on the host.
DESIGN.md section 4i.

    design = dataprep.build_timeline(data_dir, 2016, ["2016-09-01", "2016-10-01", "2016-11-08"])
    tl = timeline.fit(design, "full", chains_per_date=4, num_warmup=1000, num_samples=1000)
    s = tl.summary(design["meta"]["ev_state"])          # s["state"][date, day, state, (low, high, mean, prob)]
    tl.outcomes(0, ev).win_probability()
"""
from __future__ import annotations

import numpy as np

from . import _abi
from .sampler import SCALE_NAMES, Handle, PotusError, device_diagnostics_of_block

_BATCHED = dict(cus_per_chain=1, twin=0)     # what potus_set_datasets_ex needs: one workgroup per chain
MAX_DRAWS = 16384                            # post-warm-up draws per date that potus_timeline sorts in LDS


def mask(data, keep_state, keep_national, mu_b_prior=None, mu_b_T_scale=None):
    """The plain `data` dict of one run date: polls outside the masks get n_two_share = n_democrat = 0; prior and scale replaced when given.
    A stand-alone Handle takes it."""
    ks, kn = np.asarray(keep_state, dtype=bool), np.asarray(keep_national, dtype=bool)
    if ks.shape != (int(data["N_state_polls"]),) or kn.shape != (int(data["N_national_polls"]),):
        raise ValueError(f"mask: keep_state {ks.shape} / keep_national {kn.shape} for {data['N_state_polls']} / {data['N_national_polls']} polls")
    d = dict(data)
    for name, k in (("state", ks), ("national", kn)):
        for f in ("n_two_share", "n_democrat"):
            d[f"{f}_{name}"] = np.where(k, np.asarray(data[f"{f}_{name}"], dtype=np.int32), 0).astype(np.int32)
    if mu_b_prior is not None:
        p = np.asarray(mu_b_prior, dtype=np.float64)
        if p.shape != (int(data["S"]),):
            raise ValueError(f"mask: mu_b_prior has shape {p.shape}")
        d["mu_b_prior"] = p.copy()
    if mu_b_T_scale is not None:
        d["mu_b_T_scale"] = float(mu_b_T_scale)
    return d


def design_of(data, keep_state, keep_national, mu_b_prior=None, mu_b_T_scale=None, run_dates=None, meta=None):
    """A timeline design from its parts (what dataprep.build_timeline returns, and what a fixture holds)."""
    ks, kn = np.atleast_2d(np.asarray(keep_state, dtype=bool)), np.atleast_2d(np.asarray(keep_national, dtype=bool))
    n = ks.shape[0]
    if kn.shape[0] != n:
        raise ValueError("design_of: keep_state and keep_national give different numbers of run dates")
    out = dict(data=data, meta=meta or {}, keep_state=ks, keep_national=kn, run_dates=list(run_dates) if run_dates is not None else list(range(n)),
               mu_b_prior=None if mu_b_prior is None else np.asarray(mu_b_prior, dtype=np.float64).reshape(n, int(data["S"])),
               mu_b_T_scale=None if mu_b_T_scale is None else np.asarray(mu_b_T_scale, dtype=np.float64).reshape(n))
    return out


def data_of(design, d):
    """The `data` dict of run date d of a design (mask applied; with the prior scales of setting d where the design has a grid of them,
    sensitivity.grid)."""
    out = mask(design["data"], design["keep_state"][d], design["keep_national"][d],
               None if design.get("mu_b_prior") is None else design["mu_b_prior"][d],
               None if design.get("mu_b_T_scale") is None else design["mu_b_T_scale"][d])
    if design.get("scales") is not None:
        out.update({name: float(v) for name, v in zip(SCALE_NAMES, design["scales"][d])})
    return out


def set_design(handle, design):
    """potus_set_datasets_ex with the masks, priors and scales of a design."""
    data = design["data"]
    ks, kn = design["keep_state"], design["keep_national"]
    n = ks.shape[0]
    arr = {}
    for name, k in (("state", ks), ("national", kn)):
        for f in ("n_two_share", "n_democrat"):
            arr[f"{f}_{name}"] = np.where(k, np.asarray(data[f"{f}_{name}"], dtype=np.int32)[None, :], 0).astype(np.int32)
    if design.get("scales") is not None:      # prior settings (sensitivity.grid): potus_set_datasets_grid
        handle.set_datasets_grid(design["scales"], n_democrat_state=arr["n_democrat_state"], n_democrat_national=arr["n_democrat_national"],
                                 n_two_share_state=arr["n_two_share_state"], n_two_share_national=arr["n_two_share_national"],
                                 mu_b_prior=design.get("mu_b_prior"), mu_b_T_scale=design.get("mu_b_T_scale"), n=n)
        return
    handle.set_datasets_ex(arr["n_democrat_state"], arr["n_democrat_national"], arr["n_two_share_state"], arr["n_two_share_national"],
                           design.get("mu_b_prior"), design.get("mu_b_T_scale"), n=n)


def lfo_masks(design):
    """(held_state, held_national) of leave-future-out: date d is scored on the polls date d + 1 keeps and date d does not; the last date on none."""
    out = []
    for k in (design["keep_state"], design["keep_national"]):
        h = np.zeros_like(k, dtype=bool)
        h[:-1] = k[1:] & ~k[:-1]
        out.append(h)
    return out[0], out[1]


class Timeline:
    """The fitted run dates of a design: `.handle` holds chains_per_date consecutive chains per date."""

    def __init__(self, handle, design, chains_per_date, wall_s=None):
        self.handle, self.design, self.chains_per_date, self.wall_s = handle, design, int(chains_per_date), wall_s
        self.n_dates = int(design["keep_state"].shape[0])
        self._w = np.asarray(design["data"]["state_weights"], dtype=np.float64)

    def _days(self, days):
        T = int(self.design["data"]["T"])
        return (T - 1, T) if days is None else (int(days[0]), int(days[1]))

    def summary(self, ev, days=None, ev_to_win=270, diagnostics=True):
        """potus_timeline over `days` = (begin, end), 0-based, default election day alone: dict(state [dates, days, S, 4], national
        [dates, days, 4], electoral_votes [dates, days, 5], n_draws [dates]) plus, per date, rhat_max and ess_bulk_min over the summarised
        cells (the state scores and the national vote of those days; potus_diagnostics_device on the date's slice; NaN for a failed date)."""
        h = self.handle
        t0, t1 = self._days(days)
        out = h.timeline(ev, (t0, t1), ev_to_win)
        out["timing"] = h.timeline_timing()
        if diagnostics:
            out["rhat_max"], out["ess_bulk_min"] = self.diagnostics((t0, t1), out["n_draws"])
        out["days"], out["run_dates"] = (t0, t1), list(self.design.get("run_dates", range(self.n_dates)))
        return out

    def diagnostics(self, days=None, n_draws=None):
        """(rhat_max, ess_bulk_min) per date over the state scores and the national vote of `days` (potus_diagnostics_device on the date's
        slice); NaN for a date whose n_draws is 0 (a failed chain) or with fewer than 4 draws per chain."""
        import torch
        x = self.handle.timeline_scores_device(self._days(days))                      # [dates, draws, days, S]
        w = torch.as_tensor(self._w / self._w.sum(), device=x.device)
        rh, es = np.full(self.n_dates, np.nan), np.full(self.n_dates, np.nan)
        per = x.shape[1] // self.chains_per_date
        for d in range(self.n_dates):
            if (n_draws is not None and n_draws[d] == 0) or per < 4:
                continue
            cells = torch.cat([x[d], (x[d] * w).sum(-1, keepdim=True)], dim=-1)        # [draws, days, S + 1]
            blk = cells.reshape(self.chains_per_date, per, -1).permute(1, 0, 2).contiguous()
            r, e = device_diagnostics_of_block(blk)
            rh[d], es[d] = float(np.nanmax(r)), float(np.nanmin(e))
        return rh, es

    def lfo(self, integrate=True):
        """Leave-future-out (Buerkner, Gabry, Vehtari 2020) on the fitted run dates, no refit: date d is scored on the polls that arrived
        before date d + 1 (lfo_masks), under its own draws, by one potus_cv_lpd call.  dict(elpd [dates] the sum over the date's held-out
        polls (0 where it holds none, NaN for a date with a failed chain), n_held [dates], lpd [dates, polls, 2] the pointwise log mean p
        and log mean p^2, NaN where not held out; n_draws [dates])."""
        hs, hn = lfo_masks(self.design)
        lpd, cnt = self.handle.cv_lpd(hs, hn, integrate)
        held = np.concatenate([hs, hn], axis=1)
        elpd = np.array([lpd[d, held[d], 0].sum() for d in range(self.n_dates)])
        return dict(elpd=elpd, n_held=held.sum(1), lpd=lpd, n_draws=cnt, run_dates=list(self.design.get("run_dates", range(self.n_dates))))

    def _block(self, d, days):
        if not 0 <= int(d) < self.n_dates:
            raise IndexError(f"run date {d} of {self.n_dates}")
        if self.handle.chain_status()[0][d * self.chains_per_date:(d + 1) * self.chains_per_date] != [0] * self.chains_per_date:
            raise PotusError(f"run date {d}: a chain of its fit failed (chain_status)")
        return self.handle.timeline_scores_device(days)[int(d)].contiguous()

    def outcomes(self, d, ev, actual=None, days=None, ev_to_win=270, states=None):
        """Joint election outcomes of run date d (potus_outcomes_device on its slice of the scores); days default: election day alone."""
        from .outcomes import outcomes_of_block
        days = self._days(days)
        o = outcomes_of_block(self._block(d, days), self._w, ev, actual=actual, ev_to_win=ev_to_win, states=states)
        o.days = days
        return o

    def scenario(self, d, ev=None, given=None, day=-1, days=None, ev_to_win=270, states=None):
        """Conditional forecast of run date d (potus_scenario_device on its slice); `day` indexes the range `days`."""
        from .scenario import scenario_of_block
        return scenario_of_block(self._block(d, self._days(days)), self._w, ev=ev, given=given, day=day, ev_to_win=ev_to_win, states=states)

    def forecast_scores(self, ev, actual, days=None, **kw):
        """Proper scoring rules of every run date's forecast against the result in one call (potus_forecast_scores_datasets): a ForecastScores
        whose scores are [dates, days, ...]; days default: election day alone.  A date with a failed chain has NaN scores and n_draws 0."""
        from .scoring import score_datasets
        return score_datasets(self.handle, ev, actual, days=self._days(days), **kw)

    def close(self):
        self.handle.close()


def fit(design, variant="full", chains_per_date=4, _cls=None, **opts):
    """Fit every run date of a design as chains of one launch.  opts: the sampler options of Handle (num_warmup, num_samples, seed, ...)."""
    import time
    n = int(design["keep_state"].shape[0])
    for k, v in _BATCHED.items():
        if opts.get(k, v) != v:
            raise ValueError(f"timeline.fit: {k} = {opts[k]} (the run dates are chains of one launch: {k} = {v})")
    o = dict(opts, **_BATCHED)
    h = Handle(design["data"], variant, chains=n * int(chains_per_date), **o)
    if int(chains_per_date) * h.opts.num_samples > MAX_DRAWS:
        h.close()
        raise ValueError(f"timeline.fit: {chains_per_date} chains x {h.opts.num_samples} draws per date (at most {MAX_DRAWS})")
    try:
        set_design(h, design)
        t0 = time.perf_counter()
        h.init()
        h.run(h.opts.num_warmup + h.opts.num_samples)
        wall = time.perf_counter() - t0
    except Exception:
        h.close()
        raise
    return (_cls or Timeline)(h, design, chains_per_date, wall)


def modes(design, variant="full", paths_per_date=1, device=0, seed=1843, init_radius=2.0, **opts):
    """The posterior mode of every run date of a design in ONE launch (potus_optimize on a potus_set_datasets_ex handle: batched
    L-BFGS, one workgroup per path), with the election-day predicted_score of every path from row_out -- built with the date's own
    model.  opts: the fields of potus_optimize_opts (jacobian, iter, history_size, tol_*, ...).  dict(q [dates, paths, D], lp,
    grad_norm, return_code, iterations, grad_evals [dates, paths], predicted_score [dates, paths, S], best [dates] the path with the
    highest lp among the date's converged ones, ms the kernel's time)."""
    n, k = int(design["keep_state"].shape[0]), int(paths_per_date)
    h = Handle(design["data"], variant, chains=n, num_warmup=0, num_samples=0, seed=int(seed), init_radius=float(init_radius), device=int(device),
               **_BATCHED)                                        # one chain per date carries the date's model; nothing is sampled
    try:
        set_design(h, design)
        S, T = int(design["data"]["S"]), int(design["data"]["T"])
        a = h.layout["predicted_score"][0]
        res = h.optimize(None, n * k, cols=(a + T - 1, a + T * (S - 1) + T), **opts)       # predicted_score is T x S column-major: day T of every state
        out = {key: res[key].reshape((n, k) + res[key].shape[1:]) for key in ("q", "lp", "grad_norm", "return_code", "iterations", "grad_evals")}
        out["predicted_score"] = np.ascontiguousarray(res["rows"][:, ::T]).reshape(n, k, S)
        ok = (out["return_code"] >= 1) & (out["return_code"] <= 5)
        out["best"] = np.array([int(np.argmax(np.where(ok[d] if ok[d].any() else np.isfinite(out["lp"][d]), out["lp"][d], -np.inf))) for d in range(n)])
        out["ms"] = h.optimize_timing()
        out["run_dates"] = list(design.get("run_dates", range(n)))
        return out
    finally:
        h.close()


def laplace(design, variant="full", draws=1000, ev=None, days=None, ev_to_win=270, jacobian=True, device=0, seed=1843, h=None):
    """The approximate forecast of a whole campaign without a sampler run: the modes of all run dates (modes(), tol_grad = 1e-2 as the only
    stopping rule), then ONE potus_laplace call on a potus_set_datasets_ex handle -- date d's Hessian, factor and `draws` draws with the
    date's own model -- and, with ev, the per-date summary of potus_laplace_summary over `days` (default: election day).  dict(mode [dates, D],
    return_code, log_det, grad_norm [dates], lp, lp_approx, log_ratio [dates, draws] (lp - lp(mode) - lp_approx; with jacobian = False up to a
    constant per date), optimize (what modes() returned), timing (laplace_timing), and with ev: state [dates, days, S, 4], national,
    electoral_votes, n_draws).  A date whose code is not 0 has NaN."""
    n = int(design["keep_state"].shape[0])
    if int(draws) < 1 or (ev is not None and int(draws) > MAX_DRAWS):
        raise ValueError(f"timeline.laplace: {draws} draws per date (1 .. {MAX_DRAWS} with a summary)")
    opt = modes(design, variant, paths_per_date=1, device=device, seed=seed, jacobian=int(bool(jacobian)), tol_obj=0.0, tol_rel_obj=0.0,
                tol_grad=1e-2, tol_rel_grad=0.0, tol_param=0.0)
    q = np.ascontiguousarray(opt["q"][:, 0])
    hd = Handle(design["data"], variant, chains=n, num_warmup=0, num_samples=0, seed=int(seed), device=int(device), **_BATCHED)
    try:
        set_design(hd, design)
        fields = dict(jacobian=int(bool(jacobian)))
        if h is not None:
            fields["h"] = float(h)
        res = hd.laplace(q, int(draws), **fields)
        out = dict(mode=q, return_code=res["return_code"], log_det=res["log_det"], grad_norm=res["grad_norm"], lp=res["lp"], lp_approx=res["lp_approx"],
                   log_ratio=res["lp"] - opt["lp"][:, :1] - res["lp_approx"], optimize=opt, timing=hd.laplace_timing(),
                   run_dates=list(design.get("run_dates", range(n))))
        if ev is not None:
            out.update(hd.laplace_summary(ev, days, ev_to_win))
        return out
    finally:
        hd.close()


def pathfinder(design, variant="full", draws=1000, paths_per_date=1, ev=None, days=None, ev_to_win=270, device=0, seed=1843, init_radius=2.0, **opts):
    """Pathfinder for every run date of a campaign in ONE potus_pathfinder call on a potus_set_datasets_ex handle: `paths_per_date` L-BFGS paths
    per date with the date's own model, the ELBO of every iterate, `draws` draws per path from the path's best iterate, and, with ev, the summary
    of potus_pathfinder_summary over `days` (default: election day) per path.  opts: Handle.pathfinder_opts' fields.  dict(lp, lq, log_ratio
    [dates, paths, draws], return_code, iterations, best_iteration, elbo [dates, paths], timing, and with ev: state [dates, paths, days, S, 4],
    national, electoral_votes, n_draws).  A path whose code is not 0 has NaN."""
    n, k = int(design["keep_state"].shape[0]), int(paths_per_date)
    if int(draws) < 1 or (ev is not None and int(draws) > MAX_DRAWS):
        raise ValueError(f"timeline.pathfinder: {draws} draws per path (1 .. {MAX_DRAWS} with a summary)")
    hd = Handle(design["data"], variant, chains=n, num_warmup=0, num_samples=0, seed=int(seed), init_radius=float(init_radius), device=int(device), **_BATCHED)
    try:
        set_design(hd, design)
        res = hd.pathfinder(None, n * k, num_draws=int(draws), **opts)
        best = res["best_iteration"]
        out = dict(lp=res["lp"].reshape(n, k, -1), lq=res["lq"].reshape(n, k, -1), log_ratio=(res["lp"] - res["lq"]).reshape(n, k, -1),
                   return_code=res["return_code"].reshape(n, k), iterations=res["iterations"].reshape(n, k), best_iteration=best.reshape(n, k),
                   elbo=np.array([res["elbo"][p, l] if l > 0 else np.nan for p, l in enumerate(best)]).reshape(n, k), timing=hd.pathfinder_timing(),
                   run_dates=list(design.get("run_dates", range(n))))
        if ev is not None:
            sm = hd.pathfinder_summary(ev, days, ev_to_win)
            out.update({key: v.reshape((n, k) + v.shape[1:]) for key, v in sm.items()})
        return out
    finally:
        hd.close()


def variational(design, variant="full", draws=1000, runs_per_date=1, ev=None, days=None, ev_to_win=270, device=0, seed=1843, init_radius=2.0, **opts):
    """Mean-field ADVI for every run date of a campaign in ONE potus_advi call on a potus_set_datasets_ex handle: `runs_per_date` runs per date
    with the date's own model, `draws` draws per run, and, with ev, the summary of potus_advi_summary over `days` (default: election day) per
    run.  opts: Handle.variational_opts' fields.  dict(lp, lq, log_ratio [dates, runs, draws], return_code, flags, iterations, eta, elbo
    [dates, runs] (the last one evaluated), timing, and with ev: state [dates, runs, days, S, 4], national, electoral_votes, n_draws).  A run
    without an approximation has NaN."""
    n, k = int(design["keep_state"].shape[0]), int(runs_per_date)
    if int(draws) < 1 or (ev is not None and int(draws) > MAX_DRAWS):
        raise ValueError(f"timeline.variational: {draws} draws per run (1 .. {MAX_DRAWS} with a summary)")
    hd = Handle(design["data"], variant, chains=n, num_warmup=0, num_samples=0, seed=int(seed), init_radius=float(init_radius), device=int(device), **_BATCHED)
    try:
        set_design(hd, design)
        res = hd.variational(None, n * k, output_samples=int(draws), **opts)
        out = dict(lp=res["lp"].reshape(n, k, -1), lq=res["lq"].reshape(n, k, -1), log_ratio=(res["lp"] - res["lq"]).reshape(n, k, -1),
                   return_code=res["return_code"].reshape(n, k), flags=res["flags"].reshape(n, k), iterations=res["iterations"].reshape(n, k),
                   eta=res["eta"].reshape(n, k), elbo=np.array([res["elbo"][r, j] for r, j in enumerate(res["evaluations"])]).reshape(n, k),
                   timing=hd.variational_timing(), run_dates=list(design.get("run_dates", range(n))))
        if ev is not None:
            sm = hd.variational_summary(ev, days, ev_to_win)
            out.update({key: v.reshape((n, k) + v.shape[1:]) for key, v in sm.items()})
        return out
    finally:
        hd.close()


def save_fixture(path, design):
    """The per-date part of a design (masks, priors, scales, dates) as one .npz: data only."""
    np.savez_compressed(path, keep_state=np.packbits(design["keep_state"], axis=1), keep_national=np.packbits(design["keep_national"], axis=1),
                        n_state=np.int64(design["keep_state"].shape[1]), n_national=np.int64(design["keep_national"].shape[1]),
                        mu_b_prior=design["mu_b_prior"], mu_b_T_scale=design["mu_b_T_scale"], run_dates=np.asarray([str(x) for x in design["run_dates"]]))


def load_fixture(path, data, meta=None):
    """The design of a fixture written by save_fixture, on the `data` of its last run date."""
    z = np.load(path, allow_pickle=False)
    ks = np.unpackbits(z["keep_state"], axis=1, count=int(z["n_state"])).astype(bool)
    kn = np.unpackbits(z["keep_national"], axis=1, count=int(z["n_national"])).astype(bool)
    return design_of(data, ks, kn, z["mu_b_prior"], z["mu_b_T_scale"], [str(x) for x in z["run_dates"]], meta)
