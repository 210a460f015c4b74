"""Prior sensitivity by refit: a grid of prior scales fitted as the data sets of ONE handle and compared with the baseline on the device.

The model has nine hand-set prior scales (sampler.SCALE_NAMES).  How much a forecast depends on them is asked by refitting with other
values -- the reference's authors did (scripts/deprecated/R/Refactored/poll_run_v7_test_sigma.R:273-366, a 3 x 3 grid of two sigmas scored
with loo()), and reweighting the baseline's draws is no substitute here (D = 15 098 coordinates: a few effective draws under the weights).
A setting is a data set of potus_set_datasets_grid: chain c of the handle holds the bytes of a stand-alone handle on the setting's data.
How far a setting's forecast lies from the baseline's is measured per column by three distances between the two sets of draws
(potus_grid_compare, potus_sens.hpp): Wasserstein-1, Kolmogorov-Smirnov and the cumulative Jensen-Shannon distance that Kallioinen et al.
(2023) use for power-scaling sensitivity.  A second copy of the baseline with other chains gives the Monte-Carlo floor of each.
DESIGN.md section 4t.

    design = sensitivity.grid(data, {"sigma_c": [0.5, 2], "mu_b_T_scale": [0.5, 2]})
    g = sensitivity.fit(design, "full", chains_per_setting=4, num_warmup=1000, num_samples=1000)
    c = g.compare(ev)                 # c.cjs[setting, day, column]; c.table(); c.flag()
    loo.loo_compare(*g.loo())
"""
from __future__ import annotations

import itertools

import numpy as np

from . import timeline
from .sampler import N_SCALES, SCALE_NAMES, PotusError

KINDS = ("state", "national", "electoral_votes")


def scales_of(data):
    """The nine scales of a data dict, in the order of SCALE_NAMES (0 where the data has none: the no-mode variant's sigma_m, sigma_pop,
    sigma_e_bias, which the library ignores)."""
    return np.array([float(data.get(name, 0.0) or 0.0) for name in SCALE_NAMES])


def grid(data, scales=None, product=False, null=True):
    """A design of prior settings: a timeline design (every poll kept in every setting) plus scales [n, 9], labels [n], factors [n, 9] (the
    multiplier of every scale, 1 where it is the data's own), null (the index of the null copy, or None) and varied (per setting the index of
    the one scale it changes, -1 for the baseline, the null copy and settings that change several).
    scales: {name: [factor, ...]} multiplies the data's own value of the scale.  Setting 0 is the data as given.  With null = True setting 1 is
    a second copy of it with other chains: its distance to setting 0 is the Monte-Carlo floor at the same sample size.  After that comes one
    setting per (scale, factor), in the order given; product = True builds the full factorial of the factor lists instead (a factor of 1
    included where listed)."""
    scales = dict(scales or {})
    for name, fs in scales.items():
        if name not in SCALE_NAMES:
            raise ValueError(f"sensitivity.grid: {name!r} is not a prior scale ({', '.join(SCALE_NAMES)})")
        for f in np.atleast_1d(fs):
            if not (np.isfinite(f) and f > 0):
                raise ValueError(f"sensitivity.grid: factor {f} of {name} (positive and finite expected)")
    base = scales_of(data)
    rows, labels = [np.ones(N_SCALES)], ["baseline"]
    if null:
        rows.append(np.ones(N_SCALES)); labels.append("null copy")
    names = list(scales)
    if product:
        for combo in itertools.product(*[np.atleast_1d(scales[nm]) for nm in names]):
            f = np.ones(N_SCALES)
            for nm, v in zip(names, combo):
                f[SCALE_NAMES.index(nm)] = float(v)
            rows.append(f); labels.append(", ".join(f"{nm} x {float(v):g}" for nm, v in zip(names, combo)))
    else:
        for nm in names:
            for v in np.atleast_1d(scales[nm]):
                f = np.ones(N_SCALES)
                f[SCALE_NAMES.index(nm)] = float(v)
                rows.append(f); labels.append(f"{nm} x {float(v):g}")
    factors = np.stack(rows)
    n = factors.shape[0]
    Ns, Nn = int(data["N_state_polls"]), int(data["N_national_polls"])
    design = timeline.design_of(data, np.ones((n, Ns), bool), np.ones((n, Nn), bool), run_dates=labels)
    changed = factors != 1.0
    design.update(scales=factors * base[None, :], labels=labels, factors=factors, null=1 if null else None,
                  varied=np.where(changed.sum(1) == 1, changed.argmax(1), -1))
    return design


class Comparison:
    """Grid.compare's result.  w1, ks, cjs [settings, days, S + 2]: the columns are the S state scores, the national vote and the electoral
    votes of a draw (kind_of_column names the kind of each).  floor [3, days, S + 2]: the null copy's w1, ks, cjs (None without one).
    sensitivity [settings, days, S + 2] = cjs / |log2 factor| for the settings that change one scale, NaN for the others."""

    def __init__(self, distance, n_draws, design, days, base):
        self.distance, self.n_draws, self.design, self.days, self.base = distance, n_draws, design, days, int(base)
        self.w1, self.ks, self.cjs = distance[..., 0], distance[..., 1], distance[..., 2]
        S = distance.shape[2] - 2
        self.kind_of_column = np.array([0] * S + [1, 2])
        null = design.get("null")
        self.floor = None if null is None else np.moveaxis(distance[null], -1, 0)
        self.sensitivity = sensitivity_of(self.cjs, design["factors"], design["varied"])

    def floor_of_kind(self, what="cjs"):
        """The largest value of the null copy's distance over the columns of each kind, [days, 3 kinds]; zeros without a null copy."""
        nd = self.distance.shape[1]
        if self.floor is None:
            return np.zeros((nd, 3))
        f = self.floor[("w1", "ks", "cjs").index(what)]
        return np.stack([f[:, self.kind_of_column == k].max(1) for k in range(3)], axis=1)

    def flag(self, threshold=0.05):
        """[settings, days, S + 2] bool: the sensitivity of a one-at-a-time setting (its cjs for a setting that changes several scales) is at
        least `threshold` (Kallioinen et al.'s default) AND its cjs exceeds the largest floor of the column's kind on that day.  The baseline
        and the null copy are never flagged; NaN (a failed setting) is not flagged."""
        return flag_of(self.cjs, self.sensitivity, self.floor_of_kind("cjs"), self.kind_of_column, self.base, self.design.get("null"), threshold)

    def table(self, day=-1, threshold=0.05):
        """One line per setting for day `day` of the compared range: the largest state cjs, the national and the electoral-vote cjs, the
        largest sensitivity, and which kinds are flagged."""
        fl = self.flag(threshold)[:, day]
        k = self.kind_of_column
        lines = [f"{'setting':44s}{'cjs state':>10s}{'cjs natl':>10s}{'cjs EV':>10s}{'w1 natl':>10s}{'sens':>8s}  flagged"]
        for d, lab in enumerate(self.design["labels"]):
            c, s = self.cjs[d, day], self.sensitivity[d, day]
            what = [KINDS[j] for j in range(3) if fl[d][k == j].any()]
            sens = np.nanmax(s) if np.isfinite(s).any() else np.nan
            lines.append(f"{lab:44s}{np.max(c[k == 0]):10.4f}{c[k == 1][0]:10.4f}{c[k == 2][0]:10.4f}{self.w1[d, day][k == 1][0]:10.5f}{sens:8.3f}  "
                         + (", ".join(what) if what else "-"))
        return "\n".join(lines)


def sensitivity_of(cjs, factors, varied):
    """cjs / |log2 factor| [settings, ...] for the settings that change one scale (varied >= 0), NaN for the others."""
    out = np.full(cjs.shape, np.nan)
    for d, j in enumerate(varied):
        if j >= 0:
            out[d] = cjs[d] / abs(np.log2(factors[d, j]))
    return out


def flag_of(cjs, sensitivity, floor_of_kind, kind_of_column, base, null, threshold):
    measure = np.where(np.isfinite(sensitivity), sensitivity, cjs)
    with np.errstate(invalid="ignore"):
        out = (measure >= threshold) & (cjs > floor_of_kind[None, :, kind_of_column])
    out[base] = False
    if null is not None:
        out[null] = False
    return out


class Grid(timeline.Timeline):
    """The fitted settings of a grid: `.handle` holds chains_per_setting consecutive chains per setting.  summary, outcomes(k), scenario(k),
    diagnostics are Timeline's, per setting."""

    @property
    def n_settings(self):
        return self.n_dates

    @property
    def chains_per_setting(self):
        return self.chains_per_date

    def compare(self, ev, days=None, base=0, ev_to_win=270):
        """potus_grid_compare: the three distances of every setting to setting `base`, per day of `days` = (begin, end) (0-based; default
        election day alone) and column: a Comparison."""
        days = self._days(days)
        out = self.handle.grid_compare(ev, base, days, ev_to_win)
        c = Comparison(out["distance"], out["n_draws"], self.design, days, base)
        c.timing = self.handle.grid_timing()
        return c

    def log_lik_device(self, integrate=True):
        """log p(y | n, draw) of every poll under every setting's own draws and model, every poll held in-sample: a torch tensor [settings,
        polls, chains per setting, draws] on the handle's GPU (potus_cv_log_lik_device with all-ones masks)."""
        n, Ns, Nn = self.n_settings, int(self.design["data"]["N_state_polls"]), int(self.design["data"]["N_national_polls"])
        ll = self.handle.cv_log_lik_device(np.ones((n, Ns), np.int32), np.ones((n, Nn), np.int32), integrate)
        return ll.reshape(n, Ns + Nn, self.chains_per_setting, -1)

    def loo(self, integrate=True):
        """One Loo per setting, which loo_compare takes: potus_loo_device on the setting's slice of log_lik_device, r_eff computed per poll as for
        a plain handle.  A setting with a failed chain raises."""
        from .loo import loo_of_block, poll_vectors
        ll = self.log_lik_device(integrate)
        status = self.handle.chain_status()[0]
        y, n = poll_vectors(self.design["data"])
        out = []
        for d, lab in enumerate(self.design["labels"]):
            k = self.chains_per_setting
            if status[d * k:(d + 1) * k] != [0] * k:
                raise PotusError(f"setting {d} ({lab}): a chain of its fit failed (chain_status)")
            o = loo_of_block(ll[d].contiguous(), name=lab, y=y, n=n)
            o.integrate = bool(integrate)
            out.append(o)
        return out

    def modes(self, paths_per_setting=1, q0=None, **opts):
        """The posterior mode of every setting in ONE potus_optimize launch on this handle (the chains' state is left alone): Handle.optimize's
        dict with q, lp, grad_norm, return_code, iterations, grad_evals reshaped to [settings, paths, ...].  q0: [settings x paths, D] starts,
        or None for the library's."""
        n, k = self.n_settings, int(paths_per_setting)
        res = self.handle.optimize(q0, n * k, **opts)
        out = {key: res[key].reshape((n, k) + res[key].shape[1:]) for key in ("q", "lp", "grad_norm", "return_code", "iterations", "grad_evals")}
        out["ms"] = self.handle.optimize_timing()
        out["labels"] = list(self.design["labels"])
        return out


def fit(design, variant="full", chains_per_setting=4, **opts):
    """Fit every setting of a grid() design as chains of one launch.  opts: the sampler options of Handle (num_warmup, num_samples, seed, ...)."""
    if design.get("scales") is None:
        raise ValueError("sensitivity.fit: the design has no scales (sensitivity.grid builds one)")
    return timeline.fit(design, variant, chains_per_setting, _cls=Grid, **opts)
