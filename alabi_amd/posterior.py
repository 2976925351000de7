"""Which part of the log-posterior the device kernels evaluate themselves and which part is a host call.

``SurrogateModel.run_emcee`` and ``run_dynesty`` each ask once (``plan_ensemble`` / ``plan_nested``) and hand the fields of the
``PosteriorPlan`` they get to ``EnsembleSampler`` / ``GPUWalkBackend``.  Host only: no GPU, no shared library.  The kernels fold
  * a theta scaler that is an affine map per dimension (``_affine_map``): the walkers move in scaled theta;
  * a y scaler whose inverse is affine with a positive slope, or ``nlog_scaler`` / ``log_scaler`` (``_y_unscale_kind``);
  * the box prior; for the ensemble sampler ``lnprior_normal`` on top of it; for nested sampling the uniform prior transform and
    ``prior_transform_normal`` (the inverse normal CDF on the coordinates with a Gaussian prior; no Jacobian term: in nested
    sampling the prior enters through the transform alone, so it folds behind the nlog / log y maps too).
Everything else is a host callable on a batch of points in the sampler's coordinates ([n,d] -> [n])."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import numpy as np

from . import utility as ut


@dataclass
class PosteriorPlan:
    box: np.ndarray                # [d,2] the sampler's box: the prior box in scaled theta (nested, host likelihood: the cube)
    to_theta: Callable             # sampler coordinates [n,d] -> theta [n,d]
    theta_box: np.ndarray = None   # the prior box in theta, where the prior is a box
    t_mult: np.ndarray = None      # ensemble: sampler coordinates = t_mult * theta + t_add per dimension (the theta scaler;
    t_add: np.ndarray = None       # the identity with a host likelihood)
    logp_affine: tuple = (1.0, 0.0)    # (scale, shift) applied to the GP mean on the device
    logp_map: str = None           # "nlog" or "log": the non-affine y un-scaling applied after logp_affine
    normal_prior: tuple = None     # (mean[d], std[d]) in scaled theta, NaN = no normal on that coordinate (nested: std is signed,
                                   # negative under a decreasing theta scaler)
    host_prior: Callable = None    # sampler coordinates [n,d] -> [n]
    host_like: Callable = None     # sampler coordinates [n,d] -> [n]

    @property
    def fused(self):
        """No host callable: the whole log-probability is evaluated inside the kernels."""
        return self.host_prior is None and self.host_like is None


def _affine_map(fn, box):
    """(mult, add) with fn(x) == mult * x + add per column on `box` ([d, 2] lower / upper), or None if fn is not an
    increasing-or-decreasing affine map per dimension there (checked at three interior points)."""
    try:
        box = np.asarray(box, dtype=np.float64).reshape(-1, 2)
        lo, hi = box[:, 0], box[:, 1]
        f_lo = np.asarray(fn(lo.reshape(1, -1)), dtype=np.float64).reshape(-1)
        f_hi = np.asarray(fn(hi.reshape(1, -1)), dtype=np.float64).reshape(-1)
        if f_lo.shape != lo.shape or np.any(hi == lo):
            return None
        mult = (f_hi - f_lo) / (hi - lo)
        add = f_lo - mult * lo
        if not (np.all(np.isfinite(mult)) and np.all(np.isfinite(add)) and np.all(mult != 0)):
            return None
        for frac in (0.25, 0.5, 0.8):
            x = lo + frac * (hi - lo)
            fx = np.asarray(fn(x.reshape(1, -1)), dtype=np.float64).reshape(-1)
            if not np.allclose(fx, mult * x + add, rtol=1e-11, atol=1e-11 * (np.abs(f_hi) + np.abs(f_lo) + 1e-300)):
                return None
        return mult, add
    except Exception:  # noqa: BLE001
        return None


def _y_unscale_kind(y_scaler, _y):
    """How y_scaler.inverse_transform acts on a GP mean over the scaled training values `_y`: ("affine", slope, offset),
    ("nlog",) / ("log",) for the two non-affine scalers the reference ships (alabi/utility.py:62-71), or None (anything else)."""
    y_lo, y_hi = float(np.min(_y)), float(np.max(_y))
    aff = _affine_map(y_scaler.inverse_transform, np.array([[y_lo - 1.0, y_hi + 1.0]]))
    if aff is not None and aff[0][0] > 0:
        return ("affine", float(aff[0][0]), float(aff[1][0]))
    try:
        probe = np.linspace(y_lo - 0.5, y_hi + 0.5, 7).reshape(-1, 1)
        got = np.asarray(y_scaler.inverse_transform(probe), dtype=np.float64).reshape(-1)
        p10 = 10.0 ** probe.reshape(-1)
        if np.allclose(got, -p10, rtol=1e-12, atol=0.0):
            return ("nlog",)
        if np.allclose(got, p10, rtol=1e-12, atol=0.0):
            return ("log",)
    except Exception:  # noqa: BLE001
        pass
    return None


def _fold_scalers(theta_scaler, y_scaler, _y, bounds):
    """((t_mult, t_add), logp_affine, logp_map) when the kernels can fold both scalers (a model without a theta scaler moves in
    theta itself), else None."""
    ndim = len(bounds)
    t_aff = (np.ones(ndim), np.zeros(ndim)) if theta_scaler is None else _affine_map(theta_scaler.transform, bounds)
    y_kind = _y_unscale_kind(y_scaler, _y)
    if t_aff is None or y_kind is None:
        return None
    if y_kind[0] == "affine":
        return t_aff, (y_kind[1], y_kind[2]), None
    return t_aff, (1.0, 0.0), y_kind[0]


def _shipped_prior(prior_fn):
    """(bounds, data) of ``partial(lnprior_uniform, bounds=...)`` (data None) or ``partial(lnprior_normal, bounds=..., data=...)``,
    arguments by keyword or by position; None for any other callable."""
    f = getattr(prior_fn, "func", None)
    kwp = dict(getattr(prior_fn, "keywords", None) or {})
    argp = tuple(getattr(prior_fn, "args", ()) or ())
    name = getattr(f, "__name__", "")
    if name == "lnprior_uniform" and f is ut.lnprior_uniform and ("bounds" in kwp or len(argp) >= 1):
        return kwp.get("bounds", argp[0] if argp else None), None
    if name == "lnprior_normal" and f is ut.lnprior_normal and (("bounds" in kwp and "data" in kwp) or len(argp) >= 2):
        return kwp.get("bounds", argp[0] if argp else None), kwp.get("data", argp[1] if len(argp) > 1 else None)
    return None


def _uniform_prior_box(prior_transform, ndim):
    """The box [ndim, 2] of ``partial(ut.prior_transform_uniform, bounds=B)`` (the tutorials' prior transform, which the
    fused nested-sampling path samples directly), else None (any other callable runs on the host)."""
    f = getattr(prior_transform, "func", None)
    kwp = dict(getattr(prior_transform, "keywords", None) or {})
    if f is ut.prior_transform_uniform and "bounds" in kwp and not getattr(prior_transform, "args", ()):
        return np.asarray(kwp["bounds"], dtype=np.float64).reshape(ndim, 2)
    return None


def _normal_prior_transform(prior_transform, ndim):
    """(box [ndim, 2], mean [ndim], std [ndim]) of ``partial(ut.prior_transform_normal, bounds=B, data=D)`` (keywords only, the
    rule of ``_uniform_prior_box``), NaN mean / std on the coordinates whose data is ``(None, None)``; None for any other callable.
    A normal coordinate with std <= 0 or a non-finite mean or std raises ValueError."""
    f = getattr(prior_transform, "func", None)
    kwp = dict(getattr(prior_transform, "keywords", None) or {})
    if f is not ut.prior_transform_normal or set(kwp) != {"bounds", "data"} or getattr(prior_transform, "args", ()):
        return None
    box, data = np.asarray(kwp["bounds"], dtype=np.float64).reshape(ndim, 2), kwp["data"]
    if len(data) != ndim:
        raise ValueError(f"prior_transform_normal: data length ({len(data)}) must match the {ndim} dimensions")
    mean = np.array([np.nan if dd[0] is None else float(dd[0]) for dd in data])
    std = np.array([np.nan if dd[0] is None else float(dd[1]) for dd in data])
    on = np.array([dd[0] is not None for dd in data])
    if np.any(on & ~(np.isfinite(mean) & np.isfinite(std) & (std > 0))):
        raise ValueError("prior_transform_normal: every (mean, std) must be finite with std > 0")
    return box, mean, std


def host_rows(fn, row_shape, to_theta=None):
    """[n,d] -> [n] with one call of ``fn`` per point.  ``row_shape`` is the argument shape the sampler promises: (1, -1) for the
    ensemble sampler, what lnprob hands to like_fn / prior_fn (core.py:2097-2098); (-1,) for nested sampling, as dynesty calls."""
    def call(q):
        th = q if to_theta is None else to_theta(q)
        return np.array([float(np.asarray(fn(row.reshape(row_shape))).reshape(-1)[0]) for row in th], dtype=np.float64)
    return call


def host_likelihood(fn, surrogate, row_shape, to_theta=None):
    """The surrogate (``fn == surrogate``) takes the whole batch in one GPU predict; every other callable is called row by row."""
    if fn == surrogate:
        return lambda q: np.asarray(fn(q if to_theta is None else to_theta(q)), dtype=np.float64).reshape(-1)
    return host_rows(fn, row_shape, to_theta)


def plan_ensemble(like_host, surrogate, prior_fn, bounds, theta_scaler, y_scaler, _y):
    """The ensemble sampler's plan.  ``like_host``: the likelihood if it is a host callable on theta, None for the surrogate;
    ``surrogate``: the model's ``surrogate_log_likelihood``, which becomes the host likelihood when a scaler cannot be folded;
    ``prior_fn``: None (the box ``bounds``) or any callable.  With a host likelihood the walkers move in theta itself."""
    ndim = len(bounds)
    shipped = _shipped_prior(prior_fn)
    prior_bounds, prior_data = shipped or (None, None)
    prior_host = None if shipped else prior_fn
    folded = _fold_scalers(theta_scaler, y_scaler, _y, bounds) if like_host is None else None
    if like_host is None and folded is None:
        like_host = surrogate                      # exotic scalers: surrogate_log_likelihood (batched GPU predict) on the host side
    (t_mult, t_add), logp_affine, logp_map = folded or ((np.ones(ndim), np.zeros(ndim)), (1.0, 0.0), None)
    theta_box = bounds if prior_bounds is None else np.asarray(prior_bounds, dtype=np.float64).reshape(ndim, 2)
    normal_prior = None
    if prior_data is not None:
        pm = np.array([np.nan if dd[0] is None else float(dd[0]) for dd in prior_data])
        ps = np.array([np.nan if dd[0] is None else float(dd[1]) for dd in prior_data])
        # N(m, s) on theta_k is N(mult m + add, |mult| s) on the scaled coordinate; the density stays the theta-space one,
        # so log|mult| per normal coordinate goes back into the log-probability through the constant shift
        normal_prior = (pm * t_mult + t_add, ps * np.abs(t_mult))
        if logp_map is None:
            logp_affine = (logp_affine[0], logp_affine[1] + float(np.sum(np.log(np.abs(t_mult[np.isfinite(pm)])))))
        elif np.any(t_mult[np.isfinite(pm)] != 1.0):
            prior_host, normal_prior = prior_fn, None            # cannot fold the Jacobian behind a non-affine map: host prior
        if like_host is not None:
            prior_host, normal_prior = prior_fn, None            # the fused normal prior lives in the device likelihood path
    to_theta = lambda c: (np.asarray(c) - t_add) / t_mult  # noqa: E731
    return PosteriorPlan(
        box=np.sort(theta_box * t_mult[:, None] + t_add[:, None], axis=1), to_theta=to_theta, theta_box=theta_box, t_mult=t_mult,
        t_add=t_add, logp_affine=logp_affine, logp_map=logp_map, normal_prior=normal_prior,
        host_prior=None if prior_host is None else host_rows(prior_host, (1, -1), to_theta),
        host_like=None if like_host is None else host_likelihood(like_host, surrogate, (1, -1), to_theta))


def plan_nested(like_fn, surrogate, prior_transform, bounds, theta_scaler, y_scaler, _y):
    """Nested sampling's plan: the sampler moves in the unit cube.  Fused when ``like_fn`` is the surrogate, ``prior_transform`` is
    the uniform one over a box or ``partial(ut.prior_transform_normal, bounds=..., data=...)`` and both scalers fold: ``box`` is
    then the box in scaled theta, lower / upper as the cube maps to them, and ``normal_prior`` (mean, std) in scaled theta for the
    coordinates with a Gaussian prior (std negative under a decreasing theta scaler; None when there is none).  Otherwise the
    host evaluates ``like_fn(prior_transform(u))`` and ``box`` is the cube; ``prior_transform_normal`` then takes a whole batch in
    one call, any other callable is called row by row."""
    ndim = len(bounds)
    theta_box, normal = _uniform_prior_box(prior_transform, ndim), None
    batched = False
    if theta_box is None:
        normal = _normal_prior_transform(prior_transform, ndim)
        if normal is not None:
            theta_box, batched = normal[0], True
            if not np.any(np.isfinite(normal[1])):
                normal = None                                                    # all (None, None): the uniform transform
    folded = _fold_scalers(theta_scaler, y_scaler, _y, bounds) if (like_fn == surrogate and theta_box is not None) else None
    if folded is not None:
        (t_mult, t_add), logp_affine, logp_map = folded
        lo_t, hi_t = theta_box[:, 0], theta_box[:, 1]
        plan = PosteriorPlan(box=np.stack([lo_t * t_mult + t_add, hi_t * t_mult + t_add], axis=1), theta_box=theta_box,
                             to_theta=lambda u: lo_t + u * (hi_t - lo_t),        # prior_transform_uniform
                             logp_affine=logp_affine, logp_map=logp_map)
        if normal is not None:
            plan.normal_prior = (t_mult * normal[1] + t_add, t_mult * normal[2])
            plan.to_theta = lambda u: np.asarray(prior_transform(np.atleast_2d(u)), dtype=np.float64)
        return plan

    def to_theta(u):
        if batched:                                              # prior_transform_normal: [n, d] in one call
            return np.asarray(prior_transform(np.atleast_2d(u)), dtype=np.float64)
        return np.array([np.asarray(prior_transform(row), dtype=np.float64).reshape(-1) for row in np.atleast_2d(u)])
    return PosteriorPlan(box=np.tile([0.0, 1.0], (ndim, 1)), to_theta=to_theta,
                         host_like=host_likelihood(like_fn, surrogate, (-1,), to_theta))


def run_until_min_ess(run, min_ess, note=None):
    """Call ``run(k)`` for k = 1, 2, ... (it performs run number k and returns that run's samples [n,d]) until ``min_ess`` samples
    exist, at most 10 runs, and return the samples of all runs.  With ``note`` (total so far -> text) and ``min_ess`` > 0 every run
    is reported on a line that ends with it."""
    chains, accumulated = [], 0
    for k in range(1, 11):
        chains.append(run(k))
        accumulated += chains[-1].shape[0]
        if note is not None and min_ess > 0:
            print(f"Run {k} complete: {chains[-1].shape[0]} samples{note(accumulated)}")
        if accumulated >= min_ess:
            break
    else:
        print(f"WARNING: Reached maximum of 10 runs, stopping with {accumulated} samples")
    return np.vstack(chains) if len(chains) > 1 else chains[0]
