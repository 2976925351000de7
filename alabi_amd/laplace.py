"""The Laplace approximation at a maximum of the log-posterior: covariance and evidence estimate from the Hessian there.  Pure
NumPy, no GPU: the Hessian comes from ``EnsembleSampler.log_prob_hessian`` (closed form, on the device) at the point
``EnsembleSampler.maximize`` found; ``SurrogateModel.laplace_approximation`` puts the three together.

With H the Hessian of the log-posterior at its interior maximum x* and lp = log-posterior(x*):

    covariance        (-H)^-1
    log evidence      lp + (d / 2) ln 2 pi - (1 / 2) ln det(-H) - sum_k ln width_k

The last sum runs over the coordinates WITHOUT a normal prior: the library's uniform prior (``lnprior_uniform``) is 0 inside the
box, not -ln width, while ``run_dynesty``'s prior transform is normalised; with the subtraction the number is comparable to
``run_dynesty``'s log Z.  A normal prior's log-density is normalised already.

Coordinates.  The sampler moves in c = T theta + t with T = diag(t_mult) (the theta scaler folded into the kernels), so a Hessian
taken there is with respect to c:  H_theta = T H_c T,  cov_theta = T^-1 cov_c T^-1, and back.  The evidence does not depend on the
frame as long as lp is the density in theta (which the plan's constant shift makes it) and the widths are theta's.
"""
from __future__ import annotations

import numpy as np

__all__ = ["laplace_covariance", "laplace_log_evidence", "hessian_to_theta", "hessian_to_scaled", "covariance_to_theta",
           "covariance_to_scaled"]

LOG_2PI = 1.8378770664093453


def _neg_cholesky(H):
    """Lower Cholesky factor of -H (symmetrised), or None where -H is not positive definite or not finite."""
    H = np.asarray(H, dtype=np.float64)
    if H.ndim != 2 or H.shape[0] != H.shape[1] or not np.all(np.isfinite(H)):
        return None
    try:
        return np.linalg.cholesky(-0.5 * (H + H.T))
    except np.linalg.LinAlgError:
        return None


def laplace_covariance(H):
    """(-H)^-1 through the Cholesky factor of -H; None if -H is not positive definite."""
    L = _neg_cholesky(H)
    if L is None:
        return None
    Li = np.linalg.solve(L, np.eye(L.shape[0]))
    return Li.T @ Li


def laplace_log_evidence(lp_max, H, widths_of_uniform_coords=()):
    """lp + (d / 2) ln 2 pi - (1 / 2) ln det(-H) - sum ln width; None if -H is not positive definite.
    ``widths_of_uniform_coords``: the box widths, in theta, of the coordinates that carry the (unnormalised) uniform prior."""
    L = _neg_cholesky(H)
    if L is None:
        return None
    w = np.asarray(widths_of_uniform_coords, dtype=np.float64).reshape(-1)
    d = L.shape[0]
    return float(lp_max) + 0.5 * d * LOG_2PI - float(np.sum(np.log(np.diag(L)))) - float(np.sum(np.log(w)))


def _t(t_mult, d):
    t = np.asarray(t_mult, dtype=np.float64).reshape(-1)
    if t.shape != (d,) or np.any(t == 0.0) or not np.all(np.isfinite(t)):
        raise ValueError("t_mult must hold one finite non-zero factor per dimension")
    return t


def hessian_to_theta(H_scaled, t_mult):
    """H_theta = T H_c T for c = T theta + t."""
    H = np.asarray(H_scaled, dtype=np.float64)
    t = _t(t_mult, H.shape[0])
    return t[:, None] * H * t[None, :]


def hessian_to_scaled(H_theta, t_mult):
    """H_c = T^-1 H_theta T^-1."""
    H = np.asarray(H_theta, dtype=np.float64)
    t = _t(t_mult, H.shape[0])
    return H / t[:, None] / t[None, :]


def covariance_to_theta(cov_scaled, t_mult):
    """cov_theta = T^-1 cov_c T^-1."""
    return hessian_to_scaled(cov_scaled, t_mult)


def covariance_to_scaled(cov_theta, t_mult):
    """cov_c = T cov_theta T: the form ``GaussianMove`` / ``HMCMove`` take under ``run_emcee``."""
    return hessian_to_theta(cov_theta, t_mult)
