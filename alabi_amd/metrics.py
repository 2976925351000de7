"""Divergences between posteriors: the reference's ``alabi.metrics`` (alabi/metrics.py), with every KDE on the GPU.

* ``kl_divergence_gaussian`` / ``js_divergence_gaussian``: closed forms on the host.  They return the reference's numbers,
  including the regularisation ``js_divergence_gaussian`` ends up adding twice to the averaged covariance (the reference's
  in-place ``+=`` on it), but never modify the caller's arrays.
* ``kl_divergence_integral``: ``quad`` through SciPy; ``mc`` (global ``np.random`` stream) and ``qmc`` (scrambled Sobol) as
  the reference.  The library's own surrogate callables (``SurrogateModel.surrogate_log_likelihood``, the object of
  ``create_cached_surrogate_likelihood``) are evaluated in one batched device prediction; any other callable row by row.
* ``kl_divergence_kde``: the reference's estimator with both densities as ``DeviceKDE`` (csrc/kde.hip).
* ``compute_kl_single_trial_joblib`` / ``compute_kl_full_parallel``: the reference's file layout and statistics; the tasks
  run in this process (``n_jobs`` is accepted) -- the GPU is the parallel axis, and a pool of workers would each open it.
"""
from __future__ import annotations

import os
import pickle

import numpy as np
from scipy import integrate
from scipy.stats import qmc

from .kde import DeviceKDE

__all__ = ["kl_divergence_gaussian",
           "js_divergence_gaussian",
           "kl_divergence_integral",
           "kl_divergence_kde",
           "compute_kl_single_trial_joblib",
           "compute_kl_full_parallel"]


def _regularised(cov, reg):
    cov = np.array(cov, dtype=float)                  # a copy: the caller's array stays as it was
    return cov + reg * np.eye(cov.shape[0])


def _kl_gauss(mu1, cov1r, mu2, cov2r):
    """0.5 (log(det2 / det1) - d + tr(cov2^-1 cov1) + dmu^T cov2^-1 dmu) of already regularised covariances."""
    det1 = np.linalg.det(cov1r)
    det2 = np.linalg.det(cov2r)
    inv_cov2 = np.linalg.inv(cov2r)
    dmu = mu2 - mu1
    return 0.5 * (np.log(det2 / det1) - len(mu1) + np.trace(inv_cov2 @ cov1r) + dmu.T @ inv_cov2 @ dmu)


def kl_divergence_gaussian(mu1, cov1, mu2, cov2, reg=1e-6):
    """D_KL(N(mu1, cov1) || N(mu2, cov2)) with ``reg`` added to both diagonals (alabi/metrics.py:15-45)."""
    mu1, mu2 = np.asarray(mu1), np.asarray(mu2)
    return _kl_gauss(mu1, _regularised(cov1, reg), mu2, _regularised(cov2, reg))


def js_divergence_gaussian(mu1, cov1, mu2, cov2):
    """Jensen-Shannon divergence of two Gaussians through the moment-matched average (alabi/metrics.py:48-65).  As in the
    reference, the second KL term sees the averaged covariance regularised twice (1e-6 I each time)."""
    mu1, mu2 = np.asarray(mu1), np.asarray(mu2)
    cov1, cov2 = np.asarray(cov1), np.asarray(cov2)
    mu_avg = (mu1 + mu2) / 2
    cov_avg = (cov1 + cov2) / 2
    reg = 1e-6
    cov_avg_r = _regularised(cov_avg, reg)
    kl1 = _kl_gauss(mu1, _regularised(cov1, reg), mu_avg, cov_avg_r)
    kl2 = _kl_gauss(mu2, _regularised(cov2, reg), mu_avg, _regularised(cov_avg_r, reg))
    return (kl1 + kl2) / 2


def _is_surrogate(fn):
    """The library's own surrogate log-likelihoods, which take a whole (n, d) batch in one device prediction."""
    from .core import CachedSurrogateLikelihood, SurrogateModel
    if isinstance(fn, CachedSurrogateLikelihood):
        return True
    return getattr(fn, "__func__", None) is SurrogateModel.surrogate_log_likelihood and \
        isinstance(getattr(fn, "__self__", None), SurrogateModel)


def kl_divergence_integral(log_p, log_q, bounds, method='qmc', n_samples=int(2**14), epsilon=1e-12, n_jobs=1):
    """KL(P||Q) = int p log(p / q) dx by 'quad' (SciPy quad / nquad), 'mc' (uniform draws from the global np.random stream)
    or 'qmc' (scrambled Sobol) (alabi/metrics.py:68-207).  Returns (estimate, error).  ``n_jobs`` is accepted and unused, as in
    the reference."""
    bounds = np.asarray(bounds)

    def integrand(x):
        if np.isscalar(x):
            x = np.array([x])
        p_val = np.maximum(np.exp(log_p(x)), epsilon)
        q_val = np.maximum(np.exp(log_q(x)), epsilon)
        return p_val * np.log(p_val / q_val)

    if method == 'quad' and bounds.ndim == 1:
        return integrate.quad(integrand, bounds[0], bounds[1])
    if method == 'quad' and bounds.ndim == 2:
        return integrate.nquad(lambda *args: integrand(np.array(args)), bounds)
    if method not in ('mc', 'qmc'):
        raise ValueError("Invalid method. Choose 'quad', 'mc', or 'qmc'")
    if bounds.ndim == 1:
        bounds = bounds.reshape(1, -1)
    ndim = bounds.shape[0]
    if method == 'mc':
        samples = np.random.uniform(low=bounds[:, 0], high=bounds[:, 1], size=(n_samples, ndim))
    else:
        unit = qmc.Sobol(d=ndim, scramble=True).random(n_samples)
        samples = qmc.scale(unit, bounds[:, 0], bounds[:, 1])
    volume = np.prod(bounds[:, 1] - bounds[:, 0])

    def batch_log(fn):
        return np.asarray(fn(samples), dtype=np.float64).reshape(-1) if _is_surrogate(fn) else None

    lp, lq = batch_log(log_p), batch_log(log_q)
    if lp is None and lq is None:
        vals = np.array([integrand(sample) for sample in samples])
    else:
        # at least one side in one batched prediction; the other (if a plain callable) row by row, as the reference calls it
        if lp is None:
            lp = np.array([np.asarray(log_p(s)).reshape(-1)[0] for s in samples], dtype=np.float64)
        if lq is None:
            lq = np.array([np.asarray(log_q(s)).reshape(-1)[0] for s in samples], dtype=np.float64)
        p_val = np.maximum(np.exp(lp), epsilon)
        q_val = np.maximum(np.exp(lq), epsilon)
        vals = p_val * np.log(p_val / q_val)
    vals = np.asarray(vals, dtype=np.float64)
    vals[vals > 1e10] = np.nan
    vals[vals < 0] = np.nan
    return volume * np.nanmean(vals), volume * np.nanstd(vals) / np.sqrt(n_samples)


def kl_divergence_kde(samples_p, samples_q, bandwidth=None, epsilon=1e-12, n_eval=1000):
    """KDE estimate of D_KL(P||Q) from samples (alabi/metrics.py:210-336), both KDEs as DeviceKDE.  Reference semantics:
    Scott's factor whether or not ``bandwidth`` is given; ``n_eval`` evaluation points uniform on the combined min/max box from
    the global np.random stream; densities clamped at ``epsilon``; log-ratios weighted by the normalised pdf_p; abs() of the
    sum; NaN when no ratio is finite."""
    samples_p = np.asarray(samples_p)
    samples_q = np.asarray(samples_q)
    if samples_p.ndim == 1:
        samples_p = samples_p.reshape(-1, 1)
    if samples_q.ndim == 1:
        samples_q = samples_q.reshape(-1, 1)
    if samples_p.shape[1] != samples_q.shape[1]:
        raise ValueError("Samples must have same dimensionality")
    kde_p = DeviceKDE(samples_p.T, bw_method="scott")
    kde_q = DeviceKDE(samples_q.T, bw_method="scott")
    all_samples = np.vstack([samples_p, samples_q])
    lo, hi = np.min(all_samples, axis=0), np.max(all_samples, axis=0)
    eval_points = np.random.uniform(lo, hi, size=(n_eval, samples_p.shape[1])).T
    pdf_p = np.maximum(kde_p.pdf(eval_points), epsilon)
    pdf_q = np.maximum(kde_q.pdf(eval_points), epsilon)
    log_ratio = np.log(pdf_p / pdf_q)
    valid = np.isfinite(log_ratio)
    if np.sum(valid) == 0:
        return np.nan
    weights = pdf_p[valid] / np.sum(pdf_p[valid])
    return np.abs(np.sum(weights * log_ratio[valid]))


def load_pickle(savedir, fname="surrogate_model.pkl"):
    """The pickled SurrogateModel in ``savedir`` (alabi/cache_utils.py:18-24)."""
    with open(os.path.join(savedir, fname), "rb") as f:
        return pickle.load(f)


def load_model_cache(savedir):
    """The model cache of ``savedir`` (alabi/cache_utils.py:27-66, without MPI: one process reads it)."""
    return load_pickle(savedir)


def compute_kl_single_trial_joblib(trial, ii, base_dir, example, kernel):
    """KL between the surrogate posterior of one trial at iteration ``ii`` and the true posterior (alabi/metrics.py:339-362).
    Missing sample files are produced by run_dynesty from the cached models, as in the reference."""
    root = f"{base_dir}/{example}/{kernel}"
    file_p = f"{root}/{trial}/dynesty_samples_final_surrogate_iter_{ii}.npz"
    file_q = f"{root}/dynesty_samples_final_true.npz"
    if not os.path.exists(file_p):
        sm = load_model_cache(f"{root}/{trial}/")
        print(f"Loaded model from cache for trial {trial}, iteration {ii}")
        sm.run_dynesty(like_fn=sm.surrogate_log_likelihood)
    if not os.path.exists(file_q):
        sm = load_model_cache(f"{root}/")
        print(f"Loaded true model from cache for trial {trial}, iteration {ii}")
        sm.run_dynesty(like_fn=sm.lnlike_fn)
    try:
        samples_p = np.load(file_p)["samples"]
        samples_q = np.load(file_q)["samples"]
        return kl_divergence_kde(samples_p, samples_q)
    except Exception as e:  # noqa: BLE001  (the reference reports and returns NaN)
        print(f"Error processing trial {trial}, iteration {ii}: {e}")
        return np.nan


def compute_kl_full_parallel(base_dir, example, kernel, trials=np.arange(0, 30), iterations=np.arange(10, 250, 10), n_jobs=16):
    """KL statistics per iteration over trials (alabi/metrics.py:365-402): rows [mean, std, 25th percentile, median, 75th
    percentile] of the finite KLs, one per entry of ``iterations``.  The tasks run in this process, in the reference's order."""
    tasks = [(trial, ii) for trial in trials for ii in iterations]
    print(f"Processing {len(tasks)} tasks for {base_dir}/{example}/{kernel}")
    results = [compute_kl_single_trial_joblib(trial, ii, base_dir, example, kernel) for trial, ii in tasks]
    by_iter = {}
    for (trial, ii), kl in zip(tasks, results):
        by_iter.setdefault(ii, []).append(kl)
    rows = []
    for ii in iterations:
        valid = [kl for kl in by_iter[ii] if not np.isnan(kl)]
        if valid:
            rows.append(np.array([np.mean(valid), np.std(valid), np.percentile(valid, 25), np.median(valid),
                                  np.percentile(valid, 75)]))
        else:
            rows.append([np.nan, np.nan, np.nan, np.nan, np.nan])
    return np.array(rows)
