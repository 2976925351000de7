#!/usr/bin/env python3
"""Generate tests/golden/reference_metrics_vectors.npz by EXECUTING the reference's alabi/metrics.py.

Run in the build container only (the reference tree does not exist on the GPU box):

    python tests/golden/make_golden_metrics.py

metrics.py is loaded by file path as a module of a placeholder package whose ``cache_utils`` is inert (its
``load_model_cache`` is only reached when a sample file is missing, which never happens here).  Nothing from the reference
is copied: this script stores INPUTS, seeds and the OUTPUTS the reference functions returned.

Vectors written (float64 unless noted):
  g_*     : kl_divergence_gaussian (default reg and reg=1e-3) and js_divergence_gaussian on 3-D Gaussians
  mc_*    : kl_divergence_integral(method="mc") of two 2-D Gaussians (analytic log-densities below), np.random.seed(mc_seed)
  quad_*  : kl_divergence_integral(method="quad") of two 1-D normals
  kde_*   : kl_divergence_kde on fixed sample sets after np.random.seed(kde_seed): 2-D defaults, and 3-D with
            bandwidth=0.3, n_eval=500
  full_*  : compute_kl_full_parallel(n_jobs=1) over a tree of fixed sample files after np.random.seed(full_seed)
"""
import importlib.util
import os
import sys
import tempfile
import types
import warnings

import numpy as np
from scipy.stats import multivariate_normal, norm

REF = "/root/reference/alabi"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_metrics_vectors.npz")

# the two analytic densities of the mc case (tests/test_metrics_host.py defines the same)
MC_MU_P, MC_COV_P = np.array([0.0, 0.5]), np.array([[1.0, 0.3], [0.3, 0.8]])
MC_MU_Q, MC_COV_Q = np.array([0.4, 0.0]), np.array([[1.5, -0.2], [-0.2, 1.1]])


def mc_log_p(x):
    return multivariate_normal.logpdf(x, MC_MU_P, MC_COV_P)


def mc_log_q(x):
    return multivariate_normal.logpdf(x, MC_MU_Q, MC_COV_Q)


def quad_log_p(x):
    return norm.logpdf(x, loc=0, scale=1)


def quad_log_q(x):
    return norm.logpdf(x, loc=1, scale=1.5)


def _load_metrics():
    pkg = types.ModuleType("alabi_ref")
    pkg.__path__ = []
    cu = types.ModuleType("alabi_ref.cache_utils")

    def load_model_cache(savedir):
        raise RuntimeError("placeholder cache_utils: no model cache in golden generation")

    cu.load_model_cache = load_model_cache
    sys.modules["alabi_ref"] = pkg
    sys.modules["alabi_ref.cache_utils"] = cu
    spec = importlib.util.spec_from_file_location("alabi_ref.metrics", f"{REF}/metrics.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules["alabi_ref.metrics"] = mod
    spec.loader.exec_module(mod)
    return mod


def write_tree(root, out):
    """The sample files compute_kl_full_parallel reads: <root>/ex/k/<trial>/..._iter_<ii>.npz and <root>/ex/k/..._true.npz."""
    for key, val in out.items():
        if key.startswith("full_p_"):
            _, _, trial, ii = key.split("_")
            d = os.path.join(root, "ex", "k", trial)
            os.makedirs(d, exist_ok=True)
            np.savez(os.path.join(d, f"dynesty_samples_final_surrogate_iter_{ii}.npz"), samples=val)
    np.savez(os.path.join(root, "ex", "k", "dynesty_samples_final_true.npz"), samples=out["full_q"])


def main():
    warnings.filterwarnings("ignore")
    met = _load_metrics()
    rng = np.random.RandomState(20261016)
    out = {}

    # ---------------- Gaussian closed forms
    d = 3
    A, B = rng.randn(d, d), rng.randn(d, d)
    mu1, mu2 = rng.randn(d), rng.randn(d)
    cov1, cov2 = A @ A.T + 0.5 * np.eye(d), B @ B.T + 0.5 * np.eye(d)
    out.update(g_mu1=mu1, g_mu2=mu2, g_cov1=cov1, g_cov2=cov2)
    out["g_kl"] = met.kl_divergence_gaussian(mu1, cov1.copy(), mu2, cov2.copy())
    out["g_kl_reg"] = met.kl_divergence_gaussian(mu1, cov1.copy(), mu2, cov2.copy(), reg=1e-3)
    out["g_js"] = met.js_divergence_gaussian(mu1, cov1.copy(), mu2, cov2.copy())

    # ---------------- integrals
    out["mc_seed"] = np.int64(12345)
    out["mc_n"] = np.int64(2048)
    out["mc_bounds"] = np.array([[-4.0, 4.0], [-3.0, 5.0]])
    np.random.seed(int(out["mc_seed"]))
    out["mc_out"] = np.array(met.kl_divergence_integral(mc_log_p, mc_log_q, out["mc_bounds"], method="mc",
                                                        n_samples=int(out["mc_n"])))
    out["quad_bounds"] = np.array([-5.0, 5.0])
    out["quad_out"] = np.array(met.kl_divergence_integral(quad_log_p, quad_log_q, out["quad_bounds"], method="quad"))

    # ---------------- KDE estimator
    out["kde_p2"] = rng.multivariate_normal([0.0, 0.0], [[1.0, 0.5], [0.5, 1.0]], 1500)
    out["kde_q2"] = rng.multivariate_normal([0.7, -0.2], [[1.5, 0.0], [0.0, 0.8]], 1200)
    out["kde_p3"] = rng.randn(900, 3)
    out["kde_q3"] = 1.3 * rng.randn(700, 3) + 0.2
    out["kde_seed"] = np.int64(7)
    np.random.seed(7)
    out["kde_kl2"] = met.kl_divergence_kde(out["kde_p2"], out["kde_q2"])
    np.random.seed(8)
    out["kde_kl3"] = met.kl_divergence_kde(out["kde_p3"], out["kde_q3"], bandwidth=0.3, n_eval=500)

    # ---------------- compute_kl_full_parallel over a tree of sample files (in-process: n_jobs=1)
    trials, iters = np.array([0, 1, 2]), np.array([10, 20])
    out["full_trials"], out["full_iters"] = trials, iters
    out["full_q"] = rng.randn(400, 2)
    for t in trials:
        for ii in iters:
            out[f"full_p_{t}_{ii}"] = rng.randn(300, 2) * (1.0 + 2.0 / ii) + 0.5 / ii + 0.1 * t
    out["full_seed"] = np.int64(99)
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, out)
        np.random.seed(99)
        out["full_out"] = met.compute_kl_full_parallel(root, "ex", "k", trials=trials, iterations=iters, n_jobs=1)

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", {k: out[k] for k in ("g_kl", "g_js", "mc_out", "quad_out", "kde_kl2",
                                                                          "kde_kl3")})


if __name__ == "__main__":
    main()
