"""alabi_amd.metrics host paths against the reference's recorded outputs (tests/golden/make_golden_metrics.py), and the KDE
bandwidth math against scipy.stats.gaussian_kde.  No GPU needed."""
import os
import re

import numpy as np
import pytest
from scipy import stats
from scipy.stats import multivariate_normal, norm

from alabi_amd import metrics
from alabi_amd.kde import kde_bandwidth, kde_factor, kde_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "reference_metrics_vectors.npz"))

# the analytic densities of the golden mc case (make_golden_metrics.py)
MU_P, COV_P = np.array([0.0, 0.5]), np.array([[1.0, 0.3], [0.3, 0.8]])
MU_Q, COV_Q = np.array([0.4, 0.0]), np.array([[1.5, -0.2], [-0.2, 1.1]])


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))


def test_public_names_match_the_reference():
    assert metrics.__all__ == ["kl_divergence_gaussian", "js_divergence_gaussian", "kl_divergence_integral",
                               "kl_divergence_kde", "compute_kl_single_trial_joblib", "compute_kl_full_parallel"]


def test_gaussian_divergences_match_golden_and_leave_inputs_alone():
    mu1, mu2, cov1, cov2 = G["g_mu1"], G["g_mu2"], G["g_cov1"], G["g_cov2"]
    c1, c2, m1, m2 = cov1.copy(), cov2.copy(), mu1.copy(), mu2.copy()
    assert _rel(metrics.kl_divergence_gaussian(m1, c1, m2, c2), G["g_kl"]) < 1e-12
    assert _rel(metrics.kl_divergence_gaussian(m1, c1, m2, c2, reg=1e-3), G["g_kl_reg"]) < 1e-12
    assert _rel(metrics.js_divergence_gaussian(m1, c1, m2, c2), G["g_js"]) < 1e-12
    for a, b in ((c1, cov1), (c2, cov2), (m1, mu1), (m2, mu2)):
        assert np.array_equal(a, b)


def test_js_counts_the_average_regularisation_twice():
    mu1, mu2, cov1, cov2 = G["g_mu1"], G["g_mu2"], G["g_cov1"], G["g_cov2"]
    mu_a, cov_a = (mu1 + mu2) / 2, (cov1 + cov2) / 2
    once = (metrics.kl_divergence_gaussian(mu1, cov1, mu_a, cov_a) + metrics.kl_divergence_gaussian(mu2, cov2, mu_a, cov_a)) / 2
    js = metrics.js_divergence_gaussian(mu1, cov1, mu2, cov2)
    assert js != once and abs(js - once) < 1e-5


def test_mc_integral_matches_golden():
    np.random.seed(int(G["mc_seed"]))
    out = metrics.kl_divergence_integral(lambda x: multivariate_normal.logpdf(x, MU_P, COV_P),
                                         lambda x: multivariate_normal.logpdf(x, MU_Q, COV_Q),
                                         G["mc_bounds"], method="mc", n_samples=int(G["mc_n"]))
    assert _rel(out, G["mc_out"]) < 1e-12


def test_quad_integral_1d_matches_golden():
    out = metrics.kl_divergence_integral(lambda x: norm.logpdf(x, loc=0, scale=1), lambda x: norm.logpdf(x, loc=1, scale=1.5),
                                         G["quad_bounds"], method="quad")
    assert _rel(out[0], G["quad_out"][0]) < 1e-12


def test_integral_rejects_unknown_method():
    with pytest.raises(ValueError):
        metrics.kl_divergence_integral(np.log, np.log, np.array([[0.0, 1.0]]), method="simpson")


class _Stub:
    """What kde_factor / a callable bandwidth reads from a KDE object."""

    def __init__(self, d, n, weights):
        self.d, self.n = d, n
        self.weights, self.neff = kde_weights(weights, n)

    def scotts_factor(self):
        return np.power(self.neff, -1. / (self.d + 4))


@pytest.mark.parametrize("d", [1, 2, 5, 10])
@pytest.mark.parametrize("bw", [None, "scott", "silverman", 0.37, "callable"])
@pytest.mark.parametrize("weighted", [False, True])
def test_bandwidth_math_equals_scipy(d, bw, weighted):
    rng = np.random.default_rng(d * 7 + weighted)
    n = 300
    X = rng.normal(size=(d, n)) * np.linspace(0.5, 2.0, d)[:, None] + 3.0
    w = rng.uniform(0.1, 1.0, n) if weighted else None
    bw_method = (lambda k: 0.8 * k.scotts_factor()) if bw == "callable" else bw
    ref = stats.gaussian_kde(X, bw_method=bw_method, weights=w)
    s = _Stub(d, n, w)
    factor = kde_factor(bw_method, s)
    cov, cho, log_det = kde_bandwidth(np.cov(X, rowvar=1, bias=False, aweights=s.weights), factor)
    assert np.array_equal(s.weights, ref.weights) and s.neff == ref.neff
    assert factor == ref.factor
    assert np.array_equal(cov, ref.covariance)
    assert np.array_equal(cho, ref.cho_cov)
    assert log_det == ref.log_det


def test_singular_data_raises_value_error_as_scipy():
    rng = np.random.default_rng(0)
    X = np.vstack([rng.normal(size=200), np.zeros(200)])
    with pytest.raises(ValueError):
        stats.gaussian_kde(X)
    with pytest.raises(ValueError):
        kde_bandwidth(np.cov(X, rowvar=1, bias=False), 0.5)


def test_bad_bandwidth_and_weights_raise():
    s = _Stub(2, 10, None)
    with pytest.raises(ValueError):
        kde_factor("wide", s)
    with pytest.raises(ValueError):
        kde_weights(np.ones(9), 10)


def test_kde_entries_in_header_and_binding():
    from alabi_amd import _lib
    text = open(os.path.join(ROOT, "include", "alabi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(alabi_kde_[a-z0-9_]+)\s*\(", text))
    want = {"alabi_kde_create", "alabi_kde_destroy", "alabi_kde_set_data", "alabi_kde_logpdf", "alabi_kde_pdf", "alabi_kde_plan"}
    assert declared == want
    assert want <= set(_lib.SIGNATURES)
