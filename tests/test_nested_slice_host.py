"""Host side of the random-direction slice move (sample="rslice") of alabi_amd/nested.py, with the NumPy model of the move in
tests/rslice_numpy.py as the backend: the evidence of the 3-D correlated Gaussian of test_nested_host.py, the evidence of a
24-D Gaussian (where the 25-step random walk is off by 4-7 logzerr), the slice scale rule, and what run_dynesty still refuses."""
import inspect
import math

import numpy as np
import pytest

from alabi_amd import nested as ns
from rslice_numpy import SliceCubeBackend, separable_gaussian


def _problem3(seed):
    A = np.array([[1.0, 0.6, 0.2], [0.6, 1.5, -0.4], [0.2, -0.4, 0.8]])
    mu = np.array([0.3, -0.5, 0.1])
    lo, hi = np.full(3, -6.0), np.full(3, 6.0)
    prec = np.linalg.inv(A)
    norm = -0.5 * (3 * math.log(2 * math.pi) + np.linalg.slogdet(A)[1])

    def logl_theta(theta):
        r = theta - mu
        return norm - 0.5 * np.einsum("ni,ij,nj->n", r, prec, r)
    return SliceCubeBackend(logl_theta, lo, hi, seed), mu, A, lo, hi


@pytest.mark.parametrize("dynamic", [False, True])
def test_rslice_evidence_of_correlated_gaussian_in_a_box(dynamic):
    """The assertions of test_nested_host.py::test_evidence_of_correlated_gaussian_in_a_box, with the slice move."""
    be, mu, A, lo, hi = _problem3(12)
    s = ns.NestedSampler(be, 300, dynamic=dynamic, seed=13, sample="rslice")
    assert s.slices == ns.default_slices(3) == ns.SLICES_MULT * 6
    r = s.run_nested(dlogz=0.1, n_effective=3000, maxbatch=3) if dynamic else s.run_nested(dlogz=0.1)
    logz_true = -np.sum(np.log(hi - lo))
    assert abs(r.logz[-1] - logz_true) < 3 * r.logzerr[-1], (r.logz[-1], logz_true, r.logzerr[-1])
    eq = r.samples_equal(np.random.default_rng(0))
    assert np.allclose(eq.mean(0), mu, atol=0.25)
    assert np.allclose(np.cov(eq.T), A, atol=0.35)
    assert r.status in (("converged",) if not dynamic else ("n_effective", "maxbatch"))
    assert r.eff > 0 and r.ncall >= r.niter
    assert r.n_stuck == 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rslice_evidence_in_24_dimensions(seed):
    """Separable Gaussian, sigma_k = exp(U(-1,1)), box +-10 sigma, d = 24, nlive = 200, the default number of slices: log Z
    within 3 logzerr of -sum log(hi - lo) and no capped walk.  (The random walk returns log Z high by 1.4-2.2 here.)"""
    logl, lo, hi, truth = separable_gaussian(24)
    be = SliceCubeBackend(logl, lo, hi, seed=1000 + seed)
    s = ns.NestedSampler(be, 200, sample="rslice", seed=seed)
    assert s.slices == ns.SLICES_MULT * 27
    r = s.run_nested(dlogz=0.1)
    print(seed, r.logz[-1] - truth, r.logzerr[-1], r.ncall / r.niter, s.scale)
    assert r.status == "converged"
    assert abs(r.logz[-1] - truth) <= 3 * r.logzerr[-1], (r.logz[-1], truth, r.logzerr[-1])
    assert r.n_stuck == 0


def test_slice_scale_rule_pinned():
    assert ns.update_scale_slice(1.0, 10, 5) == 1.0                    # as many expansions as two contractions: unchanged
    assert ns.update_scale_slice(0.8, 30, 10) == pytest.approx(0.8 * 30 / 20, rel=1e-15)
    assert ns.update_scale_slice(2.0, 3, 12) == pytest.approx(2.0 * 3 / 24, rel=1e-15)
    assert ns.update_scale_slice(1.5, 4, 0) == pytest.approx(1.5 * 4 / 2, rel=1e-15)      # max(Cn, 1)
    assert ns.update_scale_slice(1.0, 0, 7) == 0.5 and ns.update_scale_slice(1.0, 0, 0) == 0.5   # E = 0: halved
    assert ns.update_scale_slice(9.0, 100, 1) == ns.SCALE_MAX == 10.0
    assert ns.update_scale_slice(1.5e-4, 0, 3) == ns.SCALE_MIN == 1e-4
    assert ns.update_scale_slice(2e-4, 1, 50) == 1e-4
    # the random walk's rule is what it was
    assert ns.update_scale(1.0, 0.8, 2) == pytest.approx(math.exp(0.3), rel=1e-15)
    assert ns.update_scale(9.9, 1.0, 1) == 10.0 and ns.update_scale(1.5e-4, 0.0, 1) == 1e-4


def test_sampler_applies_the_slice_scale_rule_and_counts_capped_walks():
    class Fixed:
        ndim = 2

        def rslice(self, call, u0, logl0, lstar, chol, scale, slices):
            K = len(u0)
            self.seen = (call, scale, slices)
            one = np.ones(K, int)
            return u0, logl0, 7 * one, 3 * one, 2 * one, np.arange(K) % 2        # every second walk capped once
    s = ns.NestedSampler(Fixed(), 10, sample="rslice", slices=5)
    u0 = np.full((4, 2), 0.5)
    s._walk(u0, np.zeros(4), -1.0, np.eye(2))
    assert s.backend.seen == (0, 1.0, 5) and s.call == 1
    assert s.ncall == 28 and s.n_stuck == 2
    assert s.scale == pytest.approx(12 / 16, rel=1e-15)
    with pytest.raises(ValueError):
        ns.NestedSampler(Fixed(), 10, sample="slice")


def test_run_dynesty_still_refuses_other_sample_methods(tmp_path):
    from alabi_amd import SurrogateModel
    sm = SurrogateModel(lnlike_fn=lambda t: -0.5 * float(np.sum(np.asarray(t) ** 2)), bounds=[(-1, 1), (-1, 1)],
                        savedir=str(tmp_path), verbose=False, random_state=0)
    for sample in ("hslice", "unif"):
        with pytest.raises(NotImplementedError, match="random walk"):
            sm.run_dynesty(like_fn="true", sampler_kwargs={"sample": sample})
    sig = inspect.signature(SurrogateModel.run_dynesty)
    ref = ("(self, like_fn=None, prior_transform=None, mode='dynamic', sampler_kwargs={}, run_kwargs={}, multi_proc=False, "
           "save_iter=None, prior_transform_comment=None, samples_file=None, min_ess=10000)")
    assert str(sig) == ref
