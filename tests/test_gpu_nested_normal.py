"""Gaussian priors fused into the nested-sampling kernels (alabi_ns_set_normal_prior; the reference's prior_transform_normal,
alabi/utility.py:381-482): the device inverse normal CDF against 40-digit values, the walk and the slice move against their NumPy
replays with the transformed likelihood, the split path, the empty mask, and run_dynesty's evidence under a Gaussian prior."""
import functools
import math
import os
from fractions import Fraction
from functools import partial

import numpy as np
import pytest
from scipy.special import ndtri

from conftest import make_problem
from nested_replay_numpy import replay_slice, replay_walk

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ndtri_truth.npz")
K, WALKS, SEED, CALL = 64, 25, 0x1234_5678_9ABC, 7
MEAN, STD = 0.5, 0.7


# ------------------------------------------------------------------ shared inputs and references (computed once)
@functools.lru_cache(maxsize=None)
def _oracle(N, d, kernel="ExpSquaredKernel"):
    from oracle.gp_oracle import OracleGP
    X, y, h = make_problem(N, d, 3, log_wn=-4.0)
    o = OracleGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel).compute(X)
    return X, y, h, o


def _gp(N, d, kernel="ExpSquaredKernel"):
    from alabi_amd import HipGP
    X, y, h, o = _oracle(N, d, kernel)
    g = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel)
    g.compute(X)
    return g, o, y


def _prior(d, normal, decreasing=False):
    """(box [d,2], (mean [d], std [d]), theta(u)): box +-3, N(0.5, 0.7) on the coordinates ``normal``; ``decreasing`` flips the
    box and the sign of std, as a decreasing affine theta scaler does."""
    from alabi_amd import utility as ut
    box = np.array([[3.0, -3.0] if decreasing else [-3.0, 3.0]] * d)
    on = np.zeros(d, dtype=bool)
    on[list(normal)] = True
    mean, std = np.where(on, MEAN, np.nan), np.where(on, -STD if decreasing else STD, np.nan)
    if decreasing:            # scipy's norm.ppf refuses a negative scale: the same map written out
        def theta(u):
            return np.where(on, MEAN - STD * ndtri(u), box[:, 0] + u * (box[:, 1] - box[:, 0]))
    else:
        data = [(MEAN, STD) if k else (None, None) for k in on]
        theta = partial(ut.prior_transform_normal, bounds=box, data=data)
    return box, (mean, std), theta


def _starts(logl_fn, d, n, rng):
    u = rng.random((4 * n, d))
    l = logl_fn(u)
    lstar = float(np.quantile(l, 0.5))
    keep = np.flatnonzero(l > lstar)[:n]
    return u[keep], l[keep], lstar, np.linalg.cholesky(np.cov(u.T))


WALK_CASES = [(400, 4, "ExpSquaredKernel", 1, (0,), False), (400, 5, "ExpSquaredKernel", 1, (4,), False),
              (400, 4, "ExpSquaredKernel", 1, (0, 1, 2, 3), False), (400, 4, "Matern52Kernel", 1, (1, 2), False),
              (400, 18, "ExpSquaredKernel", 1, (0, 17), False), (5000, 10, "ExpSquaredKernel", 2, (3,), False),
              (400, 4, "ExpSquaredKernel", 1, (0, 2), True)]
WALK_SCALE = {4: 0.6, 5: 0.6, 10: 0.6, 18: 0.3}
SLICE_CASES = [(400, 4, (0, 3)), (400, 18, (5,))]


@functools.lru_cache(maxsize=None)
def walk_case(N, d, kernel, normal, decreasing):
    """Inputs and NumPy replay of one walk case (no GPU needed)."""
    X, y, h, o = _oracle(N, d, kernel)
    box, prior, theta = _prior(d, normal, decreasing)
    logl_fn = lambda uu: o.predict(y, theta(uu))  # noqa: E731
    u0, l0, lstar, chol = _starts(logl_fn, d, K, np.random.default_rng(1))
    ref = replay_walk(SEED, CALL, 0, u0, l0, lstar, chol, WALK_SCALE[d], WALKS, logl_fn)
    return (box, prior, u0, l0, lstar, chol), ref


@functools.lru_cache(maxsize=None)
def slice_case(N, d, normal):
    X, y, h, o = _oracle(N, d)
    box, prior, theta = _prior(d, normal)
    logl_fn = lambda uu: o.predict(y, theta(uu))  # noqa: E731
    u0, l0, lstar, chol = _starts(logl_fn, d, K, np.random.default_rng(1))
    ref = replay_slice(SEED, CALL, 0, u0, l0, lstar, chol, 1.0, 3 + d, logl_fn)
    return (box, prior, u0, l0, lstar, chol), ref


# ------------------------------------------------------------------ 1. the device inverse normal CDF
def test_device_ndtri_accuracy_and_uniform_columns():
    """x = ndtri(u) on the normal columns through backend.transform (the walks' own device function) against 40-digit values
    (tests/golden/make_golden_ndtri.py).  Measure |x - truth| / max(1, |truth|); bound 8 x the same measure of
    scipy.special.ndtri (3.1e-16 with scipy 1.15.3): room for another few-ulp rational approximation, seven orders below a wrong
    coefficient or branch.  The uniform columns are fma(u, width, lo), bit for bit."""
    from alabi_amd.nested import GPUWalkBackend
    z = np.load(GOLDEN)
    u, truth = z["u"], z["truth"]
    assert len(u) >= 100 and 2.0 ** -54 in u and u.min() == 1e-300 and u.max() == 1.0 - 2.0 ** -53
    g, o, y = _gp(400, 4)
    box = np.array([[-3.0, 3.0], [-1.25, 2.2], [0.7, -3.1], [-3.0, 3.0]])
    nan = np.nan
    be = GPUWalkBackend(g, y, box, seed=1, to_theta=lambda v: v, normal_prior=([0.0, nan, nan, 0.0], [1.0, nan, nan, 1.0]))
    x = be.transform(np.repeat(u[:, None], 4, axis=1))
    be.close()
    assert x.shape == (len(u), 4)
    measure = lambda v: np.abs(v - truth) / np.maximum(1.0, np.abs(truth))  # noqa: E731
    e_ref = float(measure(ndtri(u)).max())
    e_dev = max(float(measure(x[:, 0]).max()), float(measure(x[:, 3]).max()))
    print("ndtri: device max error %.3e, scipy %.3e, bound %.3e" % (e_dev, e_ref, 8 * e_ref))
    assert np.array_equal(x[:, 0], x[:, 3])
    assert 1e-17 < e_ref < 1e-15
    assert e_dev <= 8 * e_ref, (e_dev, e_ref, u[np.argmax(measure(x[:, 0]))])
    for k in (1, 2):
        lo, w = Fraction(float(box[k, 0])), Fraction(float(box[k, 1] - box[k, 0]))      # the width as alabi_ns_create forms it
        want = np.array([float(Fraction(float(v)) * w + lo) for v in u])               # one rounding: the fma
        assert np.array_equal(x[:, k], want), k


# ------------------------------------------------------------------ 2. the walk
@pytest.mark.parametrize("N,d,kernel,path,normal,decreasing", WALK_CASES)
def test_walk_matches_numpy_replay(N, d, kernel, path, normal, decreasing):
    """The criteria of test_gpu_nested.py::test_walk_matches_numpy_replay with logL(u) = oracle(prior_transform_normal(u))."""
    from alabi_amd.nested import GPUWalkBackend
    (box, prior, u0, l0, lstar, chol), (ur, lr, nr, er) = walk_case(N, d, kernel, normal, decreasing)
    g, o, y = _gp(N, d, kernel)
    be = GPUWalkBackend(g, y, box, seed=SEED, to_theta=lambda u: u, normal_prior=prior)
    u, l, nacc, nev = be.walk(CALL, u0, l0, lstar, chol, WALK_SCALE[d], WALKS)
    assert be.last_path() == path
    be.close()
    print(N, d, kernel, normal, "acc", nacc.sum(), "ev", nev.sum(), "du", np.max(np.abs(u - ur)),
          "dl", np.max(np.abs(l - lr) / np.abs(lr)))
    assert np.array_equal(nacc, nr) and np.array_equal(nev, er)
    assert nacc.sum() > 0 and (nacc == 0).sum() < K
    assert np.max(np.abs(u - ur)) <= 1e-13
    assert np.max(np.abs(l - lr) / np.abs(lr)) <= 1e-12


# ------------------------------------------------------------------ 3. the slice move
@pytest.mark.parametrize("N,d,normal", SLICE_CASES)
def test_slice_matches_numpy_replay(N, d, normal):
    """The criteria of test_gpu_nested_slice.py::test_slice_kernel_matches_numpy_replay; d = 18 runs the 256-lane bucket."""
    from alabi_amd.nested import GPUWalkBackend
    (box, prior, u0, l0, lstar, chol), (ur, lr, ner, nxr, ncr, ncapr) = slice_case(N, d, normal)
    assert ncapr.sum() == 0 and nxr.sum() >= 1 and ncr.sum() >= 1
    g, o, y = _gp(N, d)
    be = GPUWalkBackend(g, y, box, seed=SEED, to_theta=lambda u: u, normal_prior=prior)
    u, l, nev, nexp, ncon, ncap = be.rslice(CALL, u0, l0, lstar, chol, 1.0, 3 + d)
    assert be.last_path() == 1
    be.close()
    print(N, d, normal, "evals", nev.sum(), "exp", nexp.sum(), "con", ncon.sum(), "du", np.max(np.abs(u - ur)),
          "dl", np.max(np.abs(l - lr) / np.abs(lr)))
    assert np.array_equal(nev, ner) and np.array_equal(nexp, nxr) and np.array_equal(ncon, ncr) and np.array_equal(ncap, ncapr)
    assert np.max(np.abs(u - ur)) <= 1e-13
    assert np.max(np.abs(l - lr) / np.abs(lr)) <= 1e-12


# ------------------------------------------------------------------ 4. fused = split
def test_split_path_replays_the_fused_walk():
    """The same backend around host_loglike = logl(prior_transform_normal(u)) (the host path) and the same seed: the replay's and
    the fused kernel's walk, as test_gpu_nested.py::test_split_path_replays_the_fused_draws."""
    from alabi_amd.nested import GPUWalkBackend
    g, o, y = _gp(400, 4)
    box, prior, theta = _prior(4, (1,))
    logl_fn = lambda uu: o.predict(y, theta(uu))  # noqa: E731
    u0, l0, lstar, chol = _starts(logl_fn, 4, 40, np.random.default_rng(4))
    be = GPUWalkBackend(g, y, box, seed=77, to_theta=lambda u: u, host_loglike=logl_fn)
    u, l, nacc, nev = be.walk(2, u0, l0, lstar, chol, 0.6, WALKS)
    ur, lr, nr, er = replay_walk(77, 2, 0, u0, l0, lstar, chol, 0.6, WALKS, logl_fn)
    assert np.array_equal(nacc, nr) and np.array_equal(nev, er) and be.host_calls == er.sum()
    assert np.max(np.abs(u - ur)) <= 1e-13
    assert np.max(np.abs(l - lr) / np.abs(lr)) <= 1e-12
    bf = GPUWalkBackend(g, y, box, seed=77, to_theta=lambda u: u, normal_prior=prior)
    uf, lf, naf, nef = bf.walk(2, u0, l0, lstar, chol, 0.6, WALKS)
    assert np.array_equal(naf, nacc) and np.array_equal(nef, nev) and 0 < naf.sum()
    assert np.max(np.abs(u - uf)) <= 1e-13 and np.max(np.abs(l - lf) / np.abs(lf)) <= 1e-12
    be.close()
    bf.close()


# ------------------------------------------------------------------ 5. the empty mask, the prior draw
def test_empty_mask_is_the_uniform_backend_bit_for_bit():
    from alabi_amd.nested import GPUWalkBackend
    g, o, y = _gp(400, 4)
    box = np.array([[-3.0, 3.0]] * 4)
    nan4 = np.full(4, np.nan)
    a = GPUWalkBackend(g, y, box, seed=99, to_theta=lambda u: u)
    b = GPUWalkBackend(g, y, box, seed=99, to_theta=lambda u: u, normal_prior=(nan4, nan4))
    (ua, la), (ub, lb) = a.prior(0, 128), b.prior(0, 128)
    assert np.array_equal(ua, ub) and np.array_equal(la, lb)
    lstar = float(np.quantile(la, 0.5))
    keep = np.flatnonzero(la > lstar)
    chol = np.linalg.cholesky(np.cov(ua.T))
    wa, wb = a.walk(3, ua[keep], la[keep], lstar, chol, 0.5, WALKS), b.walk(3, ua[keep], la[keep], lstar, chol, 0.5, WALKS)
    assert wa[2].sum() > 0 and all(np.array_equal(x, z) for x, z in zip(wa, wb))
    sa, sb = a.rslice(4, ua[keep], la[keep], lstar, chol, 1.0, 7), b.rslice(4, ua[keep], la[keep], lstar, chol, 1.0, 7)
    assert sa[2].sum() > 0 and all(np.array_equal(x, z) for x, z in zip(sa, sb))
    assert np.array_equal(a.transform(ua), b.transform(ua))
    a.close()
    b.close()


def test_prior_draw_with_normal_coordinates():
    from alabi_amd.nested import GPUWalkBackend
    g, o, y = _gp(400, 4)
    box, prior, theta = _prior(4, (0, 3))
    be = GPUWalkBackend(g, y, box, seed=5, to_theta=theta, normal_prior=prior)
    u, l = be.prior(1, 256)
    assert np.all((u >= 0) & (u < 1))
    assert np.allclose(l, o.predict(y, theta(u)), rtol=1e-12, atol=0)
    x = be.transform(u)
    # |ndtri| <= 8.4 on [2^-54, 1), std 0.7: the device's ndtri bound (8 x 3.1e-16 relative), scipy's own error and the roundings
    # of the two maps at |x| <= 6.4 come to 1.8e-14
    assert np.max(np.abs(x - theta(u))) <= 2e-14
    # std == 0 and a non-finite std on a normal coordinate are refused by the library
    from alabi_amd._lib import AlabiHipError
    for bad in (0.0, np.nan, np.inf):
        bb = GPUWalkBackend(g, y, box, seed=5, to_theta=theta, normal_prior=(prior[0], np.where(np.isfinite(prior[1]), bad, np.nan)))
        with pytest.raises(AlabiHipError):
            bb.prior(1, 4)
    be.close()


# ------------------------------------------------------------------ 6. run_dynesty
def _gauss2(theta):
    t = np.asarray(theta, dtype=float).reshape(-1, 2)
    S = np.array([[1.0, 0.4], [0.4, 0.6]])
    r = t - np.array([0.5, -0.3])
    out = -0.5 * np.einsum("ni,ij,nj->n", r, np.linalg.inv(S), r)
    return out if np.ndim(theta) == 2 else float(out[0])


def _gauss2_neg(theta):
    return _gauss2(theta) - 5.0                   # strictly negative: nlog_scaler's domain


DATA2 = [(None, None), (0.0, 1.0)]


def _model(fn, savedir, **gp_kwargs):
    """The 2-D surrogate of test_gpu_nested.py::sm2 and the quadrature of exp(surrogate) pi(theta) over [-4, 4] x [-8, 8]
    (mean +- 8 sigma of the un-truncated normal on theta_2), pi = (1 / 8) N(theta_2; 0, 1): log Z, posterior mean and covariance."""
    from alabi_amd import SurrogateModel
    sm = SurrogateModel(lnlike_fn=fn, bounds=[(-4.0, 4.0), (-4.0, 4.0)], savedir=savedir, verbose=False, random_state=3, cache=True)
    sm.init_samples(ntrain=200)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1, **gp_kwargs)
    n = 1000
    c1 = -4.0 + (np.arange(n) + 0.5) * (8.0 / n)
    c2 = -8.0 + (np.arange(2 * n) + 0.5) * (16.0 / (2 * n))
    XX, YY = np.meshgrid(c1, c2, indexing="ij")
    pts = np.stack([XX.ravel(), YY.ravel()], axis=1)
    lw = np.asarray(sm.surrogate_log_likelihood(pts)) - math.log(8.0) - 0.5 * pts[:, 1] ** 2 - 0.5 * math.log(2 * math.pi)
    m = lw.max()
    w = np.exp(lw - m)
    logz_grid = m + math.log(w.sum()) + 2 * math.log(8.0 / n)
    w /= w.sum()
    mean = w @ pts
    cov = (pts - mean).T @ ((pts - mean) * w[:, None])
    return sm, logz_grid, mean, cov


@pytest.fixture(scope="module")
def sm2(tmp_path_factory):
    return _model(_gauss2, str(tmp_path_factory.mktemp("nsn2")))


@pytest.fixture(scope="module")
def sm2_nlog(tmp_path_factory):
    from alabi_amd import utility as ut
    return _model(_gauss2_neg, str(tmp_path_factory.mktemp("nsn2n")), y_scaler=ut.nlog_scaler)


def _check_run(sm, logz_grid, mean, cov):
    assert sm.dynesty_path == "fused"
    r = sm.dynesty_results
    print(r.logz[-1], logz_grid, r.logzerr[-1], r.ncall, r.niter)
    assert abs(r.logz[-1] - logz_grid) <= 3 * r.logzerr[-1] + 0.02, (r.logz[-1], logz_grid, r.logzerr[-1])
    s = sm.dynesty_samples
    sd = np.sqrt(np.diag(cov))
    assert np.all(np.abs(s.mean(0) - mean) < 0.1 * sd + 3 * sd / math.sqrt(len(s) / 10))
    assert np.allclose(np.cov(s.T), cov, atol=0.15)


@pytest.mark.parametrize("mode,sample", [("static", "rwalk"), ("dynamic", "rwalk"), ("static", "rslice")])
def test_evidence_2d_normal_prior_matches_grid(sm2, mode, sample):
    from alabi_amd import utility as ut
    sm, logz_grid, mean, cov = sm2
    pt = partial(ut.prior_transform_normal, bounds=sm.bounds, data=DATA2)
    sm.run_dynesty(prior_transform=pt, mode=mode, sampler_kwargs={"seed": 11, "sample": sample}, min_ess=0)
    assert sm.dynesty_sampler.sample == sample
    _check_run(sm, logz_grid, mean, cov)


def test_evidence_2d_normal_prior_behind_the_nlog_map(sm2_nlog):
    from alabi_amd import utility as ut
    sm, logz_grid, mean, cov = sm2_nlog
    assert str(sm.y_scaler) == "nlog_scaler"
    pt = partial(ut.prior_transform_normal, bounds=sm.bounds, data=DATA2)
    sm.run_dynesty(prior_transform=pt, mode="static", sampler_kwargs={"seed": 11}, min_ess=0)
    _check_run(sm, logz_grid, mean, cov)
