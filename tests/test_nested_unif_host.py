"""Host side of the uniform-in-ellipsoids move (alabi_amd/nested.py: bounding_ellipsoids, NestedSampler(sample="unif")) with the
NumPy model of the device move (tests/unif_numpy.py): the bounds, the thinning that makes the union uniform, the evidence of
problems with a known log Z, the sampler's bookkeeping, and run_pymultinest's signature and argument checks
(alabi/core.py:2790-3238)."""
import inspect
import math
import warnings

import numpy as np
import pytest

from alabi_amd import nested as ns
from rslice_numpy import separable_gaussian
from unif_numpy import GeneratorUnifDraws, UnifCubeBackend, candidates


# ------------------------------------------------------------------------------------------------------------------- bounds
def _radii2(ells, e, p):
    y = np.einsum("ki,ni->nk", ells.inv_axes[e], p - ells.centres[e])
    return np.sum(y * y, axis=1)


@pytest.mark.parametrize("d,enlarge", [(2, 1.25), (3, 1.0), (7, 2.0)])
def test_one_ellipsoid_holds_every_point_tightly(d, enlarge):
    rng = np.random.default_rng(d)
    p = rng.standard_normal((40 * d, d)) @ rng.standard_normal((d, d)) * 0.05 + 0.5
    ells = ns.bounding_ellipsoids(p, "single", enlarge)
    assert len(ells) == 1 and ells.cum.shape == (1,) and ells.cum[-1] == 1.0
    r2 = _radii2(ells, 0, p)
    top = enlarge ** (-2.0 / d)
    assert np.all(r2 <= top * (1 + 1e-12)) and np.max(r2) >= top * (1 - 1e-12)
    assert np.allclose(ells.inv_axes[0] @ ells.axes[0], np.eye(d), rtol=0, atol=1e-12)
    assert np.array_equal(ells.axes[0], np.tril(ells.axes[0])) and np.array_equal(ells.inv_axes[0], np.tril(ells.inv_axes[0]))
    const = 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d + 1)
    assert abs(ells.logvol[0] - (np.linalg.slogdet(ells.axes[0])[1] + const)) < 1e-12
    # the volume is `enlarge` times that of the tight ellipsoid
    tight = ns.bounding_ellipsoids(p, "single", 1.0)
    assert abs(ells.logvol[0] - tight.logvol[0] - math.log(enlarge)) < 1e-12


def test_multi_splits_separated_clusters_only():
    rng = np.random.default_rng(1)
    one = rng.standard_normal((400, 3))
    assert len(ns.bounding_ellipsoids(one, "multi")) == 1
    a, b = rng.standard_normal((200, 3)), rng.standard_normal((200, 3)) + np.array([10.0, 0.0, 0.0])
    two = np.concatenate([a, b])[rng.permutation(400)]
    ells = ns.bounding_ellipsoids(two, "multi")
    assert len(ells) == 2 and ells.cum[-1] == 1.0 and 0.0 < ells.cum[0] < 1.0
    left = int(np.argmin(ells.centres[:, 0]))
    for e, own, other in ((left, a, b), (1 - left, b, a)):
        assert np.all(_radii2(ells, e, own) <= 1.0) and np.all(_radii2(ells, e, other) > 1.0)
    assert len(ns.bounding_ellipsoids(two, "single")) == 1
    assert len(ns.bounding_ellipsoids(two, "multi", max_ellipsoids=1)) == 1
    d = 3
    few = np.concatenate([a[:6], b[:4 * d - 1 - 6]])                  # 4d - 1 points are never split
    assert few.shape[0] == 4 * d - 1 and len(ns.bounding_ellipsoids(few, "multi")) == 1
    # deterministic: no generator involved
    again = ns.bounding_ellipsoids(two, "multi")
    assert np.array_equal(again.axes, ells.axes) and np.array_equal(again.cum, ells.cum)
    with pytest.raises(ValueError):
        ns.bounding_ellipsoids(two, "balls")


def test_multi_respects_the_budget():
    rng = np.random.default_rng(2)
    at = ((0.1, 0.45), (0.1, 0.55), (0.9, 0.45), (0.9, 0.55))       # two well separated pairs: the root splits, then each pair does
    blobs = np.concatenate([0.005 * rng.standard_normal((60, 2)) + c for c in at])
    assert len(ns.bounding_ellipsoids(blobs, "multi")) == 4
    for cap in (1, 2, 3):
        assert len(ns.bounding_ellipsoids(blobs, "multi", max_ellipsoids=cap)) == cap
    assert len(ns.bounding_ellipsoids(blobs, "multi", max_ellipsoids=1000)) == 4      # clipped to the device limit, not an error


# ------------------------------------------------------------------------------------------------------------------ thinning
def test_thinning_makes_the_union_uniform():
    r, D = 0.2, 0.2
    centres = np.array([[0.5 - D / 2, 0.5], [0.5 + D / 2, 0.5]])
    ells = ns.Ellipsoids(centres, np.stack([r * np.eye(2)] * 2), np.stack([np.eye(2) / r] * 2), np.zeros(2))
    assert ells.cum[0] == 0.5 and ells.cum[1] == 1.0
    lens = 2 * r * r * math.acos(D / (2 * r)) - 0.5 * D * math.sqrt(4 * r * r - D * D)
    union = 2 * math.pi * r * r - lens
    p_thin, p_raw = lens / union, 2 * lens / (union + lens)
    n = 200000
    for thin, expect in ((True, p_thin), (False, p_raw)):
        u, status, _ = candidates(ells, np.arange(n), GeneratorUnifDraws(np.random.default_rng(5), 2), thin=thin)
        assert np.all(status != 0) and (thin or np.all(status == 2))      # the discs lie inside the cube
        kept = u[status == 2]
        both = (np.sum((kept - centres[0]) ** 2, axis=1) <= r * r) & (np.sum((kept - centres[1]) ** 2, axis=1) <= r * r)
        sigma = math.sqrt(expect * (1 - expect) / len(kept))
        assert abs(both.mean() - expect) <= 4 * sigma, (thin, both.mean(), expect, sigma)
        assert abs(p_thin - p_raw) > 20 * sigma                           # the test can tell the two apart
        # every kept point lies in the union
        assert np.all((np.sum((kept - centres[0]) ** 2, axis=1) <= r * r * (1 + 1e-12))
                      | (np.sum((kept - centres[1]) ** 2, axis=1) <= r * r * (1 + 1e-12)))


# ------------------------------------------------------------------------------------------------------------------ evidence
_A3 = np.array([[1.0, 0.6, 0.2], [0.6, 1.5, -0.4], [0.2, -0.4, 0.8]])
_MU3 = np.array([0.3, -0.5, 0.1])


def _gauss3(theta):
    r = theta - _MU3
    norm = -0.5 * (3 * math.log(2 * math.pi) + np.linalg.slogdet(_A3)[1])
    return norm - 0.5 * np.einsum("ni,ij,nj->n", r, np.linalg.inv(_A3), r)


def _two_modes(theta):
    a = -0.5 * np.sum((theta - np.array([5.0, 0.0])) ** 2, axis=1)
    b = -0.5 * np.sum((theta + np.array([5.0, 0.0])) ** 2, axis=1)
    return np.logaddexp(a, b) + math.log(0.5) - math.log(2 * math.pi)


def _run(be, nlive, seed, dynamic=False, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)              # nlive >= 50 d in every evidence run: no warning
        s = ns.NestedSampler(be, nlive, dynamic=dynamic, seed=seed, sample="unif", **kw)
    r = s.run_nested(dlogz=0.1, n_effective=3000, maxbatch=3) if dynamic else s.run_nested(dlogz=0.1)
    assert r.status in (("n_effective", "maxbatch") if dynamic else ("converged",))
    assert r.ncall / r.niter < 25 and r.n_stuck == 0
    return s, r


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("dynamic", [False, True])
def test_evidence_of_correlated_gaussian_in_a_box(dynamic, seed):
    be = UnifCubeBackend(_gauss3, np.full(3, -6.0), np.full(3, 6.0), seed)
    s, r = _run(be, 300, seed, dynamic)
    logz_true = -3 * math.log(12.0)
    print("3-D z =", (r.logz[-1] - logz_true) / r.logzerr[-1], "ncall/niter", r.ncall / r.niter)
    assert abs(r.logz[-1] - logz_true) <= 3 * r.logzerr[-1], (r.logz[-1], logz_true, r.logzerr[-1])
    eq = r.samples_equal(np.random.default_rng(0))
    assert np.allclose(eq.mean(0), _MU3, atol=0.25)
    assert np.allclose(np.cov(eq.T), _A3, atol=0.35)
    assert len(s.n_ellipsoids) > 0 and max(s.n_ellipsoids) <= 32


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_evidence_of_separable_gaussian_10d(seed):
    logl_theta, lo, hi, logz_true = separable_gaussian(10)
    s, r = _run(UnifCubeBackend(logl_theta, lo, hi, seed), 500, seed)
    print("10-D z =", (r.logz[-1] - logz_true) / r.logzerr[-1], "ncall/niter", r.ncall / r.niter)
    assert abs(r.logz[-1] - logz_true) <= 3 * r.logzerr[-1], (r.logz[-1], logz_true, r.logzerr[-1])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_evidence_of_two_modes_multi_beats_single(seed):
    lo, hi = np.full(2, -10.0), np.full(2, 10.0)
    logz_true = -math.log(400.0)
    s, r = _run(UnifCubeBackend(_two_modes, lo, hi, seed), 200, seed, bound="multi")
    print("two modes z =", (r.logz[-1] - logz_true) / r.logzerr[-1], "ncall/niter", r.ncall / r.niter)
    assert abs(r.logz[-1] - logz_true) <= 3 * r.logzerr[-1], (r.logz[-1], logz_true, r.logzerr[-1])
    w = r.importance_weights()
    assert abs(np.sum(w[r.samples[:, 0] > 0]) / np.sum(w) - 0.5) <= 0.06
    assert max(s.n_ellipsoids) >= 2
    s1, r1 = _run(UnifCubeBackend(_two_modes, lo, hi, seed), 200, seed, bound="single")
    assert max(s1.n_ellipsoids) == 1
    assert r.ncall / r.niter < r1.ncall / r1.niter


# --------------------------------------------------------------------------------------------------------------- bookkeeping
class FakeUnifBackend:
    """prior: a fixed grid of logL; unif: K points each with a logL just above L*, 3 evaluations and 5 candidates per point.
    After ``short_at`` calls it returns one point fewer than asked."""
    ndim = 2

    def __init__(self, short_at=None):
        self.calls, self.short_at = [], short_at

    def theta(self, u):
        return np.asarray(u)

    def prior(self, call, n):
        self.calls.append(("prior", call, n))
        g = (np.arange(n) + 0.5) / n
        return np.stack([g, g[::-1]], axis=1), -10.0 + 5.0 * g

    def unif(self, call, ells, lstar, K):
        self.calls.append(("unif", call, len(ells), K))
        k = K - 1 if (self.short_at is not None and len(self.calls) - 1 >= self.short_at) else K
        t = (np.arange(k) + 1.0) / (K + 1)
        up = 0.3 * (1 - math.exp(lstar))                         # logL -> 0 from below: the run converges
        return np.stack([0.5 + 0.01 * t, 0.5 - 0.01 * t], axis=1), lstar + t * min(1.0, -lstar) * up, 3 * k, 5 * k


def test_sampler_bookkeeping_with_a_fixed_backend():
    be = FakeUnifBackend()
    s = ns.NestedSampler(be, 120, batch=20, seed=0, sample="unif", bound="single")
    r = s.run_nested(dlogz=0.5, maxiter=400)
    iters = r.niter // 20
    assert r.niter == 400 and r.status == "maxiter" and iters == 20
    assert be.calls[0] == ("prior", 0, 120)
    assert [c[1] for c in be.calls[1:]] == list(range(1, iters + 1)) and s.call == iters + 1
    assert all(c[0] == "unif" and c[2] == 1 and c[3] == 20 for c in be.calls[1:])
    assert s.n_ellipsoids == [1] * iters
    assert r.ncall == 120 + 3 * 20 * iters and r.n_stuck == 0 and s.scale == 1.0
    assert "n_ellipsoids" not in ns.NestedResults._FIELDS and len(ns.NestedResults._FIELDS) == 16


def test_short_return_ends_the_run_as_inefficient():
    be = FakeUnifBackend(short_at=3)
    s = ns.NestedSampler(be, 120, batch=20, seed=0, sample="unif")
    with pytest.warns(UserWarning, match="19 of 20"):
        r = s.run_nested(dlogz=1e-6)
    assert r.status == "inefficient" and r.niter == 60
    assert len(r.logl) == 60 + 100 and np.all(np.diff(r.logl) >= 0)       # the dead points and the 100 survivors
    assert r.ncall == 120 + 2 * 60 + 57


def test_constructor_checks():
    be = FakeUnifBackend()
    with pytest.warns(UserWarning, match="fewer than 50 live points per dimension"):
        ns.NestedSampler(be, 99, sample="unif")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ns.NestedSampler(be, 100, sample="unif")
        ns.NestedSampler(be, 20)                                 # the warning belongs to the ellipsoid move alone
    with pytest.raises(ValueError, match="ndim \\+ 2"):
        ns.NestedSampler(be, 100, batch=97, sample="unif")       # 3 survivors < d + 2 = 4
    with pytest.warns(UserWarning):
        ns.NestedSampler(be, 8, batch=4, sample="unif")          # 4 survivors: allowed
    with pytest.raises(ValueError, match="sample must be"):
        ns.NestedSampler(be, 100, sample="slice")
    with pytest.raises(ValueError, match="bound must be"):
        ns.NestedSampler(be, 100, sample="unif", bound="balls")


def test_rwalk_is_untouched_by_the_new_keywords():
    from test_nested_host import _problem
    out = []
    for kw in ({}, {"bound": "single", "enlarge": 2.0, "max_ellipsoids": 3}):
        be, *_ = _problem(21)
        s = ns.NestedSampler(be, 60, walks=10, seed=22, **kw)
        out.append((s.run_nested(dlogz=0.5), s))
    (a, sa), (b, sb) = out
    for k in ns.NestedResults._FIELDS:
        assert np.array_equal(a[k], b[k]), k
    assert sa.n_ellipsoids == [] and sb.n_ellipsoids == [] and sa.scale == sb.scale


# ----------------------------------------------------------------------------------------------------------- run_pymultinest
def test_run_pymultinest_signature_matches_reference():
    from alabi_amd import SurrogateModel
    ref = ("(self, like_fn=None, prior_transform=None, sampler_kwargs={}, multi_proc=True, prior_transform_comment=None, "
           "samples_file=None, prefix=None, resume=False, n_clustering_params=None, outputfiles_basename=None, min_ess=10000)")
    assert str(inspect.signature(SurrogateModel.run_pymultinest)) == ref


def test_run_pymultinest_rejects_what_is_not_built_before_any_device_call(tmp_path, monkeypatch):
    from alabi_amd import SurrogateModel
    from alabi_amd import nested
    sm = SurrogateModel(lnlike_fn=lambda t: -0.5 * float(np.sum(np.asarray(t) ** 2)), bounds=[(-1, 1), (-1, 1)],
                        savedir=str(tmp_path), verbose=False, random_state=0)
    assert sm.pymultinest_run is False

    def boom(*a, **k):
        raise AssertionError("a backend was built")
    monkeypatch.setattr(nested, "GPUWalkBackend", boom)
    monkeypatch.setattr(sm, "_handle_owner", boom)
    with pytest.raises(NotImplementedError, match="const_efficiency_mode"):
        sm.run_pymultinest(like_fn="true", sampler_kwargs={"const_efficiency_mode": True})
    with pytest.raises(NotImplementedError, match="resume"):
        sm.run_pymultinest(like_fn="true", resume=True)
    with pytest.raises(TypeError, match="nlive"):
        sm.run_pymultinest(like_fn="true", sampler_kwargs={"nlive": 100})
    assert sm.pymultinest_run is False
