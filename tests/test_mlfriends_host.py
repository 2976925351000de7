"""Host side of the MLFriends region (alabi_amd/nested.py: mlfriends_metric, NestedSampler(sample="mlfriends")) with the NumPy model
of the device move (tests/mlfriends_numpy.py): the metric, the bootstrap radius, the uniformity of the accepted points, the evidence
of problems with a known log Z, the efficiency against the ellipsoid move alone, the sampler's bookkeeping, and run_ultranest's
signature, argument checks and keyword mapping (alabi/core.py:3241-3690).  Seeds: 0, 1, 2 throughout, as in
test_nested_unif_host.py."""
import inspect
import math
import warnings

import numpy as np
import pytest

import mlfriends_numpy as mn
from alabi_amd import nested as ns
from rslice_numpy import separable_gaussian
from unif_numpy import GeneratorUnifDraws

SEEDS = [0, 1, 2]


# ------------------------------------------------------------------------------------------------------------------- metric
def _two_clusters(rng, n=300):
    A = np.array([[0.02, 0.0], [0.012, 0.01]])
    a = rng.standard_normal((n, 2)) @ A.T + np.array([0.25, 0.3])
    b = rng.standard_normal((n, 2)) @ A.T + np.array([0.75, 0.7])
    planted = np.repeat([0, 1], n)
    perm = rng.permutation(2 * n)
    return np.concatenate([a, b])[perm], planted[perm], A


def test_metric_is_the_within_cluster_covariance():
    p, planted, A = _two_clusters(np.random.default_rng(0))
    ells = ns.bounding_ellipsoids(p, "multi")
    assert len(ells) == 2
    labels, minv, w = ns.mlfriends_metric(p, ells)
    first = int(np.argmin(ells.centres[:, 0]))                   # the ellipsoid around the planted cluster 0
    assert np.array_equal(labels == first, planted == 0)
    n, E = p.shape[0], 2
    S = np.linalg.inv(minv) @ np.linalg.inv(minv).T
    within = sum((p[planted == k] - p[planted == k].mean(0)).T @ (p[planted == k] - p[planted == k].mean(0)) for k in (0, 1)) / (n - E)
    assert np.allclose(S, within, rtol=1e-9, atol=0)
    total = np.cov(p.T)
    assert total[0, 0] > 50 * S[0, 0] and np.allclose(S, A @ A.T, rtol=0.25)      # not the total covariance
    assert np.array_equal(minv, np.tril(minv)) and np.allclose(w, p @ minv.T, rtol=0, atol=0)
    # the whitened residuals have unit covariance about their own centres
    r = (p - ells.centres[labels]) @ minv.T
    assert np.allclose(r.T @ r / (n - E), np.eye(2), atol=1e-9)
    # the independent statement of the model agrees
    lm, mm, wm = mn.metric(p, ells)
    assert np.array_equal(lm, labels) and np.allclose(mm, minv, rtol=1e-9) and np.allclose(wm, w, rtol=1e-9)
    # one ellipsoid: the covariance about the mean with n - 1 degrees of freedom
    one = ns.bounding_ellipsoids(p, "single")
    l1, m1, _ = ns.mlfriends_metric(p, one)
    assert np.all(l1 == 0) and np.allclose(np.linalg.inv(m1) @ np.linalg.inv(m1).T, total, rtol=1e-9)


# ------------------------------------------------------------------------------------------------------------------- radius
def test_radius_properties():
    rng = np.random.default_rng(1)
    p = rng.random((120, 3)) * np.array([0.2, 0.5, 0.1]) + 0.3
    ells = ns.bounding_ellipsoids(p, "single")
    _, _, w = ns.mlfriends_metric(p, ells)
    B = 30
    rounds, left = mn.radius2_rounds(w, B, mn.GeneratorIndexDraws(np.random.default_rng(7)))
    assert np.all(left > 0) and np.all(rounds > 0)
    be = mn.MLFriendsCubeBackend(lambda t: np.zeros(len(t)), np.zeros(3), np.ones(3))
    be.index_draws = mn.GeneratorIndexDraws(np.random.default_rng(7))
    r2 = be.mlf_radius(0, w, B)
    assert r2 == np.max(rounds) and np.all(r2 >= rounds)
    # a round's value is a distance between two of the points, the nearest kept neighbour of a point left out
    D = mn.dist2(w, w)
    assert all(np.any(D == v) for v in rounds)
    # invariant under an affine map of the points: the whitening takes it out
    T = rng.standard_normal((3, 3)) + 2 * np.eye(3)
    q = p @ T.T + np.array([3.0, -1.0, 0.5])
    _, _, wq = ns.mlfriends_metric(q, ns.bounding_ellipsoids(q, "single"))
    rq, _ = mn.radius2_rounds(wq, B, mn.GeneratorIndexDraws(np.random.default_rng(7)))
    assert np.max(np.abs(rq - rounds) / rounds) < 1e-9
    # n = 1: nothing can be left out
    r1, l1 = mn.radius2_rounds(w[:1], 5, mn.GeneratorIndexDraws(np.random.default_rng(7)))
    assert np.all(r1 == 0.0) and np.all(l1 == 0)
    # more rounds can only widen it
    r60, _ = mn.radius2_rounds(w, 60, mn.GeneratorIndexDraws(np.random.default_rng(7)))
    assert np.max(r60) >= r2 and np.array_equal(r60[:B], rounds)


# --------------------------------------------------------------------------------------------------------------- uniformity
def test_accepted_points_are_uniform_over_the_ball_covered_cells():
    """One disc as the bound, balls of radius r around fixed live points in a sheared metric.  Cells of a 2-D grid that lie wholly
    inside one ball and the disc must hold equally many accepted points (chi-square); cells wholly outside every ball none."""
    R = 0.45
    ells = ns.Ellipsoids(np.array([[0.5, 0.5]]), np.array([R * np.eye(2)]), np.array([np.eye(2) / R]), np.zeros(1))
    live = np.array([[0.3, 0.35], [0.55, 0.5], [0.7, 0.72], [0.42, 0.7]])
    minv = np.array([[4.0, 0.0], [1.0, 5.0]])
    w, r2 = live @ minv.T, 0.7 ** 2
    n = 400000
    u, status, marg = mn.mlf_candidates(ells, np.arange(n), GeneratorUnifDraws(np.random.default_rng(5), 2), w, minv, r2)
    assert np.array_equal(marg["unif_status"] == 2, np.ones(n, dtype=bool))      # the disc lies inside the cube, one ellipsoid
    kept = u[status == 2]
    assert 0.2 < len(kept) / n < 0.8
    assert np.all(mn.neighbour_margins(kept, w, minv, r2) <= 0.0) and np.all(mn.neighbour_margins(u[status == 1], w, minv, r2) > 0.0)
    G = 25
    edges = np.linspace(0.0, 1.0, G + 1)
    counts, _, _ = np.histogram2d(kept[:, 0], kept[:, 1], bins=[edges, edges])
    allc, _, _ = np.histogram2d(u[:, 0], u[:, 1], bins=[edges, edges])
    cx, cy = np.meshgrid(edges[:-1], edges[:-1], indexing="ij")
    corners = np.stack([np.stack([cx + a / G, cy + b / G], axis=-1) for a in (0, 1) for b in (0, 1)])       # [4, G, G, 2]
    in_disc = np.all(np.sum((corners - 0.5) ** 2, axis=-1) <= R * R, axis=0)
    dw = np.stack([np.sum((corners @ minv.T - wj) ** 2, axis=-1) for wj in w])                                # [n_live, 4, G, G]
    in_one_ball = np.any(np.all(dw <= r2, axis=1), axis=0)                  # balls are convex: four corners inside = the cell inside
    covered = in_disc & in_one_ball
    k = int(covered.sum())
    assert k >= 30
    obs = counts[covered]
    expect = obs.sum() / k
    chi2 = float(np.sum((obs - expect) ** 2 / expect))
    assert expect > 200 and abs(chi2 - (k - 1)) <= 4 * math.sqrt(2 * (k - 1)), (chi2, k)
    # cells wholly outside every ball (centre farther than r plus the largest whitened half diagonal): nothing accepted there,
    # though the ellipsoid move alone puts points there -- the test can tell the two apart
    centre = np.stack([cx + 0.5 / G, cy + 0.5 / G], axis=-1)
    half = max(np.linalg.norm(minv @ np.array([a, b])) for a in (0.5 / G, -0.5 / G) for b in (0.5 / G,))
    dc = np.sqrt(np.stack([np.sum((centre @ minv.T - wj) ** 2, axis=-1) for wj in w]))
    outside = in_disc & np.all(dc > math.sqrt(r2) + half, axis=0)
    assert outside.sum() >= 30 and np.all(counts[outside] == 0) and np.all(allc[outside] > 100)


# ------------------------------------------------------------------------------------------------------------------ evidence
_S2 = np.array([[1.0, 0.4], [0.4, 0.6]])
_MU2 = np.array([0.5, -0.3])


def _gauss2(theta):
    r = theta - _MU2
    return -0.5 * (2 * math.log(2 * math.pi) + np.linalg.slogdet(_S2)[1]) - 0.5 * np.einsum("ni,ij,nj->n", r, np.linalg.inv(_S2), r)


def _two_modes(theta):
    a = -0.5 * np.sum((theta - np.array([3.0, 0.0])) ** 2, axis=1)
    b = -0.5 * np.sum((theta + np.array([3.0, 0.0])) ** 2, axis=1)
    return np.logaddexp(a, b) + math.log(0.5) - math.log(2 * math.pi)


def _rosenbrock(theta):
    return -((1.0 - theta[:, 0]) ** 2 + 100.0 * (theta[:, 1] - theta[:, 0] ** 2) ** 2) / 100.0       # the reference's -rosen(x) / 100


def _rosenbrock_logz(n=2000):
    g = np.linspace(-5.0, 5.0, n + 1)
    c = 0.5 * (g[1:] + g[:-1])
    XX, YY = np.meshgrid(c, c, indexing="ij")
    ll = _rosenbrock(np.stack([XX.ravel(), YY.ravel()], axis=1))
    return math.log(np.sum(np.exp(ll))) - 2 * math.log(n)


def _run(be, nlive, seed, dynamic=False, sample="mlfriends", **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)              # nlive >= 50 d in every evidence run: no warning
        s = ns.NestedSampler(be, nlive, dynamic=dynamic, seed=seed, sample=sample, **kw)
    r = s.run_nested(dlogz=0.1, n_effective=3000, maxbatch=3) if dynamic else s.run_nested(dlogz=0.1)
    assert r.status in (("n_effective", "maxbatch") if dynamic else ("converged",))
    assert r.n_stuck == 0 and len(s.n_ellipsoids) > 0
    assert len(s.radius2) == (len(s.n_ellipsoids) if sample == "mlfriends" else 0) and all(v > 0 for v in s.radius2)
    return s, r


def _within(r, logz_true, what):
    z = (r.logz[-1] - logz_true) / r.logzerr[-1]
    print(what, "z =", z, "ncall/niter", r.ncall / r.niter)
    assert abs(z) <= 3, (what, r.logz[-1], logz_true, r.logzerr[-1])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("dynamic", [False, True])
def test_evidence_of_correlated_gaussian_2d(dynamic, seed):
    be = mn.MLFriendsCubeBackend(_gauss2, np.full(2, -6.0), np.full(2, 6.0), seed)
    s, r = _run(be, 300, seed, dynamic)
    _within(r, -2 * math.log(12.0), "2-D Gaussian")
    eq = r.samples_equal(np.random.default_rng(0))
    assert np.allclose(eq.mean(0), _MU2, atol=0.2) and np.allclose(np.cov(eq.T), _S2, atol=0.3)


@pytest.mark.parametrize("seed", SEEDS)
def test_evidence_of_separable_gaussian_10d(seed):
    logl_theta, lo, hi, logz_true = separable_gaussian(10)
    s, r = _run(mn.MLFriendsCubeBackend(logl_theta, lo, hi, seed), 500, seed)
    _within(r, logz_true, "10-D Gaussian")


@pytest.mark.parametrize("seed", SEEDS)
def test_evidence_and_mode_mass_of_two_modes(seed):
    s, r = _run(mn.MLFriendsCubeBackend(_two_modes, np.full(2, -10.0), np.full(2, 10.0), seed), 400, seed)
    _within(r, -math.log(400.0), "two modes")
    w = r.importance_weights()
    assert abs(np.sum(w[r.samples[:, 0] > 0]) / np.sum(w) - 0.5) <= 0.06
    assert max(s.n_ellipsoids) >= 2


@pytest.mark.parametrize("seed", SEEDS)
def test_rosenbrock_evidence_and_fewer_evaluations_than_the_ellipsoid_move(seed):
    lo, hi = np.full(2, -5.0), np.full(2, 5.0)
    logz_true = _rosenbrock_logz()
    s, r = _run(mn.MLFriendsCubeBackend(_rosenbrock, lo, hi, seed), 400, seed)
    _within(r, logz_true, "Rosenbrock")
    s0, r0 = _run(mn.MLFriendsCubeBackend(_rosenbrock, lo, hi, seed), 400, seed, sample="unif")
    a, b = r.ncall / r.niter, r0.ncall / r0.niter
    print("Rosenbrock evaluations per dead point: mlfriends", a, "unif", b, "ratio", a / b)
    assert a < b


# --------------------------------------------------------------------------------------------------------------- bookkeeping
class FakeMLFBackend:
    """prior: a fixed grid of logL; mlfriends: K points each with a logL just above L*, 3 evaluations and 5 candidates per point;
    mlf_radius: 0.25 + call.  After ``short_at`` calls mlfriends returns one point fewer than asked."""
    ndim = 2

    def __init__(self, short_at=None):
        self.calls, self.short_at = [], short_at

    def theta(self, u):
        return np.asarray(u)

    def prior(self, call, n):
        self.calls.append(("prior", call, n))
        g = (np.arange(n) + 0.5) / n
        return np.stack([g, g[::-1]], axis=1), -10.0 + 5.0 * g

    def mlf_radius(self, call, w, B):
        self.calls.append(("radius", call, w.shape, B))
        return 0.25 + call

    def mlfriends(self, call, ells, w, metric_inv, r2, lstar, K):
        self.calls.append(("mlfriends", call, len(ells), K, w.shape, metric_inv.shape, r2))
        k = K - 1 if (self.short_at is not None and len(self.calls) - 1 >= self.short_at) else K
        t = (np.arange(k) + 1.0) / (K + 1)
        up = 0.3 * (1 - math.exp(lstar))                         # logL -> 0 from below: the run converges
        return np.stack([0.5 + 0.01 * t, 0.5 - 0.01 * t], axis=1), lstar + t * min(1.0, -lstar) * up, 3 * k, 5 * k


def test_sampler_bookkeeping_with_a_fixed_backend():
    be = FakeMLFBackend()
    s = ns.NestedSampler(be, 120, batch=20, seed=0, sample="mlfriends", bound="single", num_bootstraps=7)
    r = s.run_nested(dlogz=0.5, maxiter=400)
    iters = r.niter // 20
    assert r.niter == 400 and r.status == "maxiter" and iters == 20
    assert be.calls[0] == ("prior", 0, 120)
    rad, drw = be.calls[1::2], be.calls[2::2]
    assert [c[1] for c in rad] == list(range(1, iters + 1)) == [c[1] for c in drw] and s.call == iters + 1
    assert all(c == ("radius", c[1], (100, 2), 7) for c in rad)
    assert all(c[0] == "mlfriends" and c[2:] == (1, 20, (100, 2), (2, 2), 0.25 + c[1]) for c in drw)
    assert s.n_ellipsoids == [1] * iters and s.radius2 == [0.25 + k for k in range(1, iters + 1)]
    assert r.ncall == 120 + 3 * 20 * iters and r.n_stuck == 0 and s.scale == 1.0
    assert "radius2" not in ns.NestedResults._FIELDS and len(ns.NestedResults._FIELDS) == 16


def test_short_return_ends_the_run_as_inefficient():
    be = FakeMLFBackend(short_at=5)
    s = ns.NestedSampler(be, 120, batch=20, seed=0, sample="mlfriends")
    with pytest.warns(UserWarning, match="19 of 20"):
        r = s.run_nested(dlogz=1e-6)
    assert r.status == "inefficient" and r.niter == 60 and len(s.radius2) == 3 == len(s.n_ellipsoids)
    assert len(r.logl) == 60 + 100 and np.all(np.diff(r.logl) >= 0)
    assert r.ncall == 120 + 2 * 60 + 57


def test_constructor_checks():
    be = FakeMLFBackend()
    with pytest.warns(UserWarning, match="fewer than 50 live points per dimension"):
        ns.NestedSampler(be, 99, sample="mlfriends")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ns.NestedSampler(be, 100, sample="mlfriends")
    with pytest.raises(ValueError, match="sample='mlfriends'.*ndim \\+ 2"):
        ns.NestedSampler(be, 100, batch=97, sample="mlfriends")
    with pytest.raises(ValueError, match="num_bootstraps"):
        ns.NestedSampler(be, 100, sample="mlfriends", num_bootstraps=0)
    with pytest.raises(ValueError, match="sample must be .*'mlfriends'"):
        ns.NestedSampler(be, 100, sample="friends")
    with pytest.raises(ValueError, match="bound must be"):
        ns.NestedSampler(be, 100, sample="mlfriends", bound="balls")
    assert ns.NestedSampler(be, 100, sample="mlfriends").num_bootstraps == 30


@pytest.mark.parametrize("sample", ["rwalk", "rslice", "unif"])
def test_existing_moves_are_untouched_by_the_new_keyword(sample):
    from rslice_numpy import SliceCubeBackend
    from test_nested_host import _problem
    logl_theta, lo, hi, _ = separable_gaussian(2)
    out = []
    for kw in ({}, {"num_bootstraps": 3}):
        if sample == "unif":
            be = mn.MLFriendsCubeBackend(logl_theta, lo, hi, 4)
        elif sample == "rslice":
            be = SliceCubeBackend(logl_theta, lo, hi, 4)
        else:
            be, *_ = _problem(21)
        s = ns.NestedSampler(be, 100, walks=10, seed=22, sample=sample, **kw)
        out.append((s.run_nested(dlogz=0.5), s))
    (a, sa), (b, sb) = out
    for k in ns.NestedResults._FIELDS:
        assert np.array_equal(a[k], b[k]), k
    assert sa.radius2 == [] and sb.radius2 == [] and sa.scale == sb.scale and sa.n_ellipsoids == sb.n_ellipsoids


# ------------------------------------------------------------------------------------------------------------- run_ultranest
def test_run_ultranest_signature_matches_reference():
    from alabi_amd import SurrogateModel
    ref = ("(self, like_fn=None, prior_transform=None, sampler_kwargs={}, run_kwargs={}, multi_proc=False, "
           "prior_transform_comment=None, samples_file=None, log_dir=None, resume='overwrite', min_ess=10000, slice_steps=0)")
    assert str(inspect.signature(SurrogateModel.run_ultranest)) == ref


def _bare_model(tmp_path):
    from alabi_amd import SurrogateModel
    return SurrogateModel(lnlike_fn=lambda t: -0.5 * float(np.sum(np.asarray(t) ** 2)), bounds=[(-1, 1), (-1, 1)],
                          savedir=str(tmp_path), verbose=False, random_state=0)


def test_run_ultranest_rejects_what_is_not_built_before_any_device_call(tmp_path, monkeypatch):
    from alabi_amd import _lib, nested
    sm = _bare_model(tmp_path)
    assert sm.ultranest_run is False

    def boom(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(nested, "GPUWalkBackend", boom)
    monkeypatch.setattr(sm, "_handle_owner", boom)
    with pytest.raises(NotImplementedError, match="derived_param_names"):
        sm.run_ultranest(like_fn="true", sampler_kwargs={"derived_param_names": ["a"]})
    with pytest.raises(NotImplementedError, match="wrapped_params"):
        sm.run_ultranest(like_fn="true", sampler_kwargs={"wrapped_params": [False, True]})
    with pytest.raises(NotImplementedError, match="region_class"):
        sm.run_ultranest(like_fn="true", run_kwargs={"region_class": object})
    with pytest.raises(TypeError, match="sampler_kwargs.*nlive"):
        sm.run_ultranest(like_fn="true", sampler_kwargs={"nlive": 100})
    with pytest.raises(TypeError, match="run_kwargs.*maxiter"):
        sm.run_ultranest(like_fn="true", run_kwargs={"maxiter": 100})
    assert sm.ultranest_run is False and not hasattr(sm, "ultranest_samples")


def _captured_run(sm, monkeypatch, tmp_path, **call):
    """run_ultranest with the sampler and the backend replaced by recorders: the NestedSampler / run_nested arguments."""
    from alabi_amd import nested
    seen = {}

    class Backend:
        path = "host-callback"

        def __init__(self, *a, **k):
            seen["backend"] = k

        def close(self):
            pass

    class Sampler:
        def __init__(self, backend, nlive, **k):
            seen["nlive"], seen["sampler"] = nlive, k
            self.sample = k.get("sample")

        def run_nested(self, **k):
            seen["run"] = k
            n = 50
            t = np.linspace(0.0, 1.0, n)
            return ns.NestedResults(samples=np.stack([t, t], 1), samples_u=np.stack([t, t], 1), logl=t, logwt=np.zeros(n),
                                    logz=np.full(n, math.log(n) + seen.get("bump", 0.0)), logzerr=np.full(n, 0.1), nbatch=0,
                                    status="converged", niter=n, ncall=n)
    monkeypatch.setattr(nested, "GPUWalkBackend", Backend)
    monkeypatch.setattr(nested, "NestedSampler", Sampler)
    monkeypatch.setattr(sm, "_handle_owner", lambda: (None, None))
    sm.run_ultranest(like_fn="true", **call)
    return seen


def test_run_ultranest_maps_the_reference_keywords(tmp_path, monkeypatch):
    import os
    sm = _bare_model(tmp_path)
    seen = _captured_run(sm, monkeypatch, tmp_path, min_ess=0)
    assert seen["nlive"] == 400
    assert seen["sampler"] == {"dynamic": True, "batch": None, "seed": seen["sampler"]["seed"], "sample": "mlfriends",
                               "num_bootstraps": 30}
    assert seen["run"] == {"dlogz": math.log1p(0.01), "dlogz_init": math.log1p(0.01), "maxiter": None, "maxcall": None,
                           "maxbatch": 1, "n_effective": 400}
    assert sm.ultranest_run and sm.ultranest_path == "host-callback" and sm.ultranest_samples.shape == (50, 2)
    assert np.array_equal(sm.ultranest_weights, np.full(50, 1 / 50)) and sm.ultranest_samples_true is sm.ultranest_samples
    assert sm.ultranest_logz == math.log(50) and sm.ultranest_logz_err == 0.1 and sm.ultranest_runtime >= 0
    f = np.load(f"{sm.savedir}/ultranest_samples_final_true.npz")
    assert sorted(f.files) == ["logz", "logz_err", "samples", "weights"] and np.array_equal(f["weights"], sm.ultranest_weights)
    # nothing is logged: no directory appears, whatever log_dir and resume say
    before = sorted(os.listdir(sm.savedir))
    seen = _captured_run(sm, monkeypatch, tmp_path, min_ess=0, log_dir=str(tmp_path / "logs"), resume="resume", multi_proc=True,
                         sampler_kwargs={"num_bootstraps": 12, "seed": 9, "batch": 50, "ndraw_min": 64, "wrapped_params": [False, False],
                                         "derived_param_names": []},
                         run_kwargs={"min_num_live_points": 250, "frac_remain": 0.5, "max_iters": 1000, "max_ncalls": 5000,
                                     "max_num_improvement_loops": 0, "min_ess": 90, "dlogz": 0.1, "dKL": 0.2, "Lepsilon": 0.01})
    assert sorted(os.listdir(sm.savedir)) == before and not (tmp_path / "logs").exists()
    assert seen["nlive"] == 250 and seen["backend"]["seed"] == 9
    assert seen["sampler"] == {"dynamic": False, "batch": 50, "seed": 9, "sample": "mlfriends", "num_bootstraps": 12}
    assert seen["run"] == {"dlogz": math.log1p(0.5), "maxiter": 1000, "maxcall": 5000}
    for loops, maxbatch in ((3, 3), (-1, 10)):
        seen = _captured_run(sm, monkeypatch, tmp_path, min_ess=0, run_kwargs={"max_num_improvement_loops": loops})
        assert seen["sampler"]["dynamic"] is True and seen["run"]["maxbatch"] == maxbatch
    # slice_steps: the slice move in place of the region draws
    seen = _captured_run(sm, monkeypatch, tmp_path, min_ess=0, slice_steps=5)
    assert seen["sampler"]["sample"] == "rslice" and seen["sampler"]["slices"] == 5 and "num_bootstraps" not in seen["sampler"]
    assert sm.ultranest_sampler.sample == "rslice"
    # the argument min_ess: runs repeat; samples stacked, weights 1 / len(run) per run, log Z of the best run
    seen = _captured_run(sm, monkeypatch, tmp_path, min_ess=120, sampler_kwargs={"seed": 4})
    assert sm.ultranest_samples.shape == (150, 2) and np.allclose(sm.ultranest_weights, 1 / 50) and sm.ultranest_weights.sum() == pytest.approx(3.0)
    assert seen["backend"]["seed"] == 4 + 2 * 1000003 and sm.ultranest_logz == math.log(50)
