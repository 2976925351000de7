"""Nested sampling on the GPU: the static and dynamic samplers behind ``SurrogateModel.run_dynesty``, ``run_pymultinest`` and
``run_ultranest``.

The reference drives dynesty's ``NestedSampler`` / ``DynamicNestedSampler`` (alabi/core.py:2417-2787) for the Bayesian
evidence log Z.  Here the nested-sampling bookkeeping runs on the host in NumPy and the likelihood work -- many independent
constrained random walks, one GP mean per step -- runs in ``ns_walk_kernel`` / ``ns_slice_kernel`` (alabi_amd/csrc/nested.hip)
through a *walk backend*.  The product's only backend is ``GPUWalkBackend``; there is no CPU fallback (tests may pass their own).

Algorithm (static; all in the unit cube u in [0,1]^d, the prior being uniform there)
  * Start.  ``nlive`` points uniform in the cube (device Philox), logL of each.
  * Iteration.  The K live points with the lowest logL die (K = ``batch``, default ceil(nlive / 4): one walk launch per K
    dead points keeps K workgroups busy; K = 1 is dynesty's sequential loop).  Dead point j = 0..K-1 of the batch is
    recorded with n = nlive - j live points, i.e. d log X = -1 / (nlive - j): exactly sequential removal from a shrinking
    live set.  L* is the largest removed logL.  K replacement walks start at survivors drawn uniformly (with replacement)
    by a seeded NumPy generator among the survivors with logL > L* strictly; if there is none (a plateau) the run stops with
    status "plateau" and a warning.
  * Walk.  ``walks`` Metropolis steps (default 25, dynesty's rwalk default): u' = u + scale C z, z ~ N(0, I_d) drawn on the
    device, C the Cholesky factor of the covariance in u of the n - K surviving live points (host, once per iteration;
    the K dead points are left out); accept iff u' lies inside
    the cube and logL(u') > L*.  A walk that accepts nothing returns its start (counted in ``n_stuck``).
  * Scale rule.  After every iteration, with acc = accepted steps / (K walks), scale <- scale exp((acc - 0.5) / (0.5 d)),
    clipped to [1e-4, 10]; the start value is 1 (dynesty's).  Acceptance above 1/2 widens the step, below narrows it, and the
    1/d damping keeps the change per iteration small in high dimension.
  * Slice move (``sample="rslice"``, dynesty's random-direction slice sampling; the move to use above d = 20, where 25
    Metropolis steps no longer decorrelate a walk from its start and log Z comes out high by several logzerr).  One walk =
    ``slices`` slice updates (default 3 (3 + d), see NOTES.md for the calibration).  Each: a direction a = scale C z / |z|;
    an interval [t_l, t_r] = [-r, 1 - r], r ~ U(0,1), along u + t a; stepping out by 1 on each side while the end lies inside
    the cube with logL > L* (one *expansion* each); then t ~ U(t_l, t_r) until the point lies inside the cube with logL > L*,
    every failure pulling the end on its side in to t (one *contraction*).  A slice that has contracted 64 times ends where
    it started and its walk is counted in ``n_stuck``.  Scale rule: with E expansions and Cn contractions over the K walks,
    scale <- scale E / (2 max(Cn, 1)) (halved when E = 0), clipped to [1e-4, 10] (dynesty's).
  * Stop.  log(1 + exp(max logL_live + log X - log Z)) < ``dlogz`` (default 0.5), or ``maxiter`` dead points, or ``maxcall``
    likelihood evaluations (in-cube proposals; the start points count too).
  * Finish (dynesty's add_live).  The remaining live points are appended in ascending logL with n = n_live - j, j = 0..n_live-1.
  * Weights.  log X_i = -sum_{k<=i} 1 / n_k; logwt_i = logaddexp(logL_i, logL_{i-1}) + log((X_{i-1} - X_i) / 2) with
    L_0 = 0, X_0 = 1; log Z = running logsumexp(logwt) (an array, as dynesty reports it); H the information by dynesty's
    recurrence; logzerr_i^2 = sum_{k<=i} (H_k - H_{k-1}) / n_k, which is H / n for a constant live set.

Dynamic mode (the reference's default; ``wt_kwargs`` / ``stop_kwargs`` with pfrac = 1.0 only)
  1. A baseline static run with ``nlive_init`` (default ``nlive``) points, stopped at ``dlogz_init`` (default 0.5).
  2. Up to ``maxbatch`` (default 10) batches, each: the importance weights w = exp(logwt - log Z) of the merged run; [L_lo, L_hi]
     = the logL span of the points with w >= 0.8 max w (dynesty's maxfrac), widened by one point on each side (-inf / the
     largest logL at the ends); ``nlive_batch`` (default ``nlive``) new points with logL > L_lo from walks with L* = L_lo
     started at merged points above L_lo (prior draws when L_lo = -inf); a static loop from there until L* >= L_hi (or the
     static dlogz rule within the batch, or maxiter / maxcall), then add_live.  Merging: the union of all dead points sorted by
     logL; n at each point is the sum over runs of that run's live count there (the n of that run's next point when the run
     covers this logL, else 0); X, the weights, log Z, H and logzerr are recomputed from the merged n.
  3. Stop when the Kish ESS (sum w)^2 / sum w^2 >= ``n_effective`` (default 10000) or after ``maxbatch`` batches.
  4. dynesty's bootstrap stopping rule is not built.

Uniform draws inside bounding ellipsoids (``sample="unif"``: MultiNest's algorithm, the reference's run_pymultinest,
alabi/core.py:2790-3238; dynesty's ``sample="unif"`` with ``bound="single"`` / ``"multi"``)
  * Bounds (host, once per iteration, from the point set the walks take their covariance from).  One ellipsoid {c + A z : |z| <= 1}:
    c the mean, A = L sqrt(f) enlarge^(1/d) with L the Cholesky factor of the sample covariance and f = max_i |L^-1 (p_i - c)|^2,
    i.e. the tightest scaled-covariance ellipsoid that holds every point, its volume enlarged by ``enlarge`` (default 1.25).
    ``bound="multi"``: a node with n >= 4d points is split by 2-means (Lloyd, at most 20 iterations, started at the two points
    extreme along the major principal axis: no random numbers); the split is kept iff both clusters hold >= 2d points and their
    ellipsoids' volumes add up to less than half the node's; then both halves are split further, breadth first, up to
    ``max_ellipsoids`` (32 at most).
  * Move.  Candidates c = 0, 1, 2, ... of the call, each from its own device draws: an ellipsoid e chosen by volume, a point uniform
    in it (u = c_e + rho A_e z / |z|, z ~ N(0, I), rho = v^(1/d)); rejected when outside the cube; kept with probability 1 / q when
    it lies in q ellipsoids (which makes the draw uniform over their union); logL evaluated for the rest.  The K replacements are
    the first K candidates with logL > L*, in candidate order.  ``ncall`` grows by the evaluations up to the last one taken.  No
    start points, no walk length, no scale rule; ``n_stuck`` stays 0.
  * The K new points are independent draws from the constrained prior as far as the ellipsoids cover {logL > L*} within the cube.
    An ellipsoid fitted to too few points cuts that region and log Z comes out high: keep nlive >= 50 d (the constructor warns below
    that; at nlive = 200 a separable 24-D Gaussian is high by 12 logzerr).  A search that does not find K points within
    max(1e5, 1e4 K) candidates ends the run with status "inefficient" and a warning.

The MLFriends region (``sample="mlfriends"``: UltraNest's bound, the reference's run_ultranest, alabi/core.py:3241-3690).  Everything as
for ``sample="unif"`` -- the same point set per iteration, the same ellipsoids, the "inefficient" status and candidate cap, the
nlive >= 50 d warning, use from the dynamic batches -- with one more test in the replacement step: a candidate counts only if it
lies within a radius r of some live point, in a metric whitened by the live points' covariance.  A union of ellipsoids cannot follow
a curved contour; a union of small balls around the live points can.
  * Bounds.  ``ells = bounding_ellipsoids(points, bound, enlarge, max_ellipsoids)``, unchanged.
  * Metric (UltraNest's cluster-wise whitening, the ellipsoid leaves as the clusters; ``mlfriends_metric``).  label_i = argmin_e
    |A_e^-1 (p_i - c_e)|^2; S = sum_i (p_i - c_label_i)(p_i - c_label_i)^T / (n - E); L = Cholesky(S) with the jitter ladder of the
    walk covariance; ``metric_inv`` = L^-1, lower triangular; w_i = L^-1 p_i, [n,d], computed once on the host and uploaded.
  * Radius.  B = ``num_bootstraps`` (30) rounds; round b draws n indices idx_k = min(floor(v_k n), n - 1) with v_k from the device's
    Philox stream (counter (call, b, 0x80000001, k)); selected = the set of drawn indices; r2_b = max over unselected i of min over
    selected j of |w_i - w_j|^2, 0 when nothing is left out; r^2 = max_b r2_b, taken on the host from the B values and listed in
    ``radius2``.  r^2 = 0 is legal and rejects everything but exact hits.
  * Candidate.  Exactly the ``unif`` candidate (the same keys, ellipsoid choice, cube test and 1 / q thinning); one that would be
    evaluated is evaluated iff some j has |metric_inv u - w_j|^2 <= r^2.  The K replacements are the first K evaluated candidates
    with logL > L*, as before.
  * Beyond 16384 points (dynamic batches over a long merged run) the balls are put around every ceil(n / 16384)-th point; the
    ellipsoids are still fitted to all of them.
  * Not carried over from UltraNest: the shrink-only region update, the wrapping-ellipsoid bootstrap
    (``enlarge`` plays that part), the from-points / bounding-box / transformed-box draw methods, the insertion-order test, the
    dlogz / dKL improvement criteria, wrapped and derived parameters, HDF5 / CSV logs and resume.

Not built (listed in DESIGN.md "Differences"): axis-aligned ``slice`` / ``hslice`` sampling, the bootstrap stop, other weight /
stop fractions than pfrac = 1; ``run_dynesty`` does not reach ``unif`` (``bound`` has no effect there).
"""
from __future__ import annotations

import ctypes as C
import math
import pickle
import warnings

import numpy as np
import torch

from . import _lib
from .gp import _dev

__all__ = ["NestedSampler", "NestedResults", "GPUWalkBackend", "PickleCheckpoint", "resample_equal", "compute_integrals",
           "merge_runs", "update_scale", "update_scale_slice", "default_slices", "Ellipsoids", "bounding_ellipsoids",
           "mlfriends_metric"]

MAXFRAC = 0.8
SCALE_MIN, SCALE_MAX = 1e-4, 10.0
SLICES_MULT = 3       # calibrated on a 24-D Gaussian (NOTES.md "Nested sampling")
MAX_ELLIPSOIDS = 32   # ALABI_NS_MAX_ELLIPSOIDS
MLF_MAX_POINTS = 16384  # ALABI_NS_MLF_MAX_POINTS
LIVE_PER_DIM = 50     # below this many live points per dimension an ellipsoid fitted to them can cut the likelihood contour


def update_scale(scale, acc, ndim):
    """The walk scale after an iteration with acceptance fraction ``acc`` (target 0.5)."""
    return float(min(max(scale * math.exp((acc - 0.5) / (0.5 * ndim)), SCALE_MIN), SCALE_MAX))


def update_scale_slice(scale, n_expand, n_contract):
    """The slice scale after an iteration with ``n_expand`` expansions and ``n_contract`` contractions over all its walks:
    as many expansions as two contractions leaves it unchanged, no expansion at all halves it."""
    n_expand, n_contract = int(n_expand), int(n_contract)
    new = 0.5 * scale if n_expand == 0 else scale * n_expand / (2.0 * max(n_contract, 1))
    return float(min(max(new, SCALE_MIN), SCALE_MAX))


def default_slices(ndim):
    """Slice updates per walk of ``sample="rslice"``: SLICES_MULT times dynesty's 3 + ndim."""
    return SLICES_MULT * (3 + int(ndim))


def compute_integrals(logl, samples_n):
    """(logvol, logwt, logz, logzerr, information) of dead points with ascending ``logl`` and live counts ``samples_n``."""
    logl = np.asarray(logl, dtype=np.float64)
    n = np.asarray(samples_n, dtype=np.float64)
    m = logl.shape[0]
    dlv = 1.0 / n
    logvol = -np.cumsum(dlv)
    logwt, logz, logzvar, h = np.empty(m), np.empty(m), np.empty(m), np.empty(m)
    lz, hh, var, lprev, vprev = -math.inf, 0.0, 0.0, -math.inf, 0.0
    for i in range(m):
        li, lv = float(logl[i]), float(logvol[i])
        ldv = vprev + math.log(-math.expm1(lv - vprev)) + math.log(0.5)       # log((X_{i-1} - X_i) / 2)
        lw = np.logaddexp(li, lprev) + ldv
        lz_new = np.logaddexp(lz, lw)
        term = math.exp(li - lz_new + ldv) * li
        if lprev > -math.inf:
            term += math.exp(lprev - lz_new + ldv) * lprev
        if lz > -math.inf:
            term += math.exp(lz - lz_new) * (hh + lz)
        h_new = term - lz_new
        var += (h_new - hh) * dlv[i]
        hh, lz, lprev, vprev = h_new, lz_new, li, lv
        logwt[i], logz[i], logzvar[i], h[i] = lw, lz, var, hh
    return logvol, logwt, logz, np.sqrt(np.maximum(logzvar, 0.0)), h


def resample_equal(samples, weights, rng=None):
    """Equal-weight resampling (systematic): as many draws as samples, sample i drawn weights_i / sum(weights) * n times in
    expectation, in random order (dynesty.utils.resample_equal)."""
    rng = np.random.default_rng() if rng is None else rng
    w = np.asarray(weights, dtype=np.float64)
    n = w.shape[0]
    cs = np.cumsum(w)
    cs /= cs[-1]
    pos = (rng.random() + np.arange(n)) / n
    idx = np.minimum(np.searchsorted(cs, pos, side="right"), n - 1)
    return np.asarray(samples)[rng.permutation(idx)]


class _Run:
    """Dead points of one static run, ascending logL, with the live count each was removed from."""

    def __init__(self, u, logl, n, logl_lo):
        self.u, self.logl, self.n, self.logl_lo = u, logl, n, float(logl_lo)


def merge_runs(runs):
    """(u, logl, samples_n) of the union of ``runs`` (objects with u, logl ascending, n, logl_lo)."""
    if not runs:
        raise ValueError("merge_runs: no runs")
    if len(runs) == 1:
        return runs[0].u, runs[0].logl, runs[0].n
    u = np.concatenate([r.u for r in runs])
    logl = np.concatenate([r.logl for r in runs])
    order = np.argsort(logl, kind="stable")
    u, logl = u[order], logl[order]
    n = np.zeros(logl.shape[0], dtype=np.int64)
    for r in runs:
        k = np.searchsorted(r.logl, logl, side="left")
        on = (logl > r.logl_lo) & (k < r.logl.shape[0])
        n[on] += r.n[k[on]]
    return u, logl, n


class NestedResults:
    """dynesty's Results fields: samples (theta), samples_u, logl, logwt, logvol, logz, logzerr, information, samples_n,
    niter (dead points of the loops, add_live excluded), ncall (likelihood evaluations), eff (100 niter / ncall), nlive,
    status ("converged", "maxiter", "maxcall", "plateau", "inefficient", "n_effective", "maxbatch"), n_stuck (walks without an accept;
    rslice: walks with a slice that hit the contraction cap)."""

    _FIELDS = ("samples", "samples_u", "logl", "logwt", "logvol", "logz", "logzerr", "information", "samples_n", "niter",
               "ncall", "eff", "nlive", "status", "n_stuck", "nbatch")

    def __init__(self, **kw):
        for k in self._FIELDS:
            setattr(self, k, kw.get(k))

    def __getitem__(self, k):
        return getattr(self, k)

    def keys(self):
        return list(self._FIELDS)

    def asdict(self):
        return {k: getattr(self, k) for k in self._FIELDS}

    def importance_weights(self):
        return np.exp(self.logwt - self.logz[-1])

    def samples_equal(self, rng=None):
        return resample_equal(self.samples, self.importance_weights(), rng)


def _chol(u):
    return _chol_cov(np.atleast_2d(np.cov(np.asarray(u).T)))


def _chol_cov(cov):
    """Lower Cholesky factor of ``cov`` [d,d] with a jitter ladder; the square roots of the diagonal when every rung fails."""
    d = cov.shape[0]
    jit = 1e-12 * max(float(np.trace(cov)) / d, 1e-300)
    for _ in range(8):
        try:
            return np.linalg.cholesky(cov + jit * np.eye(d))
        except np.linalg.LinAlgError:
            jit *= 100.0
    return np.diag(np.sqrt(np.maximum(np.diag(cov), 1e-30)))


class Ellipsoids:
    """E ellipsoids {c + A z : |z| <= 1}: ``centres`` [E,d], ``axes`` [E,d,d] (A, lower triangular), ``inv_axes`` [E,d,d] (A^-1,
    lower triangular), ``logvol`` [E] (log volume) and ``cum`` [E], the cumulative volume fractions with ``cum[-1] == 1.0``."""

    def __init__(self, centres, axes, inv_axes, logvol):
        self.centres = np.ascontiguousarray(centres, dtype=np.float64)
        self.axes = np.ascontiguousarray(axes, dtype=np.float64)
        self.inv_axes = np.ascontiguousarray(inv_axes, dtype=np.float64)
        self.logvol = np.ascontiguousarray(logvol, dtype=np.float64)
        w = np.exp(self.logvol - self.logvol.max())
        self.cum = np.cumsum(w) / np.sum(w)
        self.cum[-1] = 1.0

    def __len__(self):
        return int(self.centres.shape[0])


def _log_unit_ball(d):
    return 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d + 1.0)


def _one_ellipsoid(points, enlarge):
    """(c, A, A^-1, log volume): the covariance ellipsoid of ``points`` scaled to hold them all, its volume times ``enlarge``."""
    d = points.shape[1]
    c = points.mean(axis=0)
    L = _chol(points)
    y = np.linalg.solve(L, (points - c).T)
    f = max(float(np.max(np.sum(y * y, axis=0))), 1e-300)
    A = np.tril(L * (math.sqrt(f) * enlarge ** (1.0 / d)))
    Ainv = np.tril(np.linalg.inv(A))
    return c, A, Ainv, float(np.sum(np.log(np.diag(A)))) + _log_unit_ball(d)


def _two_means(points):
    """Boolean membership of cluster 1 after at most 20 Lloyd iterations from the two points extreme along the major principal
    axis (no random numbers), or None when a cluster empties."""
    c = points.mean(axis=0)
    cov = np.atleast_2d(np.cov(points.T))
    t = (points - c) @ np.linalg.eigh(cov)[1][:, -1]
    m0, m1 = points[int(np.argmin(t))], points[int(np.argmax(t))]
    lab = None
    for _ in range(20):
        new = np.sum((points - m1) ** 2, axis=1) < np.sum((points - m0) ** 2, axis=1)
        if new.all() or not new.any():
            return None
        if lab is not None and np.array_equal(new, lab):
            break
        lab = new
        m0, m1 = points[~lab].mean(axis=0), points[lab].mean(axis=0)
    return lab


def bounding_ellipsoids(points, bound="multi", enlarge=1.25, max_ellipsoids=MAX_ELLIPSOIDS):
    """Ellipsoids around ``points`` [n,d] (MultiNest's bounds).  One ellipsoid: centre = the mean, shape = the sample covariance
    scaled so that the tightest such ellipsoid holds every point, volume then enlarged by ``enlarge``.  ``bound="multi"``: a node
    with n >= 4d points (and budget left) is split by 2-means; the split is kept iff both clusters hold >= 2d points and their
    ellipsoids' volumes add up to less than half the node's, and then both halves are split further, breadth first, until
    ``max_ellipsoids`` exist.  ``bound="single"``: one ellipsoid."""
    if bound not in ("single", "multi"):
        raise ValueError("bound must be 'single' or 'multi'")
    p = np.ascontiguousarray(points, dtype=np.float64)
    if p.ndim != 2 or p.shape[0] < 2:
        raise ValueError("bounding_ellipsoids needs points [n,d] with n >= 2")
    d = p.shape[1]
    budget = 1 if bound == "single" else max(1, min(int(max_ellipsoids), MAX_ELLIPSOIDS))
    queue, done = [(p, _one_ellipsoid(p, enlarge))], []
    while queue:
        pts, ell = queue.pop(0)
        if len(queue) + len(done) + 1 < budget and pts.shape[0] >= 4 * d:
            lab = _two_means(pts)
            if lab is not None and min(int(lab.sum()), int((~lab).sum())) >= 2 * d:
                a, b = _one_ellipsoid(pts[~lab], enlarge), _one_ellipsoid(pts[lab], enlarge)
                if np.logaddexp(a[3], b[3]) < ell[3] + math.log(0.5):
                    queue += [(pts[~lab], a), (pts[lab], b)]
                    continue
        done.append(ell)
    return Ellipsoids(*(np.stack([e[k] for e in done]) for k in range(3)), np.array([e[3] for e in done]))


def mlfriends_metric(points, ells):
    """The whitening of the MLFriends region: (labels [n], metric_inv [d,d], w [n,d]).  ``labels[i]`` is the ellipsoid of ``ells``
    whose centre is nearest to point i in that ellipsoid's own metric; S the covariance of the points about their own ellipsoid's
    centre, pooled over the ellipsoids (n - E degrees of freedom), so that separated clusters do not inflate it; ``metric_inv`` =
    L^-1 with S = L L^T, lower triangular; ``w`` = the whitened points L^-1 p_i."""
    p = np.ascontiguousarray(points, dtype=np.float64)
    n, d = p.shape
    E = len(ells)
    m = np.empty((E, n))
    for e in range(E):
        y = np.einsum("ki,ni->nk", ells.inv_axes[e], p - ells.centres[e])
        m[e] = np.sum(y * y, axis=1)
    labels = np.argmin(m, axis=0)
    r = p - ells.centres[labels]
    L = _chol_cov((r.T @ r) / max(n - E, 1))
    metric_inv = np.ascontiguousarray(np.tril(np.linalg.inv(L)))
    return labels, metric_inv, np.ascontiguousarray(p @ metric_inv.T)


class NestedSampler:
    """Static (``dynamic=False``) or dynamic nested sampler over a walk backend.

    backend: ``ndim``, ``prior(call, n) -> (u, logl)``, ``walk(call, u0, logl0, logl_star, chol, scale, walks) ->
    (u, logl, n_accept, n_eval)``, ``theta(u) -> samples``, and for ``sample="rslice"`` ``rslice(call, u0, logl0, logl_star,
    chol, scale, slices) -> (u, logl, n_eval, n_expand, n_contract, n_capped)``.  ``sample``: "rwalk" (``walks`` Metropolis
    steps) or "rslice" (``slices`` slice updates, default ``default_slices(ndim)``).  ``seed`` seeds the host generator
    (start-point choice and
    resampling); the device draws are keyed by the backend's own seed and the call counter kept here.
    ``sample="unif"``: the replacements are uniform draws inside ellipsoids around the surviving live points
    (``bounding_ellipsoids`` with ``bound`` "multi" / "single" and ``enlarge``; at most ``max_ellipsoids``) from
    ``unif(call, ells, logl_star, K) -> (u [K,d], logl [K], n_eval, n_cand)``; no walk length, no scale.  ``n_ellipsoids`` lists
    the number of ellipsoids of every such call.  A backend that returns fewer than K points ends the run with status
    "inefficient".
    ``sample="mlfriends"``: the same with the MLFriends region on top (module docstring): per call ``mlf_radius(call, w, B) -> r2``
    with B = ``num_bootstraps`` and ``mlfriends(call, ells, w, metric_inv, r2, logl_star, K)`` returning what ``unif`` returns;
    ``radius2`` lists the r^2 of every such call beside ``n_ellipsoids``."""

    def __init__(self, backend, nlive, dynamic=False, walks=25, batch=None, seed=0, sample="rwalk", slices=None, bound="multi",
                 enlarge=1.25, max_ellipsoids=MAX_ELLIPSOIDS, num_bootstraps=30):
        self.backend = backend
        self.ndim = int(backend.ndim)
        self.nlive = int(nlive)
        if self.nlive < 2:
            raise ValueError("nlive must be >= 2")
        self.dynamic = bool(dynamic)
        self.walks = int(walks)
        if sample not in ("rwalk", "rslice", "unif", "mlfriends"):
            raise ValueError("sample must be 'rwalk', 'rslice', 'unif' or 'mlfriends'")
        self.sample = sample
        self.slices = default_slices(self.ndim) if slices is None else int(slices)
        if self.slices < 0:
            raise ValueError("slices must be >= 0")
        self.batch = int(math.ceil(self.nlive / 4)) if batch is None else int(batch)
        if not 1 <= self.batch < self.nlive:
            raise ValueError("batch must lie in [1, nlive)")
        if bound not in ("single", "multi"):
            raise ValueError("bound must be 'single' or 'multi'")
        self.bound, self.enlarge, self.max_ellipsoids = bound, float(enlarge), int(max_ellipsoids)
        if not self.enlarge >= 1.0 or self.max_ellipsoids < 1:
            raise ValueError("enlarge must be >= 1 and max_ellipsoids >= 1")
        self.num_bootstraps = int(num_bootstraps)
        if self.num_bootstraps < 1:
            raise ValueError("num_bootstraps must be >= 1")
        self.n_ellipsoids, self.radius2 = [], []
        self._bounded = sample in ("unif", "mlfriends")       # replacements drawn inside bounds around the live points
        if self._bounded:
            if self.nlive - self.batch < self.ndim + 2:
                raise ValueError(f"sample='{sample}': {self.nlive - self.batch} surviving live points per iteration (nlive - batch) "
                                 f"cannot bound an ellipsoid in {self.ndim} dimensions; at least ndim + 2 are needed")
            if self.nlive < LIVE_PER_DIM * self.ndim:
                warnings.warn("ellipsoid bounds from fewer than 50 live points per dimension can cut the likelihood contour and "
                              "bias log Z high", UserWarning, stacklevel=2)
        self.rng = np.random.default_rng(seed)
        self.call = 0
        self.scale = 1.0
        self.ncall = 0
        self.n_stuck = 0
        self.niter = 0
        self.runs = []
        self._current = None      # the static loop in progress (dead points + its live set as add_live), for snapshots
        self.results = None

    def __getstate__(self):
        st = self.__dict__.copy()
        st["backend"] = None        # device handles are not part of the saved state
        return st

    # ------------------------------------------------------------------ one static loop
    def _walk(self, u0, l0, lstar, chol):
        if self.sample == "rslice":
            u, logl, nev, nexp, ncon, ncap = self.backend.rslice(self.call, u0, l0, lstar, chol, self.scale, self.slices)
            self.call += 1
            self.ncall += int(np.sum(nev))
            self.n_stuck += int(np.count_nonzero(ncap))
            self.scale = update_scale_slice(self.scale, np.sum(nexp), np.sum(ncon))
            return np.asarray(u), np.asarray(logl)
        u, logl, nacc, nev = self.backend.walk(self.call, u0, l0, lstar, chol, self.scale, self.walks)
        self.call += 1
        self.ncall += int(np.sum(nev))
        self.n_stuck += int(np.sum(nacc == 0))
        self.scale = update_scale(self.scale, float(np.sum(nacc)) / (len(u0) * max(self.walks, 1)), self.ndim)
        return np.asarray(u), np.asarray(logl)

    def _unif(self, points, lstar, K):
        """K points with logL > ``lstar`` drawn uniformly inside ellipsoids around ``points`` (fewer: the backend gave up)."""
        if points.shape[0] < self.ndim + 2:
            raise ValueError(f"sample='{self.sample}': {points.shape[0]} points cannot bound an ellipsoid in {self.ndim} dimensions")
        ells = bounding_ellipsoids(points, self.bound, self.enlarge, self.max_ellipsoids)
        self.n_ellipsoids.append(len(ells))
        if self.sample == "mlfriends":
            friends = points[::-(-points.shape[0] // MLF_MAX_POINTS)]      # every point up to the device's limit
            _, metric_inv, w = mlfriends_metric(friends, ells)
            r2 = float(self.backend.mlf_radius(self.call, w, self.num_bootstraps))
            self.radius2.append(r2)
            u, logl, nev, _ = self.backend.mlfriends(self.call, ells, w, metric_inv, r2, lstar, K)
        else:
            u, logl, nev, _ = self.backend.unif(self.call, ells, lstar, K)
        self.call += 1
        self.ncall += int(nev)
        return np.asarray(u, dtype=np.float64).reshape(-1, self.ndim), np.asarray(logl, dtype=np.float64).reshape(-1)

    def _inefficient(self, got, K):
        warnings.warn(f"nested sampling: the ellipsoid draws found {got} of {K} points above L* before the candidate cap; the run "
                      "stops here")

    def _static(self, live_u, live_l, logl_lo, logl_hi, dlogz, maxiter, maxcall, checkpoint=None):
        live_u, live_l = np.array(live_u, dtype=np.float64), np.array(live_l, dtype=np.float64)
        n = live_l.shape[0]
        K = min(self.batch, n - 1)
        du, dl, dn = [], [], []
        lz, lprev, vprev = -math.inf, -math.inf, 0.0
        status = "converged"
        lstar = logl_lo
        while True:
            if lstar >= logl_hi:
                break
            if np.logaddexp(0.0, float(np.max(live_l)) + vprev - lz) < dlogz:
                break
            if self.niter >= maxiter:
                status = "maxiter"
                break
            if self.ncall >= maxcall:
                status = "maxcall"
                break
            order = np.argsort(live_l, kind="stable")
            rem, surv = order[:K], order[K:]
            lstar = float(live_l[rem[-1]])
            for j, i in enumerate(rem):
                du.append(live_u[i].copy()); dl.append(live_l[i]); dn.append(n - j)
                v = vprev - 1.0 / (n - j)
                lw = np.logaddexp(live_l[i], lprev) + vprev + math.log(-math.expm1(v - vprev)) + math.log(0.5)
                lz, lprev, vprev = np.logaddexp(lz, lw), float(live_l[i]), v
            self.niter += K
            cand = surv[live_l[surv] > lstar]
            if cand.shape[0] == 0:
                warnings.warn("nested sampling: no live point above L* (likelihood plateau); the run stops here")
                status = "plateau"
                live_u, live_l = live_u[surv], live_l[surv]
                break
            if self._bounded:
                nu, nl = self._unif(live_u[surv], lstar, K)
                if nl.shape[0] < K:
                    self._inefficient(nl.shape[0], K)
                    status = "inefficient"
                    live_u, live_l = live_u[surv], live_l[surv]
                    break
            else:
                chol = _chol(live_u[surv])
                starts = cand[self.rng.integers(0, cand.shape[0], size=K)]
                nu, nl = self._walk(live_u[starts], live_l[starts], lstar, chol)
            live_u[rem], live_l[rem] = nu, nl
            if checkpoint is not None:
                self._current = self._with_live(du, dl, dn, live_u, live_l, logl_lo)
                checkpoint(self.niter)
                self._current = None
        return self._with_live(du, dl, dn, live_u, live_l, logl_lo), status

    def _with_live(self, du, dl, dn, live_u, live_l, logl_lo):
        """The run of dead points (du, dl, dn) with the live set appended as add_live does."""
        order = np.argsort(live_l, kind="stable")
        m = order.shape[0]
        u = np.concatenate([np.array(du).reshape(-1, self.ndim), live_u[order]])
        logl = np.concatenate([np.array(dl, dtype=np.float64), live_l[order]])
        n = np.concatenate([np.array(dn, dtype=np.int64), m - np.arange(m)])
        return _Run(u, logl, n, logl_lo)

    # --------------------------------------------------------------------------- driver
    def run_nested(self, dlogz=0.5, maxiter=None, maxcall=None, dlogz_init=0.5, nlive_init=None, nlive_batch=None,
                   maxbatch=10, n_effective=10000, wt_kwargs=None, stop_kwargs=None, checkpoint=None):
        for name, kw in (("wt_kwargs", wt_kwargs), ("stop_kwargs", stop_kwargs)):
            if kw is not None and (set(kw) - {"pfrac"} or float(kw.get("pfrac", 1.0)) != 1.0):
                raise NotImplementedError(f"{name}={kw!r}: only pfrac=1.0 (all weight on the posterior) is built; evidence-"
                                          "weighted batches (pfrac < 1) and other weight / stop options are not")
        maxiter = math.inf if maxiter is None else int(maxiter)
        maxcall = math.inf if maxcall is None else int(maxcall)
        n0 = self.nlive if (nlive_init is None or not self.dynamic) else int(nlive_init)
        u, logl = self.backend.prior(self.call, n0)
        self.call += 1
        self.ncall += n0
        base, status = self._static(u, logl, -math.inf, math.inf, dlogz_init if self.dynamic else dlogz, maxiter, maxcall,
                                    checkpoint)
        self.runs = [base]
        nbatch = 0
        if self.dynamic and status == "converged":
            nb = self.nlive if nlive_batch is None else int(nlive_batch)
            status = "maxbatch"
            while True:
                mu, ml, mn = merge_runs(self.runs)
                _, logwt, logz, _, _ = compute_integrals(ml, mn)
                w = np.exp(logwt - logz[-1])
                if w.sum() ** 2 / np.sum(w ** 2) >= n_effective:
                    status = "n_effective"
                    break
                if nbatch >= maxbatch:
                    break
                if self.niter >= maxiter or self.ncall >= maxcall:
                    status = "maxiter" if self.niter >= maxiter else "maxcall"
                    break
                idx = np.flatnonzero(w >= MAXFRAC * w.max())
                lo_i, hi_i = int(idx.min()) - 1, int(idx.max()) + 1
                l_lo = float(ml[lo_i]) if lo_i >= 0 else -math.inf
                l_hi = float(ml[hi_i]) if hi_i < ml.shape[0] else float(ml[-1])
                if l_lo == -math.inf:
                    bu, bl = self.backend.prior(self.call, nb)
                    self.call += 1
                    self.ncall += nb
                else:
                    cand = np.flatnonzero(ml > l_lo)
                    if self._bounded:
                        bu, bl = self._unif(mu[cand], l_lo, nb)
                        if bl.shape[0] < nb:
                            self._inefficient(bl.shape[0], nb)
                            status = "inefficient"
                            break
                    else:
                        chol = _chol(mu[cand])
                        starts = cand[self.rng.integers(0, cand.shape[0], size=nb)]
                        bu, bl = self._walk(mu[starts], ml[starts], l_lo, chol)
                run, st = self._static(bu, bl, l_lo, l_hi, dlogz, maxiter, maxcall, checkpoint)
                self.runs.append(run)
                nbatch += 1
                if st in ("plateau", "inefficient"):
                    status = st
                    break
        self.results = self._results(status, nbatch)
        return self.results

    def snapshot(self):
        """Results so far (status "running"): every finished run plus, inside a checkpoint callback, the run in progress with
        its current live points added as add_live would add them."""
        return self._results("running", max(len(self.runs) - 1, 0))

    def _results(self, status, nbatch=0):
        runs = self.runs + ([self._current] if self._current is not None else [])
        u, logl, n = merge_runs(runs)
        logvol, logwt, logz, logzerr, h = compute_integrals(logl, n)
        return NestedResults(samples=np.asarray(self.backend.theta(u)), samples_u=u, logl=logl, logwt=logwt, logvol=logvol,
                             logz=logz, logzerr=logzerr, information=h, samples_n=n, niter=self.niter, ncall=self.ncall,
                             eff=100.0 * self.niter / max(self.ncall, 1), nlive=self.nlive, status=status,
                             n_stuck=self.n_stuck, nbatch=nbatch)


class PickleCheckpoint:
    """run_dynesty's ``save_iter``: a ``run_nested(checkpoint=...)`` callable that pickles ``sampler.snapshot().asdict()``
    (plain NumPy) to ``path`` whenever ``every`` more dead points have been removed; ``write(results)`` stores the final ones."""

    def __init__(self, sampler, path, every):
        self.sampler, self.path, self.every, self.last = sampler, path, int(every), 0

    def __call__(self, niter):
        if niter - self.last >= self.every:
            self.last = niter
            self.write(self.sampler.snapshot())

    def write(self, results):
        with open(self.path, "wb") as fh:
            pickle.dump(results.asdict(), fh)


class GPUWalkBackend:
    """The walks on the device (alabi_ns_* in include/alabi_hip.h).

    Fused (``host_loglike=None``): logL(u) = map(scale * GP mean(lo + u (hi - lo)) + shift) inside ``ns_walk_kernel``;
    ``bounds`` [d,2] in the GP's scaled coordinates, ``logp_affine=(scale, shift)``, ``logp_map`` None / "nlog" / "log".
    ``normal_prior=(mean[d], std[d])`` in the same coordinates (NaN mean: uniform over the box; std may be negative) replaces the
    uniform map by mean + std * ndtri(u) on its coordinates, un-truncated (the reference's prior_transform_normal);
    ``transform(u)`` returns the scaled coordinates the kernels evaluate the GP at.
    Split: ``host_loglike(u [m,d]) -> [m]`` is called between alabi_ns_propose and alabi_ns_accept for the in-cube proposals
    of every step.  ``to_theta(u [m,d]) -> [m,d]`` maps cube points to the samples reported.
    ``rslice`` is the slice move on the same two paths: ``ns_slice_kernel``, or alabi_ns_slice_step around ``host_loglike``;
    ``unif`` the uniform draws inside ellipsoids: ``ns_unif_draw_kernel`` + ``ns_unif_select_kernel``, with ``host_loglike``
    between the two; ``mlf_radius`` / ``mlfriends`` the MLFriends region over them: ``ns_mlf_radius_kernel``, and
    ``ns_mlf_draw_kernel`` in the place of ``ns_unif_draw_kernel``."""

    def __init__(self, gp, y, bounds, seed, to_theta, logp_affine=(1.0, 0.0), logp_map=None, host_loglike=None,
                 normal_prior=None):
        self.gp, self._y = gp, y
        self.ndim = int(gp.ndim)
        self.bounds = np.ascontiguousarray(np.asarray(bounds, dtype=np.float64).reshape(self.ndim, 2))
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.to_theta = to_theta
        self.logp_affine = (float(logp_affine[0]), float(logp_affine[1]))
        if logp_map not in (None, "nlog", "log"):
            raise ValueError("logp_map must be None, 'nlog' or 'log'")
        self.logp_map = logp_map
        self.host_loglike = host_loglike
        self.normal_prior = None
        if normal_prior is not None:
            self.normal_prior = tuple(np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(self.ndim))
                                      for v in normal_prior)
        self.host_calls = 0
        self.evals_launched = 0          # unif: every evaluation the device (or the host) made, discarded chunk tails included
        self._unif_eff = 0.25            # accept fraction of the previous unif call
        self._ns = None

    @property
    def path(self):
        """'fused' or 'host-callback'."""
        return "fused" if self.host_loglike is None else "host-callback"

    def _ensure(self):
        if self._ns is not None:
            return self._ns
        h = self.gp.sampler_handle(self._y, surrogate_on_device=self.host_loglike is None)
        ns = C.c_void_p()
        _lib.check(_lib.lib().alabi_ns_create(h, self.ndim, _lib.host_doubles(self.bounds.ravel()), C.c_ulonglong(self.seed),
                                              C.byref(ns)), "alabi_ns_create")
        kind = {None: 0, "nlog": 1, "log": 2}[self.logp_map]
        _lib.check(_lib.lib().alabi_ns_set_logp(ns, self.logp_affine[0], self.logp_affine[1], kind), "alabi_ns_set_logp")
        if self.normal_prior is not None:
            st = _lib.lib().alabi_ns_set_normal_prior(ns, _lib.host_doubles(self.normal_prior[0]),
                                                      _lib.host_doubles(self.normal_prior[1]))
            if st != _lib.OK:
                _lib.destroy(ns, "alabi_ns_destroy")
                _lib.check(st, "alabi_ns_set_normal_prior")
        self._ns = ns
        return ns

    def last_path(self):
        p = C.c_int(0)
        _lib.check(_lib.lib().alabi_ns_last_path(self._ensure(), C.byref(p)), "alabi_ns_last_path")
        return int(p.value)

    def close(self):
        _lib.destroy(getattr(self, "_ns", None), "alabi_ns_destroy", sync=True)
        self._ns = None

    def __del__(self):
        self.close()

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_ns"] = None
        st["host_loglike"] = None
        return st

    def theta(self, u):
        return np.asarray(self.to_theta(np.asarray(u)), dtype=np.float64).reshape(-1, self.ndim)

    def transform(self, u):
        """Scaled coordinates [n,d] (before the length scales) of the cube points ``u`` [n,d], by the kernels' own map."""
        ns, dev = self._ensure(), _dev()
        ud = torch.as_tensor(np.ascontiguousarray(np.asarray(u, dtype=np.float64).reshape(-1, self.ndim)), device=dev)
        x = torch.empty_like(ud)
        _lib.check(_lib.lib().alabi_ns_transform(ns, _lib.ptr(ud), int(ud.shape[0]), _lib.ptr(x), _lib.current_stream()),
                   "alabi_ns_transform")
        return x.cpu().numpy()

    def _host(self, up):
        inside = np.all((up > 0.0) & (up < 1.0), axis=1)
        lp = np.full(up.shape[0], -np.inf)
        if inside.any():
            lp[inside] = np.asarray(self.host_loglike(up[inside]), dtype=np.float64).reshape(-1)
            self.host_calls += int(inside.sum())
        return lp

    def prior(self, call, n):
        ns, lib, dev = self._ensure(), _lib.lib(), _dev()
        u = torch.empty((n, self.ndim), dtype=torch.float64, device=dev)
        logl = torch.empty(n, dtype=torch.float64, device=dev) if self.host_loglike is None else None
        _lib.check(lib.alabi_ns_prior_draw(ns, int(call), 0, int(n), _lib.ptr(u), _lib.ptr(logl), _lib.current_stream()),
                   "alabi_ns_prior_draw")
        uh = u.cpu().numpy()
        if logl is None:
            lh = np.full(n, -np.inf)
            lh[:] = np.asarray(self.host_loglike(uh), dtype=np.float64).reshape(-1)
            self.host_calls += int(n)
        else:
            lh = logl.cpu().numpy()
        return uh, lh

    def _upload(self, u0, logl0, chol):
        """Device copies (u, logl, chol, K) of K start points; the walk and the slice kernels update u and logl in place."""
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=_dev())  # noqa: E731
        return up(u0).clone(), up(logl0).clone(), up(chol), int(np.asarray(u0).shape[0])

    def walk(self, call, u0, logl0, logl_star, chol, scale, walks, walk_id0=0):
        ns, lib, dev, stream = self._ensure(), _lib.lib(), _dev(), _lib.current_stream()
        u, logl, ch, K = self._upload(u0, logl0, chol)
        nacc = torch.zeros(2 * K, dtype=torch.int32, device=dev)
        if self.host_loglike is None:
            _lib.check(lib.alabi_ns_walk(ns, int(call), int(walk_id0), _lib.ptr(u), _lib.ptr(logl), K, float(logl_star),
                                         _lib.ptr(ch), float(scale), int(walks), _lib.ptr(u), _lib.ptr(logl), _lib.ptr(nacc),
                                         stream), "alabi_ns_walk")
        else:
            up = torch.empty_like(u)
            for s in range(int(walks)):
                _lib.check(lib.alabi_ns_propose(ns, int(call), int(walk_id0), _lib.ptr(u), K, s, _lib.ptr(ch), float(scale),
                                                _lib.ptr(up), stream), "alabi_ns_propose")
                lp = torch.as_tensor(self._host(up.cpu().numpy()), device=dev)
                _lib.check(lib.alabi_ns_accept(ns, K, _lib.ptr(up), _lib.ptr(lp), float(logl_star), _lib.ptr(u), _lib.ptr(logl),
                                               _lib.ptr(nacc), stream), "alabi_ns_accept")
        n = nacc.cpu().numpy()
        return u.cpu().numpy(), logl.cpu().numpy(), n[:K], n[K:]

    def rslice(self, call, u0, logl0, logl_star, chol, scale, slices, walk_id0=0):
        """``slices`` random-direction slice updates of every walk: (u, logl, n_eval, n_expand, n_contract, n_capped), the
        last four per walk (in-cube likelihood evaluations, expansions, contractions, slices that hit the contraction cap)."""
        ns, lib, dev, stream = self._ensure(), _lib.lib(), _dev(), _lib.current_stream()
        u, logl, ch, K = self._upload(u0, logl0, chol)
        counts = torch.zeros(4 * K, dtype=torch.int32, device=dev)
        if self.host_loglike is None:
            _lib.check(lib.alabi_ns_slice(ns, int(call), int(walk_id0), _lib.ptr(u), _lib.ptr(logl), K, float(logl_star),
                                          _lib.ptr(ch), float(scale), int(slices), _lib.ptr(u), _lib.ptr(logl), _lib.ptr(counts),
                                          stream), "alabi_ns_slice")
        elif K > 0 and int(slices) > 0:
            nbytes = C.c_longlong(0)
            _lib.check(lib.alabi_ns_slice_state_bytes(ns, K, C.byref(nbytes)), "alabi_ns_slice_state_bytes")
            state = torch.empty((int(nbytes.value) + 7) // 8, dtype=torch.float64, device=dev)
            _lib.check(lib.alabi_ns_slice_begin(ns, _lib.ptr(u), _lib.ptr(logl), K, _lib.ptr(state), stream),
                       "alabi_ns_slice_begin")
            uq = torch.empty_like(u)
            active = torch.zeros(K, dtype=torch.int32, device=dev)
            lq = torch.zeros(K, dtype=torch.float64, device=dev)
            while True:
                _lib.check(lib.alabi_ns_slice_step(ns, int(call), int(walk_id0), K, float(logl_star), _lib.ptr(ch), float(scale),
                                                   int(slices), _lib.ptr(state), _lib.ptr(lq), _lib.ptr(uq), _lib.ptr(active),
                                                   stream),
                           "alabi_ns_slice_step")
                on = active.cpu().numpy() != 0
                if not on.any():
                    break
                lh = np.zeros(K)
                lh[on] = np.asarray(self.host_loglike(uq.cpu().numpy()[on]), dtype=np.float64).reshape(-1)
                self.host_calls += int(on.sum())
                lq = torch.as_tensor(lh, device=dev)
            _lib.check(lib.alabi_ns_slice_end(ns, K, _lib.ptr(state), _lib.ptr(u), _lib.ptr(logl), _lib.ptr(counts), stream),
                       "alabi_ns_slice_end")
        n = counts.cpu().numpy()
        return u.cpu().numpy(), logl.cpu().numpy(), n[:K], n[K:2 * K], n[2 * K:3 * K], n[3 * K:]

    def unif(self, call, ells, logl_star, K, cand_id0=0, chunk=None):
        """K points with logL > ``logl_star`` uniform in the union of the ellipsoids ``ells`` (``Ellipsoids``) inside the cube:
        (u [k,d], logl [k], n_eval, n_cand) with k = K unless the search gave up after max(1e5, 1e4 K) candidates.  Candidates
        ``cand_id0``, ``cand_id0`` + 1, ... are drawn and tested in chunks (``ns_unif_draw_kernel``) and taken in candidate order
        (``ns_unif_select_kernel``), so the result does not depend on ``chunk``; the default is ceil(1.25 need / eff) rounded up to
        64 within [256, 65536], eff being the accept fraction of the previous call (0.25 at first).  ``n_eval`` / ``n_cand``:
        likelihood evaluations / candidates up to the last one taken; ``evals_launched`` also counts the discarded tail.  With
        ``host_loglike`` the device stops after the thinning test and the host evaluates the chunk's surviving candidates."""
        lib, dev, E = _lib.lib(), _dev(), len(ells)
        tab = [torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
               for a in (ells.centres, ells.axes, ells.inv_axes, ells.cum)]

        def draw(ns, cid, M, evaluate, cu, cl, cs, stream):
            _lib.check(lib.alabi_ns_unif_draw(ns, int(call), cid, M, evaluate, E, _lib.ptr(tab[0]), _lib.ptr(tab[1]), _lib.ptr(tab[2]),
                                              _lib.ptr(tab[3]), _lib.ptr(cu), _lib.ptr(cl), _lib.ptr(cs), stream),
                       "alabi_ns_unif_draw")
        return self._draw_select(draw, logl_star, K, cand_id0, chunk)

    def mlf_radius(self, call, w, B):
        """r^2 of the MLFriends region around the whitened points ``w`` [n,d]: the largest, over ``B`` bootstrap rounds, of the
        squared distance from a point left out of the round to the nearest point drawn (``ns_mlf_radius_kernel``; the maximum of the
        B values is taken here)."""
        ns, dev = self._ensure(), _dev()
        wd = torch.as_tensor(np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1, self.ndim)), device=dev)
        r2 = torch.empty(max(int(B), 1), dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().alabi_ns_mlf_radius(ns, int(call), int(wd.shape[0]), _lib.ptr(wd), int(B), _lib.ptr(r2),
                                                  _lib.current_stream()), "alabi_ns_mlf_radius")
        return float(r2.max().item())

    def mlfriends(self, call, ells, w, metric_inv, r2, logl_star, K, cand_id0=0, chunk=None):
        """``unif`` with the MLFriends test: a candidate is evaluated only if some row of ``w`` [n,d] lies within ``r2`` (squared)
        of ``metric_inv`` u (``ns_mlf_draw_kernel``).  The same loop, chunk rule, counters and host-likelihood split."""
        lib, dev, E = _lib.lib(), _dev(), len(ells)
        tab = [torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
               for a in (ells.centres, ells.axes, ells.inv_axes, ells.cum, np.asarray(w).reshape(-1, self.ndim), metric_inv)]
        n = int(tab[4].shape[0])

        def draw(ns, cid, M, evaluate, cu, cl, cs, stream):
            _lib.check(lib.alabi_ns_mlf_draw(ns, int(call), cid, M, evaluate, E, _lib.ptr(tab[0]), _lib.ptr(tab[1]), _lib.ptr(tab[2]),
                                             _lib.ptr(tab[3]), n, _lib.ptr(tab[4]), _lib.ptr(tab[5]), float(r2), _lib.ptr(cu),
                                             _lib.ptr(cl), _lib.ptr(cs), stream), "alabi_ns_mlf_draw")
        return self._draw_select(draw, logl_star, K, cand_id0, chunk)

    def _draw_select(self, draw, logl_star, K, cand_id0, chunk):
        """The chunk loop of ``unif`` and ``mlfriends``: ``draw(ns, cid, M, evaluate, cand_u, cand_logl, cand_status, stream)``
        launches the candidates cid .. cid + M - 1; the host likelihood fills in between; ``ns_unif_select_kernel`` takes."""
        ns, lib, dev, stream = self._ensure(), _lib.lib(), _dev(), _lib.current_stream()
        K, d = int(K), self.ndim
        u_out = torch.empty((max(K, 1), d), dtype=torch.float64, device=dev)
        l_out = torch.empty(max(K, 1), dtype=torch.float64, device=dev)
        counts = torch.zeros(5, dtype=torch.int32, device=dev)
        cap = max(100000, 10000 * K)
        taken = n_eval = n_cand = launched = 0
        cid = int(cand_id0)
        while taken < K and launched < cap:
            need = K - taken
            if chunk is None:
                M = min(max(64 * int(math.ceil(1.25 * need / max(self._unif_eff, 1e-6) / 64.0)), 256), 65536)
            else:
                M = int(chunk)
            cu = torch.empty((M, d), dtype=torch.float64, device=dev)
            cl = torch.empty(M, dtype=torch.float64, device=dev)
            cs = torch.empty(M, dtype=torch.int32, device=dev)
            draw(ns, cid, M, 0 if self.host_loglike is not None else 1, cu, cl, cs, stream)
            status = cs.cpu().numpy()
            ev = status == 2
            if self.host_loglike is not None and ev.any():
                lh = np.full(M, -np.inf)
                lh[ev] = self._host(cu.cpu().numpy()[ev])
                cl = torch.as_tensor(lh, device=dev)
            self.evals_launched += int(ev.sum())
            _lib.check(lib.alabi_ns_unif_select(ns, M, _lib.ptr(cu), _lib.ptr(cl), _lib.ptr(cs), float(logl_star), need,
                                                C.c_void_p(u_out.data_ptr() + 8 * d * taken), C.c_void_p(l_out.data_ptr() + 8 * taken),
                                                _lib.ptr(counts), stream), "alabi_ns_unif_select")
            c = counts.cpu().numpy()
            taken += int(c[0]); n_cand += int(c[1]); n_eval += int(c[2])
            cid += M
            launched += M
        self._unif_eff = max(taken, 1) / max(n_cand, 1)
        return u_out[:taken].cpu().numpy(), l_out[:taken].cpu().numpy(), n_eval, n_cand
