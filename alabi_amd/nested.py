"""Nested sampling on the GPU: the static and dynamic samplers behind ``SurrogateModel.run_dynesty``.

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

Not built (listed in DESIGN.md "Differences"): bounding ellipsoids (``bound`` has no effect), ``unif`` / axis-aligned ``slice``
/ ``hslice`` sampling, the bootstrap stop, other weight / stop fractions than pfrac = 1.
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
           "merge_runs", "update_scale", "update_scale_slice", "default_slices"]

MAXFRAC = 0.8
SCALE_MIN, SCALE_MAX = 1e-4, 10.0
SLICES_MULT = 3       # calibrated on a 24-D Gaussian (NOTES.md "Nested sampling")


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
    status ("converged", "maxiter", "maxcall", "plateau", "n_effective", "maxbatch"), n_stuck (walks without an accept;
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
    cov = np.atleast_2d(np.cov(np.asarray(u).T))
    d = cov.shape[0]
    jit = 1e-12 * max(float(np.trace(cov)) / d, 1e-300)
    for _ in range(8):
        try:
            return np.linalg.cholesky(cov + jit * np.eye(d))
        except np.linalg.LinAlgError:
            jit *= 100.0
    return np.diag(np.sqrt(np.maximum(np.diag(cov), 1e-30)))


class NestedSampler:
    """Static (``dynamic=False``) or dynamic nested sampler over a walk backend.

    backend: ``ndim``, ``prior(call, n) -> (u, logl)``, ``walk(call, u0, logl0, logl_star, chol, scale, walks) ->
    (u, logl, n_accept, n_eval)``, ``theta(u) -> samples``, and for ``sample="rslice"`` ``rslice(call, u0, logl0, logl_star,
    chol, scale, slices) -> (u, logl, n_eval, n_expand, n_contract, n_capped)``.  ``sample``: "rwalk" (``walks`` Metropolis
    steps) or "rslice" (``slices`` slice updates, default ``default_slices(ndim)``).  ``seed`` seeds the host generator
    (start-point choice and
    resampling); the device draws are keyed by the backend's own seed and the call counter kept here."""

    def __init__(self, backend, nlive, dynamic=False, walks=25, batch=None, seed=0, sample="rwalk", slices=None):
        self.backend = backend
        self.ndim = int(backend.ndim)
        self.nlive = int(nlive)
        if self.nlive < 2:
            raise ValueError("nlive must be >= 2")
        self.dynamic = bool(dynamic)
        self.walks = int(walks)
        if sample not in ("rwalk", "rslice"):
            raise ValueError("sample must be 'rwalk' or 'rslice'")
        self.sample = sample
        self.slices = default_slices(self.ndim) if slices is None else int(slices)
        if self.slices < 0:
            raise ValueError("slices must be >= 0")
        self.batch = int(math.ceil(self.nlive / 4)) if batch is None else int(batch)
        if not 1 <= self.batch < self.nlive:
            raise ValueError("batch must lie in [1, nlive)")
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
                    chol = _chol(mu[cand])
                    starts = cand[self.rng.integers(0, cand.shape[0], size=nb)]
                    bu, bl = self._walk(mu[starts], ml[starts], l_lo, chol)
                run, st = self._static(bu, bl, l_lo, l_hi, dlogz, maxiter, maxcall, checkpoint)
                self.runs.append(run)
                nbatch += 1
                if st == "plateau":
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
    ``rslice`` is the slice move on the same two paths: ``ns_slice_kernel``, or alabi_ns_slice_step around ``host_loglike``."""

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

    def walk(self, call, u0, logl0, logl_star, chol, scale, walks, walk_id0=0):
        ns, lib, dev, stream = self._ensure(), _lib.lib(), _dev(), _lib.current_stream()
        K = int(np.asarray(u0).shape[0])
        u = torch.as_tensor(np.ascontiguousarray(u0, dtype=np.float64), device=dev).clone()
        logl = torch.as_tensor(np.ascontiguousarray(logl0, dtype=np.float64), device=dev).clone()
        ch = torch.as_tensor(np.ascontiguousarray(chol, dtype=np.float64), device=dev)
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
        K = int(np.asarray(u0).shape[0])
        u = torch.as_tensor(np.ascontiguousarray(u0, dtype=np.float64), device=dev).clone()
        logl = torch.as_tensor(np.ascontiguousarray(logl0, dtype=np.float64), device=dev).clone()
        ch = torch.as_tensor(np.ascontiguousarray(chol, dtype=np.float64), device=dev)
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
