"""Proposal moves of the ensemble sampler: emcee's ``EnsembleSampler(moves=...)``.

The reference documents ``sampler_kwargs['moves']`` ("Custom proposal moves", alabi/core.py:2144) and hands it to
``emcee.EnsembleSampler`` (alabi/core.py:2319).  Six moves run on the GPU here -- emcee's whole red-blue family and its Gaussian
Metropolis move --, alone or as a weighted mixture from which ONE move is chosen per step, as emcee does:

* ``StretchMove(a=2.0)``        -- emcee 3 ``moves/stretch.py`` (the default);
* ``DEMove(sigma, gamma0)``     -- emcee 3 ``moves/de.py``: q = s + gamma (C[j2] - C[j1]) with two distinct walkers of the
  complementary set and gamma = gamma0 (1 + sigma n), n standard normal; gamma0 defaults to 2.38 / sqrt(2 ndim);
* ``SnookerMove(gammas=1.7)``   -- the snooker update of ter Braak & Vrugt (2008, eq. 4) on the sampler's two-way split: three
  distinct walkers z, z1, z2 of the complementary set, e the unit vector from z to s, q = s + gammas (e.z1 - e.z2) e, log
  factor (ndim - 1) (ln|q - z| - ln|s - z|).  Typically mixed with DE: ``[(DEMove(), 0.8), (SnookerMove(), 0.2)]``.

* ``WalkMove(s=None)``           -- emcee 3 ``moves/walk.py`` (Goodman & Weare 2010): a draw from the Gaussian around the walker with
  the sample covariance of ``s`` walkers of the complementary set (all of them by default), formed without a factorisation as
  q = x + sum_j z_j (C[j] - mean) / sqrt(s - 1) with standard normal z_j; log factor 0;
* ``KDEMove(bw_method=None)``   -- emcee 3 ``moves/kde.py``: an independence sampler that draws from a Gaussian KDE of the
  complementary set (``scipy.stats.gaussian_kde``'s "scott", "silverman" or scalar bandwidth) with the Hastings factor
  kde.logpdf(x) - kde.logpdf(q); it hops between separated modes in one step.  It wants MANY walkers per dimension: with 6
  complementary walkers in 5-D it still samples the right distribution but accepts about 5 % of its proposals.  A complementary
  set without a Cholesky factor (emcee raises ``LinAlgError``) rejects that half step's proposals and is counted in
  ``EnsembleSampler.kde_singular_half_steps``.

* ``GaussianMove(cov, mode="vector", factor=None)`` -- emcee 3 ``moves/gaussian.py``: a Metropolis proposal q = x + f C z around the
  walker itself, C C^T = cov (a scalar, a vector of variances or a full matrix, factorised on the host), z standard normal; mode
  "vector" moves every coordinate, "random" one coordinate drawn per walker and step, "sequential" coordinate (step mod ndim);
  with ``factor`` the scale f = exp(v), v ~ U(-ln factor, ln factor), is drawn once per step and ensemble; log factor 0.  A
  proposal reads no other walker, so a set of Gaussian moves alone is ``nwalkers`` independent Metropolis chains: it runs with ANY
  number of walkers, one workgroup per walker and all steps of a call in one launch (``ens_mh_kernel``).  Mixed with red-blue moves
  it runs with one launch per half step, the same rule applied to each half in turn.

* ``HMCMove(cov, step_size=None, n_leapfrog=8, jitter=None)`` -- Hamiltonian Monte Carlo on the surrogate's closed-form gradient
  (not an emcee move): the GP mean's gradient costs about two more passes over the training set, and a trajectory of ``n_leapfrog``
  gradient steps decorrelates a walker where a random-walk proposal needs hundreds of steps (ndim = 32: see README.md).  ``cov``
  estimates the posterior covariance as for ``GaussianMove`` -- the mass matrix is its inverse --; ``n_leapfrog=1`` is MALA.  Like
  a Metropolis set, a set of HMC moves is ``nwalkers`` independent chains on one workgroup per walker (``ens_hmc_kernel``), any
  ``nwalkers >= 1``; it holds HMC moves only (mixtures of several step sizes and trajectory lengths are the standard cure for
  periodic trajectories) and needs the fused log-probability: no ``prior_fn`` / ``like_fn``, no ``shard``.  The step size and the
  mass are adapted by a warm-up phase, ``EnsembleSampler.tune_hmc`` (one ``HMCMove``).

* ``NUTSMove(cov, step_size=None, max_depth=8, jitter=None)`` -- the No-U-Turn sampler (multinomial NUTS, Betancourt 2017, as in
  Stan) on the same gradient and mass matrix: the trajectory length is chosen per transition by doubling a tree of leapfrog steps
  until it turns back on itself, at most ``2 ** max_depth - 1`` gradient evaluations.  A set of NUTS moves runs on
  ``ens_nuts_kernel`` under HMC's restrictions; it holds NUTS moves only.  Its warm-up is ``EnsembleSampler.tune_nuts`` (one
  ``NUTSMove``): step-size search, dual averaging on the tree's mean acceptance statistic, windowed mass matrix.

``MHMove(proposal_function, ndim=None)`` is emcee's generic Metropolis move: ``proposal_function(coords[W, d], rng) -> (q[W, d],
log_factors[W])`` is a Python callable, so it runs on a host-driven step loop (one round trip per step: slow by nature), the
log-probability still on the device.  A set that holds an ``MHMove`` consists of ``MHMove`` objects only.

The subset of a walk move, the KDE move's row and all normals are counter-based Philox draws (streams 6-10 of the library), not
emcee's ``RandomState``.  ``parse_moves`` is pure host code (no GPU, no library): it accepts what emcee accepts -- None, one move, a list of moves, a
list of (move, weight) pairs -- and recognises this module's classes as well as foreign ``StretchMove`` / ``DEMove`` objects by
class name and attributes (``WalkMove`` with ``s``, ``KDEMove`` with ``bw_method`` too), so real ``emcee.moves`` objects of these
classes work where emcee is installed.  A foreign object with the attributes ``cov``, ``mode`` and ``factor`` is taken as a
``GaussianMove``; one of any class name with a callable ``get_proposal`` -- where emcee's ``MHMove`` and its ``GaussianMove``
subclass keep their proposal function -- as an ``MHMove``, on the host loop.  Every other move raises ``NotImplementedError``, in
particular emcee's ``DESnookerMove``, which stands for different arithmetic (half the published log factor, a four-way split):
ask for ``SnookerMove`` instead.
"""
from __future__ import annotations

import numpy as np

__all__ = ["StretchMove", "DEMove", "SnookerMove", "WalkMove", "KDEMove", "GaussianMove", "HMCMove", "NUTSMove", "MHMove", "MoveSet", "parse_moves",
           "MAX_MOVES", "KIND_STRETCH", "KIND_DE", "KIND_SNOOKER", "KIND_WALK", "KIND_KDE", "KIND_GAUSS", "KIND_HMC", "KIND_NUTS", "WALK_MAX_NC",
           "HMC_MAX_LEAPFROG", "NUTS_MAX_DEPTH"]

MAX_MOVES = 8                    # ALABI_MAX_MOVES of the library: the table travels in the draw kernel's arguments
KIND_STRETCH, KIND_DE, KIND_SNOOKER, KIND_WALK, KIND_KDE, KIND_GAUSS, KIND_HMC, KIND_NUTS = 0, 1, 2, 3, 4, 5, 6, 7
HMC_MAX_LEAPFROG = 64
NUTS_MAX_DEPTH = 10              # ALABI_NUTS_MAX_DEPTH of the library
GAUSS_MODES = {"vector": 0, "random": 1, "sequential": 2}
WALK_MAX_NC = 2048               # rows of a complementary half the walk move's kernel lists hold


class StretchMove:
    """Goodman & Weare stretch move with scale ``a`` (emcee.moves.StretchMove)."""

    def __init__(self, a=2.0):
        self.a = float(a)
        if not (self.a > 1.0 and np.isfinite(self.a)):
            raise ValueError("StretchMove needs a > 1")

    def __repr__(self):
        return f"StretchMove(a={self.a})"


class DEMove:
    """Differential-evolution move (emcee.moves.DEMove; Nelson et al. 2013, ter Braak 2006).  ``gamma0=None`` means
    2.38 / sqrt(2 ndim); mix in a ``DEMove(gamma0=1.0)`` at a small weight to let walkers jump between modes."""

    def __init__(self, sigma=1.0e-5, gamma0=None):
        self.sigma = float(sigma)
        self.gamma0 = None if gamma0 is None else float(gamma0)
        if not np.isfinite(self.sigma) or (self.gamma0 is not None and not np.isfinite(self.gamma0)):
            raise ValueError("DEMove needs finite sigma and gamma0")

    def __repr__(self):
        return f"DEMove(sigma={self.sigma}, gamma0={self.gamma0})"


class SnookerMove:
    """Snooker update (ter Braak & Vrugt 2008, eq. 4) with the fixed step ``gammas`` along the line through the walker and a
    walker of the complementary set.  Not emcee's ``DESnookerMove``: the log factor is the published one."""

    def __init__(self, gammas=1.7):
        self.gammas = float(gammas)
        if not np.isfinite(self.gammas):
            raise ValueError("SnookerMove needs a finite gammas")

    def __repr__(self):
        return f"SnookerMove(gammas={self.gammas})"


class WalkMove:
    """Walk move (emcee.moves.WalkMove; Goodman & Weare 2010): a Gaussian proposal with the sample covariance of ``s`` walkers of
    the complementary set, ``s=None``: all of them.  Needs 2 <= s <= nwalkers // 2."""

    def __init__(self, s=None):
        if s is not None:
            if int(s) != s or int(s) < 2:
                raise ValueError("WalkMove needs an integer s >= 2 (or None for the whole complementary set)")
            s = int(s)
        self.s = s

    def __repr__(self):
        return f"WalkMove(s={self.s})"


class KDEMove:
    """KDE move (emcee.moves.KDEMove): proposals from a Gaussian kernel density estimate of the complementary set, with
    ``bw_method`` as ``scipy.stats.gaussian_kde`` takes it -- None / "scott", "silverman" or a scalar; a callable is refused.
    Needs nwalkers >= 2 ndim + 2, and many more to accept often."""

    def __init__(self, bw_method=None):
        if callable(bw_method):
            raise NotImplementedError("KDEMove(bw_method=<callable>) is not available on the GPU: the bandwidth factor is resolved "
                                      "on the host before the run; pass 'scott', 'silverman' or a scalar")
        if isinstance(bw_method, str):
            if bw_method not in ("scott", "silverman"):
                raise ValueError("`bw_method` should be 'scott', 'silverman' or a scalar")
        elif bw_method is not None:
            bw_method = float(bw_method)
            if not (np.isfinite(bw_method) and bw_method > 0.0):
                raise ValueError("KDEMove needs a positive, finite scalar bw_method")
        self.bw_method = bw_method

    def factor(self, nc, ndim):
        """The bandwidth factor for ``nc`` complementary walkers, as gaussian_kde resolves it with unit weights (neff = nc)."""
        from types import SimpleNamespace
        from .kde import kde_factor
        return float(kde_factor(self.bw_method, SimpleNamespace(neff=float(nc), d=int(ndim))))

    def __repr__(self):
        return f"KDEMove(bw_method={self.bw_method!r})"


class GaussianMove:
    """Gaussian Metropolis move (emcee.moves.GaussianMove): q = x + f C z with C C^T = ``cov``.  ``cov``: a positive scalar
    (isotropic), a vector of ``ndim`` positive variances (diagonal) or a positive definite ``ndim`` x ``ndim`` matrix (factorised
    here by ``numpy.linalg.cholesky``).  ``mode``: "vector" (every coordinate), "random" (one coordinate per walker and step) or
    "sequential" (coordinate step mod ndim); a full matrix allows "vector" only.  ``factor``: None or a number > 1 -- the scale
    is then multiplied by exp(v), v ~ U(-ln factor, ln factor), one draw per step and ensemble."""

    def __init__(self, cov, mode="vector", factor=None):
        if mode not in GAUSS_MODES:
            raise ValueError("GaussianMove: mode must be 'vector', 'random' or 'sequential'")
        self.mode = mode
        if factor is not None:
            factor = float(factor)
            if not (np.isfinite(factor) and factor > 1.0):
                raise ValueError("GaussianMove: factor must be None or a finite number > 1")
        self.factor = factor
        try:
            c = np.array(cov, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("Invalid proposal scale dimensions") from None
        if c.ndim > 2 or (c.ndim == 2 and c.shape[0] != c.shape[1]) or c.size == 0:
            raise ValueError("Invalid proposal scale dimensions")
        if not np.all(np.isfinite(c)):
            raise ValueError("GaussianMove: cov must be finite")
        self.cov = c
        self.form = ("scalar", "vector", "matrix")[c.ndim]
        if c.ndim < 2:
            if np.any(c <= 0.0):
                raise ValueError("GaussianMove: a scalar or diagonal cov must be positive")
            self._scale = np.sqrt(c)               # scalar, or [ndim]
        else:
            if mode != "vector":
                raise ValueError("GaussianMove: a full covariance matrix allows mode='vector' only")
            try:
                self._scale = np.linalg.cholesky(c)
            except np.linalg.LinAlgError:
                raise ValueError("GaussianMove: the covariance matrix is not positive definite") from None
        self.ndim = None if c.ndim == 0 else int(c.shape[0])

    @property
    def diagonal(self):
        return self.form != "matrix"

    def scale_matrix(self, ndim):
        """The lower-triangular scale factor C [ndim, ndim] (row-major, zeros above the diagonal) the library takes."""
        if self.ndim is not None and self.ndim != int(ndim):
            raise ValueError("Dimension mismatch in proposal")
        if self.form == "matrix":
            return np.ascontiguousarray(np.tril(self._scale))
        return np.ascontiguousarray(np.diag(np.broadcast_to(self._scale, (int(ndim),)).astype(np.float64)))

    def __repr__(self):
        return f"GaussianMove(cov=<{self.form}>, mode={self.mode!r}, factor={self.factor})"


class HMCMove:
    """Hamiltonian Monte Carlo move on the gradient of the fused log-probability (GP mean through the scalers, the y map, normal
    priors).  ``cov`` as for ``GaussianMove``: a positive scalar, a vector of ``ndim`` positive variances or a positive definite
    matrix, an estimate of the POSTERIOR covariance; with C C^T = cov the mass matrix is cov^-1 and one step is, in whitened
    momentum z: z0 ~ N(0, I); z = z0 + (e / 2) C^T g; ``n_leapfrog`` times q += e C z, z += e C^T grad lnp(q) (e / 2 the last time);
    accept iff lnp(q) - |z|^2 / 2 - lnp(x) + |z0|^2 / 2 > ln u and q lies in the open box -- only the end point is tested, in
    between the trajectory follows the surrogate's smooth extension.  ``n_leapfrog=1`` is MALA, the
    Metropolis-adjusted Langevin algorithm; at most 64.  ``step_size=None`` resolves to ``ndim ** -0.25``, the conventional scaling
    of the optimal step with the dimension for a well-estimated ``cov``: a starting point only -- ``EnsembleSampler.tune_hmc``
    (``run_emcee``'s ``sampler_kwargs["hmc_warmup"]``) adapts the step size by dual averaging and, from the walkers' positions,
    ``cov`` itself, Stan-style; without it look at the acceptance fraction (0.6 - 0.9 is the usual aim) and set the step.  ``jitter``: None or a number > 1 with the meaning of
    ``GaussianMove(factor=)`` -- e = step_size exp(v), v ~ U(-ln jitter, ln jitter), one draw per step and ensemble (ln jitter is
    rounded to a multiple of 2^-36 on its way into the library's table).  Nothing is adapted during a run: adaptation is the
    warm-up phase ``tune_hmc``, after which the sampler's move is a new ``HMCMove`` with the step size and ``cov`` it found."""

    def __init__(self, cov, step_size=None, n_leapfrog=8, jitter=None):
        if step_size is not None:
            step_size = float(step_size)
            if not (np.isfinite(step_size) and step_size > 0.0):
                raise ValueError("HMCMove: step_size must be None or a positive, finite number")
        self.step_size = step_size
        if isinstance(n_leapfrog, bool) or int(n_leapfrog) != n_leapfrog or not (1 <= int(n_leapfrog) <= HMC_MAX_LEAPFROG):
            raise ValueError(f"HMCMove: n_leapfrog must be an integer in 1 ... {HMC_MAX_LEAPFROG}")
        self.n_leapfrog = int(n_leapfrog)
        if jitter is not None:
            jitter = float(jitter)
            if not (np.isfinite(jitter) and jitter > 1.0 and np.log(jitter) < 511.0):
                raise ValueError("HMCMove: jitter must be None or a finite number > 1")
        self.jitter = jitter
        try:
            c = np.array(cov, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("Invalid proposal scale dimensions") from None
        if c.ndim > 2 or (c.ndim == 2 and c.shape[0] != c.shape[1]) or c.size == 0:
            raise ValueError("Invalid proposal scale dimensions")
        if not np.all(np.isfinite(c)):
            raise ValueError("HMCMove: cov must be finite")
        self.cov = c
        self.form = ("scalar", "vector", "matrix")[c.ndim]
        if c.ndim < 2:
            if np.any(c <= 0.0):
                raise ValueError("HMCMove: a scalar or diagonal cov must be positive")
            self._scale = np.sqrt(c)
        else:
            try:
                self._scale = np.linalg.cholesky(c)
            except np.linalg.LinAlgError:
                raise ValueError("HMCMove: the covariance matrix is not positive definite") from None
        self.ndim = None if c.ndim == 0 else int(c.shape[0])

    @property
    def diagonal(self):
        return self.form != "matrix"

    @property
    def ln_jitter(self):
        """ln jitter as the library's table carries it: rounded to a multiple of 2^-36, 0.0 for None."""
        return 0.0 if self.jitter is None else float(np.round(np.log(self.jitter) * 2.0 ** 36) / 2.0 ** 36)

    def resolved_step_size(self, ndim):
        return float(ndim) ** -0.25 if self.step_size is None else self.step_size

    scale_matrix = GaussianMove.scale_matrix

    def __repr__(self):
        return f"HMCMove(cov=<{self.form}>, step_size={self.step_size}, n_leapfrog={self.n_leapfrog}, jitter={self.jitter})"


class NUTSMove:
    """No-U-Turn sampler move: multinomial NUTS (Betancourt 2017, as in Stan) on the gradient of the fused log-probability, in
    ``HMCMove``'s whitened momentum -- ``cov``, ``step_size`` and ``jitter`` mean what they mean there and are validated alike.  One
    transition doubles a tree of leapfrog steps, forward or backward by a drawn bit, until the tree turns back on itself (rho . z
    <= 0 at either end, rho the sum of the tree's momenta), a new subtree turns inside or diverges (energy error beyond 1000; both
    drop that subtree), or ``max_depth`` doublings (1 ... 10) are done: at most ``2 ** max_depth - 1`` gradient evaluations.  The
    next state is drawn from the tree's points with weights exp(-energy error), biased towards the newer half; a point outside the
    open box has weight 0 -- the orbit itself follows the surrogate's smooth extension.  Stan's extra U-turn
    checks across subtree joints are not built.  ``EnsembleSampler.tune_nuts`` (``run_emcee``:
    ``sampler_kwargs["nuts_warmup"]``) is this move's warm-up: ``NUTSMove(cov_guess)`` followed by it leaves no knob to set by hand.
    It adapts the step size on the mean of min(1, exp(-energy error)) over all leaves of a tree, which is NUTS's statistic; an
    ``HMCMove`` tuned by ``tune_hmc`` lands on another step size, that of a fixed-length trajectory's end point."""

    def __init__(self, cov, step_size=None, max_depth=8, jitter=None):
        if isinstance(max_depth, bool) or int(max_depth) != max_depth or not (1 <= int(max_depth) <= NUTS_MAX_DEPTH):
            raise ValueError(f"NUTSMove: max_depth must be an integer in 1 ... {NUTS_MAX_DEPTH}")
        self.max_depth = int(max_depth)
        try:
            h = HMCMove(cov, step_size=step_size, n_leapfrog=1, jitter=jitter)     # its validation is HMCMove's
        except ValueError as err:
            raise ValueError(str(err).replace("HMCMove", "NUTSMove")) from None
        self.step_size, self.jitter, self.cov, self.form, self._scale, self.ndim = h.step_size, h.jitter, h.cov, h.form, h._scale, h.ndim

    diagonal = HMCMove.diagonal
    ln_jitter = HMCMove.ln_jitter
    resolved_step_size = HMCMove.resolved_step_size
    scale_matrix = GaussianMove.scale_matrix

    def __repr__(self):
        return f"NUTSMove(cov=<{self.form}>, step_size={self.step_size}, max_depth={self.max_depth}, jitter={self.jitter})"


class MHMove:
    """Generic Metropolis move (emcee.moves.MHMove): ``proposal_function(coords[W, d], rng) -> (q[W, d], log_factors[W])`` with
    ``rng`` a ``numpy.random.RandomState``.  A Python callable cannot run on the device: the sampler drives such a set from the
    host, one round trip per step (slow by nature), and evaluates the log-probability on the device."""

    def __init__(self, proposal_function, ndim=None):
        if not callable(proposal_function):
            raise ValueError("MHMove needs a callable proposal_function(coords, rng) -> (q, log_factors)")
        self.get_proposal = proposal_function
        self.ndim = None if ndim is None else int(ndim)

    def __repr__(self):
        return f"MHMove({getattr(self.get_proposal, '__name__', 'proposal_function')}, ndim={self.ndim})"


def _table_row(m, ndim, nc=None):
    """(kind, p0, p1) of a move in the library's table.  ``nc`` = (|C| of split 0, |C| of split 1): a KDE move's two factors need
    it and are NaN without."""
    if isinstance(m, GaussianMove):
        return KIND_GAUSS, 0.0 if m.factor is None else float(np.log(m.factor)), float(GAUSS_MODES[m.mode])
    if isinstance(m, HMCMove):
        return KIND_HMC, m.resolved_step_size(ndim), float(m.n_leapfrog) + m.ln_jitter / 512.0
    if isinstance(m, NUTSMove):
        return KIND_NUTS, m.resolved_step_size(ndim), float(m.max_depth) + m.ln_jitter / 512.0
    if isinstance(m, MHMove):
        return -1, 0.0, 0.0                        # not a row of the library's table: the host loop runs it
    if isinstance(m, WalkMove):
        return KIND_WALK, 0.0 if m.s is None else float(m.s), 0.0
    if isinstance(m, KDEMove):
        if nc is None:
            return KIND_KDE, np.nan, np.nan
        return KIND_KDE, m.factor(nc[0], ndim), m.factor(nc[1], ndim)
    if isinstance(m, DEMove):
        return KIND_DE, 2.38 / np.sqrt(2 * ndim) if m.gamma0 is None else m.gamma0, m.sigma
    if isinstance(m, SnookerMove):
        return KIND_SNOOKER, m.gammas, 0.0
    return KIND_STRETCH, m.a, 0.0


class MoveSet:
    """A parsed move set: ``moves`` (this module's objects), normalised ``weights`` and the table the library takes --
    ``kind``, ``cum`` = np.cumsum(w / w.sum()), ``p0`` (a | gamma0 with its default resolved | gammas | s, 0 for all | KDE factor of
    split 0 | ln factor, 0 for None | HMC step size, resolved), ``p1`` (0 | sigma | 0 | 0 | KDE factor of split 1 | mode 0 / 1 / 2 |
    n_leapfrog + ln jitter / 512; a NUTS move: step size and max_depth + ln jitter / 512).  A Gaussian, HMC or NUTS move's scale factor travels apart: ``scales()``.  The KDE factors depend on the number of walkers: they are NaN
    until ``resolve(nwalkers)`` (called by EnsembleSampler, or pass ``nwalkers`` here)."""

    def __init__(self, moves, weights, ndim, nwalkers=None):
        self.moves = list(moves)
        self.ndim = int(ndim)
        w = np.asarray(weights, dtype=np.float64)
        self.weights = w / w.sum()
        self.cum = np.cumsum(w / w.sum())
        self.nwalkers = None
        self._fill(None)
        if nwalkers is not None:
            self.resolve(nwalkers)

    def _fill(self, nc):
        rows = [_table_row(m, self.ndim, nc) for m in self.moves]
        self.kind = np.array([r[0] for r in rows], dtype=np.int32)
        self.p0 = np.array([r[1] for r in rows], dtype=np.float64)
        self.p1 = np.array([r[2] for r in rows], dtype=np.float64)

    def resolve(self, nwalkers):
        """Check the moves against the number of walkers and fill in what depends on it (the KDE factors).  The complementary set
        has W - n0 walkers in split 0 and n0 in split 1, n0 = (W + 1) // 2."""
        W = int(nwalkers)
        n0 = (W + 1) // 2
        nc = (W - n0, n0)
        for m in self.moves:
            if isinstance(m, WalkMove):
                s0 = min(nc) if m.s is None else m.s
                if min(nc) < 2:
                    raise ValueError("WalkMove needs two walkers in each half of the ensemble: nwalkers >= 4")
                if s0 > min(nc):
                    raise ValueError(f"WalkMove(s={m.s}) draws s distinct walkers from the complementary half, which has {min(nc)} "
                                     f"with nwalkers = {W}: s <= nwalkers // 2")
                if max(nc) > WALK_MAX_NC:
                    raise ValueError(f"WalkMove runs with at most {2 * WALK_MAX_NC} walkers per ensemble")
            elif isinstance(m, KDEMove):
                if min(nc) < self.ndim + 1:
                    raise ValueError(f"KDEMove needs more complementary walkers than dimensions (a covariance of full rank): nwalkers "
                                     f">= 2 ndim + 2 = {2 * self.ndim + 2}, got {W}")
        self.nwalkers = W
        self._fill(nc)
        return self

    def scales(self):
        """[(k, C [ndim, ndim], diagonal)] for the Gaussian, HMC and NUTS moves of the table (alabi_ens_set_move_scale, ahead of
        alabi_ens_set_moves)."""
        return [(k, m.scale_matrix(self.ndim), m.diagonal) for k, m in enumerate(self.moves) if isinstance(m, (GaussianMove, HMCMove, NUTSMove))]

    @property
    def has_hmc(self):
        return bool(np.any(self.kind == KIND_HMC))

    @property
    def all_hmc(self):
        """Every member is an HMCMove: independent chains on the surrogate's gradient (ens_hmc_kernel)."""
        return bool(len(self.moves) > 0 and np.all(self.kind == KIND_HMC))

    @property
    def has_nuts(self):
        return bool(np.any(self.kind == KIND_NUTS))

    @property
    def all_nuts(self):
        """Every member is a NUTSMove: independent chains on the surrogate's gradient (ens_nuts_kernel)."""
        return bool(len(self.moves) > 0 and np.all(self.kind == KIND_NUTS))

    @property
    def has_gauss(self):
        return bool(np.any(self.kind == KIND_GAUSS))

    @property
    def all_metropolis(self):
        """Every member is a GaussianMove: the walkers are independent Metropolis chains (ens_mh_kernel)."""
        return bool(len(self.moves) > 0 and np.all(self.kind == KIND_GAUSS))

    @property
    def all_mh(self):
        """Every member is an MHMove: the host-driven step loop."""
        return bool(len(self.moves) > 0 and all(isinstance(m, MHMove) for m in self.moves))

    @property
    def has_de(self):
        return bool(np.any(self.kind == KIND_DE))

    @property
    def has_snooker(self):
        return bool(np.any(self.kind == KIND_SNOOKER))

    @property
    def has_walk(self):
        return bool(np.any(self.kind == KIND_WALK))

    @property
    def has_kde(self):
        return bool(np.any(self.kind == KIND_KDE))

    @property
    def multi_partner(self):
        """Some move reads more than one partner row (DE, snooker) or the whole complementary half (walk, KDE): one launch per
        half step, no sharding."""
        return self.has_de or self.has_snooker or self.has_walk or self.has_kde

    def __len__(self):
        return len(self.moves)


def _as_move(obj):
    """This module's move for ``obj``: one of its own, or a foreign object recognised by class name and attributes."""
    if isinstance(obj, (StretchMove, DEMove, SnookerMove, WalkMove, KDEMove, GaussianMove, HMCMove, NUTSMove, MHMove)):
        return obj
    name = type(obj).__name__
    if name == "GaussianMove" and all(hasattr(obj, a) for a in ("cov", "mode", "factor")):
        return GaussianMove(obj.cov, mode=obj.mode, factor=obj.factor)
    if callable(getattr(obj, "get_proposal", None)):
        return MHMove(obj.get_proposal, ndim=getattr(obj, "ndim", None))
    if name == "WalkMove" and hasattr(obj, "s"):
        return WalkMove(s=obj.s)
    if name == "KDEMove" and hasattr(obj, "bw_method"):
        return KDEMove(bw_method=obj.bw_method)
    if name == "StretchMove" and hasattr(obj, "a"):
        return StretchMove(a=obj.a)
    if name == "DEMove" and hasattr(obj, "sigma") and hasattr(obj, "gamma0"):
        return DEMove(sigma=obj.sigma, gamma0=obj.gamma0)
    hint = ""
    if name == "DESnookerMove":
        hint = ("; emcee's DESnookerMove stands for different arithmetic (half the published log factor, a four-way split) -- "
                "use alabi_amd.moves.SnookerMove, the published snooker update")
    if name in ("GaussianMove", "MHMove"):
        hint = ("; a Metropolis move is recognised by its attributes (cov, mode and factor, or a callable get_proposal) -- use "
                "alabi_amd.moves.GaussianMove")
    raise NotImplementedError(f"move {name} is not available on the GPU: the ensemble sampler runs StretchMove, DEMove, WalkMove, "
                              f"KDEMove, alabi_amd.moves.SnookerMove and weighted mixtures of them{hint}")


def parse_moves(moves, ndim):
    """``moves`` as emcee's EnsembleSampler takes it -> ``MoveSet``, or None for None (the default stretch move)."""
    if moves is None:
        return None
    if isinstance(moves, (list, tuple)):
        items = list(moves)
        if not items:
            raise ValueError("moves must not be empty")
        if all(isinstance(it, (list, tuple)) and len(it) == 2 for it in items):
            objs, weights = [it[0] for it in items], [float(it[1]) for it in items]
        else:
            objs, weights = items, [1.0] * len(items)
    else:
        objs, weights = [moves], [1.0]
    parsed = [_as_move(o) for o in objs]
    w = np.asarray(weights, dtype=np.float64)
    if not np.all(np.isfinite(w)) or np.any(w < 0.0) or not (w.sum() > 0.0):
        raise ValueError("move weights must be non-negative, finite and not all zero")
    if len(parsed) > MAX_MOVES:
        raise ValueError(f"at most {MAX_MOVES} moves in a mixture")
    if any(isinstance(m, MHMove) for m in parsed) and not all(isinstance(m, MHMove) for m in parsed):
        raise ValueError("a move set that holds an MHMove must consist of MHMove objects only: its proposal function runs on the "
                         "host, every other move on the device")
    if any(isinstance(m, HMCMove) for m in parsed) and not all(isinstance(m, HMCMove) for m in parsed):
        raise ValueError("a move set that holds an HMCMove must consist of HMCMove objects only: mixtures of an HMCMove with other "
                         "kinds of move are not built (ens_hmc_kernel runs a table of HMC moves alone)")
    if any(isinstance(m, NUTSMove) for m in parsed) and not all(isinstance(m, NUTSMove) for m in parsed):
        raise ValueError("a move set that holds a NUTSMove must consist of NUTSMove objects only: mixtures of a NUTSMove with other "
                         "kinds of move are not built (ens_nuts_kernel runs a table of NUTS moves alone)")
    for m in parsed:
        if isinstance(m, (GaussianMove, HMCMove, NUTSMove)):
            m.scale_matrix(int(ndim))              # emcee's ValueError("Dimension mismatch in proposal")
        elif isinstance(m, MHMove) and m.ndim is not None and m.ndim != int(ndim):
            raise ValueError("Dimension mismatch in proposal")
    return MoveSet(parsed, w, int(ndim))
