"""GPU-resident ensemble sampler exposing the emcee.EnsembleSampler members alabi uses.

Reference seam: ``EnsembleSampler(nwalkers, ndim, log_prob_fn,
pool=)``, ``.run_mcmc(p0, nsteps, progress=True)``, ``.get_chain(discard, thin, flat)``,
``.get_last_sample().coords``, ``.acceptance_fraction``, ``.get_autocorr_time(tol=0)``
(alabi/core.py:2319-2387, alabi/mcmc_utils.py:45).

Instead of a Python ``log_prob_fn`` called once per walker, the log-probability
(surrogate GP mean + uniform box prior, alabi/core.py:2073-2100) is evaluated inside the
HIP half-step kernel; walker coordinates, log-probabilities, the random draws and the
chain never leave HBM during a run.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np
import torch

from . import _lib
from .gp import HipGP, _dev, _to_dev
from . import diagnostics
from .mcmc_utils import integrated_time
from .moves import parse_moves

__all__ = ["EnsembleSampler", "MaximizeResult", "State"]


class State:
    def __init__(self, coords, log_prob=None):
        self.coords = coords
        self.log_prob = log_prob
        self.blobs = None
        self.random_state = None

    def __iter__(self):
        return iter((self.coords, self.log_prob, self.random_state))


class MaximizeResult:
    """What ``EnsembleSampler.maximize`` returns: device tensors ``x``, ``log_prob``, ``iterations``, ``evaluations``, ``status``,
    ``grad_norm`` and, with ``trace=n``, ``trace`` -- the raw [S, n, 4] doubles of ``alabi_ens_maximize`` (lp, step length, the held
    set's bits, update flag; NaN rows beyond the last iteration) -- and its columns decoded: ``trace_log_prob``, ``trace_step``,
    ``trace_held`` (int64), ``trace_updated`` (bool)."""
    x = log_prob = iterations = evaluations = status = grad_norm = None
    trace = trace_log_prob = trace_step = trace_held = trace_updated = None


class EnsembleSampler:
    def __init__(self, nwalkers, ndim, gp, y, bounds, seed=None, a=2.0, pool=None, live_dangerously=False,
                 n_ensembles=1, logp_affine=(1.0, 0.0), normal_prior=None, logp_map=None, prior_fn=None, like_fn=None,
                 gate_box=True, shard=False, group=None, moves=None, **unused):
        """``n_ensembles`` > 1 runs that many INDEPENDENT ensembles of ``nwalkers`` walkers in the same kernel
        launches (rows [e*nwalkers, (e+1)*nwalkers) of every array belong to ensemble e).
        ``logp_affine=(scale, shift)``: log-probability = scale * GP mean + shift inside the box (an affine y scaler).
        ``normal_prior=(mean[d], std[d])``: independent normal priors on top of the box (NaN / non-positive std = none on
        that coordinate), the reference's ``lnprior_normal``.
        ``logp_map``: None, "nlog" or "log" -- the inverse of the reference's non-affine y scalers (-10^x, 10^x,
        alabi/utility.py:62-71) applied to the (affinely mapped) GP mean inside the kernels.
        ``prior_fn`` / ``like_fn``: arbitrary HOST callables on a batch of points in the sampler's coordinates
        ([n,d] -> [n]); the reference's lnprob = like_fn + prior_fn with any Python callable (alabi/core.py:2073-2100).
        With either one set, every half step is split into a propose launch, the host call and an accept launch
        (alabi_ens_propose / alabi_ens_accept): the ensemble, the draws and the accept test stay on the device.  With
        ``like_fn=None`` the surrogate part is evaluated by the propose kernel; ``gate_box`` says whether that value is
        -inf outside ``bounds`` (True when the prior is the box itself, False when ``prior_fn`` is the whole prior).
        ``moves``: emcee's proposal moves (alabi_amd.moves) -- None (the stretch move with ``a``), a ``StretchMove``,
        ``DEMove``, ``SnookerMove`` (the snooker update of ter Braak & Vrugt 2008), ``WalkMove`` or ``KDEMove``, a list of them, or a
        list of (move, weight) pairs from which one move is chosen per step; emcee's own ``StretchMove`` / ``DEMove`` / ``WalkMove`` /
        ``KDEMove`` objects are recognised, its ``DESnookerMove`` is refused.  A ``GaussianMove(cov, mode, factor)`` is emcee's
        Gaussian Metropolis move: a set of Gaussian moves alone is ``nwalkers`` independent chains (any ``nwalkers >= 1``; one
        workgroup per walker and all steps of a call in one launch, ``last_path == "metropolis"``), mixed with red-blue moves it
        runs with one launch per half step.  An ``MHMove(proposal_function)`` -- or any object with a callable ``get_proposal``,
        emcee's own Metropolis moves among them -- runs on a host-driven loop: per step the walkers travel to the host, the
        proposal function is called with a ``numpy.random.RandomState`` seeded from ``seed`` and the log-probability of the
        proposals is evaluated on the device; one round trip per step, slow by nature; ``n_ensembles == 1`` and such moves only.
        Neither can be sharded.  An ``HMCMove(cov, step_size, n_leapfrog, jitter)`` -- alone or in a weighted mixture of HMC
        moves -- runs Hamiltonian Monte Carlo on the surrogate's closed-form gradient: independent chains again (any ``nwalkers >=
        1``, ``last_path == "hmc"``, ``ens_hmc_kernel``); it needs the fused log-probability (no ``prior_fn`` / ``like_fn``) and
        cannot be sharded.  A ``NUTSMove(cov, step_size, max_depth, jitter)`` -- alone or in a mixture of NUTS moves -- is the
        No-U-Turn sampler on the same gradient under the same restrictions (``last_path == "nuts"``, ``ens_nuts_kernel``);
        ``nuts_stats`` reports its trees.  Moves work with ``n_ensembles``
        > 1 and with host callables; a set holding a ``DEMove`` needs ``nwalkers >= 4``, one holding a ``SnookerMove`` ``nwalkers >=
        6``, a ``WalkMove(s)`` ``2 <= s <= nwalkers // 2``, a ``KDEMove`` ``nwalkers >= 2 ndim + 2`` (and warns below about
        ``8 (ndim + 1)``: few walkers per dimension mean few accepted proposals); each of these runs with one launch per half step
        and cannot be sharded.  ``kde_singular_half_steps`` counts the half steps whose KDE had no Cholesky factor (all their
        proposals were rejected; emcee would raise ``LinAlgError``).
        ``shard=True`` under an initialised ``torch.distributed`` group of more than one rank (``group``: default WORLD): ONE
        ensemble whose active half is partitioned over the ranks, an all-gather of the new rows per half step
        (alabi_amd.dist.ShardedRun -> alabi_ens_run_sharded); every rank must construct the sampler with the same arguments and
        make the same calls, and every rank ends with the same chain (counter-based draws).  The reference's analogue:
        ``EnsembleSampler(..., pool=pool)`` spreading one ensemble's lnprob calls over processes (alabi/core.py:2300, :2322)."""
        if not isinstance(gp, HipGP):
            raise TypeError("EnsembleSampler needs the HipGP surrogate (the log-probability is fused into the kernel)")
        self.nwalkers = int(nwalkers)
        self.n_ensembles = int(n_ensembles)
        self.total_walkers = self.nwalkers * self.n_ensembles
        self.ndim = int(ndim)
        if self.ndim != gp.ndim:
            raise ValueError("ndim does not match the GP")
        if self.nwalkers < 2 * self.ndim and not live_dangerously:
            few = parse_moves(moves, self.ndim)           # looked at here only to see whether the rule applies: a set of
            if few is None or not (few.all_metropolis or few.all_mh or few.all_hmc or few.all_nuts):   # such moves have no halves to keep populated
                raise RuntimeError("It is unadvisable to use a red-blue move with fewer walkers than twice the "
                                   "number of dimensions.")
        self.gp = gp
        self._y = y
        self.bounds = np.ascontiguousarray(np.asarray(bounds, dtype=np.float64).reshape(self.ndim, 2))
        self.a = float(a)
        self.logp_affine = (float(logp_affine[0]), float(logp_affine[1]))
        self.normal_prior = None
        if normal_prior is not None:
            m = np.ascontiguousarray(np.asarray(normal_prior[0], dtype=np.float64).reshape(self.ndim))
            sd = np.ascontiguousarray(np.asarray(normal_prior[1], dtype=np.float64).reshape(self.ndim))
            self.normal_prior = (m, sd)
        if logp_map not in (None, "nlog", "log"):
            raise ValueError("logp_map must be None, 'nlog' or 'log'")
        self.logp_map = logp_map
        self.prior_fn_host = prior_fn
        self.like_fn_host = like_fn
        self.generic = prior_fn is not None or like_fn is not None
        self.gate_box = bool(gate_box)
        if self.generic and self.n_ensembles != 1:
            raise ValueError("host callables need n_ensembles == 1")
        self.shard, self.group, self._sharded, self._sharded_ens = bool(shard), group, None, None
        if self.shard and (self.generic or self.n_ensembles != 1):
            raise ValueError("shard=True needs the fused log-probability (no host callables) and n_ensembles == 1")
        self._move_set = parse_moves(moves, self.ndim)
        metropolis = self._move_set is not None and (self._move_set.all_metropolis or self._move_set.all_mh or self._move_set.all_hmc or
                                                     self._move_set.all_nuts)
        if self.nwalkers < 1:
            raise ValueError("nwalkers must be at least 1")
        if self.nwalkers < 2 and not metropolis:
            raise ValueError("a red-blue move needs at least two walkers")
        if self._move_set is not None and (self._move_set.has_gauss or self._move_set.all_mh):
            if self.shard:
                raise ValueError("shard=True cannot run a GaussianMove or an MHMove: a Metropolis proposal reads no other walker, so "
                                 "there is nothing to exchange -- run replicas (n_ensembles, or one sampler per rank) instead")
            if self._move_set.all_mh and self.n_ensembles != 1:
                raise ValueError("an MHMove runs on the host loop, which needs n_ensembles == 1")
        if self._move_set is not None and self._move_set.has_hmc:
            if self.generic:
                raise ValueError("an HMCMove needs the gradient of the log-probability, which exists for the fused surrogate only: "
                                 "a Python prior_fn or like_fn (the host-callback path) has none -- gradients through host "
                                 "callables are not built")
            if self.shard:
                raise ValueError("shard=True cannot run an HMCMove: the sharded form is not built (a trajectory reads no other "
                                 "walker, so there is nothing to exchange -- run replicas with n_ensembles instead)")
        if self._move_set is not None and self._move_set.has_nuts:
            if self.generic:
                raise ValueError("a NUTSMove needs the gradient of the log-probability, which exists for the fused surrogate only: "
                                 "a Python prior_fn or like_fn (the host-callback path) has none")
            if self.shard:
                raise ValueError("shard=True cannot run a NUTSMove: the sharded form is not built (a tree reads no other walker, so "
                                 "there is nothing to exchange -- run replicas with n_ensembles instead)")
        self._mh_rng = None
        if self._move_set is not None and self._move_set.multi_partner:
            if self._move_set.has_de and self.nwalkers < 4:
                raise ValueError("DEMove draws two distinct walkers from the complementary half: nwalkers >= 4")
            if self._move_set.has_snooker and self.nwalkers < 6:
                raise ValueError("SnookerMove draws three distinct walkers from the complementary half: nwalkers >= 6")
            if self.shard:
                raise ValueError("shard=True cannot run a DEMove, SnookerMove, WalkMove or KDEMove: the sharded history links one "
                                 "partner row per proposal")
            self._move_set.resolve(self.nwalkers)          # WalkMove's s and KDEMove's ndim against nwalkers; the KDE factors
            if self._move_set.has_kde and self.nwalkers // 2 < 4 * (self.ndim + 1):
                import warnings
                warnings.warn(f"KDEMove with {self.nwalkers // 2} complementary walkers in {self.ndim} dimensions: a kernel density "
                              f"estimate from fewer than about 4 (ndim + 1) = {4 * (self.ndim + 1)} points makes poor proposals and "
                              "few are accepted (about 5 % with 6 walkers in 5-D); use more walkers", RuntimeWarning, stacklevel=2)
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(2, dtype=np.uint32).view(np.uint64)[0])
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.iteration = 0
        self._rng_step = 0      # global step index of the counter-based draws: never rewound (reset() keeps it, as emcee's
                                # reset() keeps the RandomState), so a burn-in / reset / production run uses fresh draws
        self._coords = None
        self._logp = None
        self._chains = []
        self._chain_lps = []
        self._thins = []
        self._naccept = torch.zeros(self.total_walkers, dtype=torch.int64, device=_dev())
        self._stream = torch.cuda.Stream()
        self._ens = None
        self._ens_gp_handle = None
        self.last_run_seconds = 0.0

    # ------------------------------------------------------------------ handle lifetime
    def _ensure_ens(self):
        h = self.gp.sampler_handle(self._y, surrogate_on_device=self.like_fn_host is None)
        if self._ens is not None and self._ens_gp_handle is not None and self._ens_gp_handle.value == h.value:
            return
        self._release()
        e = C.c_void_p()
        create = _lib.lib().alabi_ens_create if self.nwalkers >= 2 else _lib.lib().alabi_ens_create_metropolis
        st = create(h, self.nwalkers, self.ndim, self.n_ensembles,
                                         _lib.host_doubles(self.bounds.ravel()), C.c_ulonglong(self.seed), C.byref(e))
        _lib.check(st, "alabi_ens_create")
        if self.logp_affine != (1.0, 0.0):
            _lib.check(_lib.lib().alabi_ens_set_logp_affine(e, self.logp_affine[0], self.logp_affine[1]),
                       "alabi_ens_set_logp_affine")
        if self.normal_prior is not None:
            _lib.check(_lib.lib().alabi_ens_set_normal_prior(e, _lib.host_doubles(self.normal_prior[0]),
                                                             _lib.host_doubles(self.normal_prior[1])),
                       "alabi_ens_set_normal_prior")
        if self.logp_map is not None:
            _lib.check(_lib.lib().alabi_ens_set_logp_map(e, {"nlog": 1, "log": 2}[self.logp_map]), "alabi_ens_set_logp_map")
        if self._move_set is not None and not self._move_set.all_mh:
            m = self._move_set
            for k, Cm, diagonal in m.scales():            # a Gaussian move's factor goes ahead of the table that names it
                _lib.check(_lib.lib().alabi_ens_set_move_scale(e, k, _lib.host_doubles(Cm.ravel()), int(diagonal)),
                           "alabi_ens_set_move_scale")
            _lib.check(_lib.lib().alabi_ens_set_moves(e, len(m), (C.c_int * len(m))(*[int(k) for k in m.kind]),
                                                      _lib.host_doubles(m.cum), _lib.host_doubles(m.p0), _lib.host_doubles(m.p1)),
                       "alabi_ens_set_moves")
        self._ens = e
        self._ens_gp_handle = C.c_void_p(h.value)
        self._nuts_transitions = 0                        # a new handle's NUTS sums start at zero

    @property
    def moves(self):
        """The configured moves as (move, normalised weight) pairs; the default is one StretchMove(a)."""
        if getattr(self, "_move_set", None) is None:
            from .moves import StretchMove
            return [(StretchMove(self.a), 1.0)]
        return list(zip(self._move_set.moves, (float(w) for w in self._move_set.weights)))

    @property
    def kde_singular_half_steps(self):
        """Half steps (counted per ensemble) of this sampler's handle in which a KDEMove found a complementary set without a
        Cholesky factor -- emcee would raise LinAlgError; here every proposal of that half step was rejected."""
        if getattr(self, "_ens", None) is None:
            return 0
        n = C.c_longlong(0)
        _lib.check(_lib.lib().alabi_ens_kde_singular(self._ens, C.byref(n)), "alabi_ens_kde_singular")
        return int(n.value)

    def nuts_counts(self, reset=False):
        """alabi_ens_nuts_stats: (counts [E W, 3] int64 -- leaves, depths reached, divergent transitions --, the sum of the leaves'
        acceptance statistics [E W]) per walker since the handle's last reset."""
        counts = np.zeros((self.total_walkers, 3), dtype=np.int64)
        acc = np.zeros(self.total_walkers, dtype=np.float64)
        if getattr(self, "_ens", None) is not None:
            _lib.check(_lib.lib().alabi_ens_nuts_stats(self._ens, C.c_void_p(counts.ctypes.data), C.c_void_p(acc.ctypes.data), int(bool(reset))),
                       "alabi_ens_nuts_stats")
        if reset:
            self._nuts_transitions = 0
        return counts, acc

    @property
    def nuts_stats(self):
        """What the NUTS transitions of this sampler's handle did since its last reset (None without a ``NUTSMove``):
        ``transitions``, ``mean_depth`` (completed doublings per transition), ``leaves_per_transition`` (gradient evaluations),
        ``divergences`` and ``mean_accept_stat`` (the mean over all leaves of min(1, exp(-energy error)), 0 outside the box)."""
        if self._move_set is None or not self._move_set.all_nuts:
            return None
        counts, acc = self.nuts_counts()
        n = int(getattr(self, "_nuts_transitions", 0))
        leaves = int(counts[:, 0].sum())
        return dict(transitions=n, mean_depth=float(counts[:, 1].sum()) / max(n, 1), leaves_per_transition=leaves / max(n, 1),
                    divergences=int(counts[:, 2].sum()), mean_accept_stat=float(acc.sum()) / max(leaves, 1))

    def _release(self):
        _lib.destroy(getattr(self, "_ens", None), "alabi_ens_destroy", sync=True)
        self._ens = None
        self._ens_gp_handle = None

    def __del__(self):
        self._release()

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_ens"] = None
        st["_ens_gp_handle"] = None
        st["_stream"] = None
        st["_sharded"] = None
        st["_sharded_ens"] = None
        st["group"] = None
        st["prior_fn_host"] = None      # host callables (often closures) are not part of the saved state
        st["like_fn_host"] = None
        st["_last_window_chain"] = None    # tune_hmc's scratch chain of its last window (device)
        for k in ("_coords", "_logp", "_naccept"):
            st[k] = None if st[k] is None else st[k].cpu()
        st["_chains"] = [c.cpu() for c in self._chains]
        st["_chain_lps"] = [c.cpu() for c in self._chain_lps]
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        if "_rng_step" not in st:                       # saved before the draw counter was separated from `iteration`
            self._rng_step = st.get("iteration", 0)
        self.__dict__.setdefault("_move_set", None)     # saved before the sampler had moves
        if torch.cuda.is_available():
            self._stream = torch.cuda.Stream()
            for k in ("_coords", "_logp", "_naccept"):
                if getattr(self, k) is not None:
                    setattr(self, k, getattr(self, k).to(_dev()))

    # ------------------------------------------------------------------------- sampling
    def compute_log_prob(self, coords):
        """Surrogate mean + box prior for an ensemble of points (device in, device out)."""
        self._ensure_ens()
        c = _to_dev(coords, 2)
        if c.shape != (self.total_walkers, self.ndim):
            raise ValueError("coords must have shape (nwalkers * n_ensembles, ndim)")
        lp = torch.empty(self.total_walkers, dtype=torch.float64, device=c.device)
        if self.generic:
            return self._host_log_prob(c, self.surrogate(c) if self.like_fn_host is None else None)
        _lib.check(_lib.lib().alabi_ens_lnprob(self._ens, _lib.ptr(c), _lib.ptr(lp), _lib.current_stream()), "alabi_ens_lnprob")
        return lp

    def log_prob_grad(self, coords):
        """The fused log-probability and its gradient with respect to the coordinates at arbitrary points [M, d] (device
        tensors (logp [M], grad [M, d])): what an ``HMCMove`` integrates -- GP mean through the scalers, the y map, normal priors;
        -inf and a zero gradient outside the box.  Needs the fused log-probability (no host callables)."""
        if self.generic:
            raise ValueError("log_prob_grad needs the fused log-probability: host callables (prior_fn / like_fn) have no gradient")
        self._ensure_ens()
        c = _to_dev(coords, 2)
        if c.ndim != 2 or c.shape[1] != self.ndim:
            raise ValueError("coords must have shape (M, ndim)")
        lp = torch.empty(c.shape[0], dtype=torch.float64, device=c.device)
        g = torch.empty((c.shape[0], self.ndim), dtype=torch.float64, device=c.device)
        _lib.check(_lib.lib().alabi_ens_log_prob_grad(self._ens, _lib.ptr(c), int(c.shape[0]), _lib.ptr(lp), _lib.ptr(g),
                                                      _lib.current_stream()), "alabi_ens_log_prob_grad")
        return lp, g

    def maximize(self, starts, maxiter=200, gtol=1e-8, trace=0):
        """Maxima of the fused log-probability inside the box from ``starts`` [S, d] (any S >= 1, no relation to ``nwalkers``):
        a projected BFGS ascent on the closed-form gradient, one workgroup per start and every iteration of every search in ONE
        launch (``ens_map_kernel``).  Returns a ``MaximizeResult`` of device tensors: ``x`` [S, d], ``log_prob`` [S],
        ``iterations`` / ``evaluations`` / ``status`` [S] (int32) and ``grad_norm`` [S], the largest component of the projected
        gradient.  status 0: ``grad_norm <= gtol``; 1: ``maxiter`` iterations taken; 2: no ascent at the smallest step (the best
        point is kept); 3: the start lies outside the open box or the log-probability is not finite there (NaN outputs).  The
        search runs on the box shrunk by 1e-9 of its width; a coordinate held on a bound ends exactly on that shrunk wall.  The
        result is never worse than the start.  ``trace=n`` adds ``trace`` (the raw [S, n, 4] record) and its columns ``trace_log_prob``, ``trace_step`` [S, n] (NaN beyond the last
        iteration), ``trace_held`` (int64 bit masks) and ``trace_updated`` (bool) of the first n accepted iterations.  Needs the
        fused log-probability (no host callables)."""
        if self.generic:
            raise ValueError("maximize needs the fused log-probability: host callables (prior_fn / like_fn) have no gradient")
        self._ensure_ens()
        c = _to_dev(starts, 2)
        if c.ndim != 2 or c.shape[1] != self.ndim or c.shape[0] < 1:
            raise ValueError("starts must have shape (S, ndim) with S >= 1")
        maxiter, ntrace, gtol = int(maxiter), int(trace), float(gtol)
        if maxiter < 0 or ntrace < 0 or not gtol >= 0.0:
            raise ValueError("maxiter and trace must not be negative, nor gtol")
        S, dev = int(c.shape[0]), c.device
        res = MaximizeResult()
        res.x = torch.empty((S, self.ndim), dtype=torch.float64, device=dev)
        res.log_prob = torch.empty(S, dtype=torch.float64, device=dev)
        res.grad_norm = torch.empty(S, dtype=torch.float64, device=dev)
        res.status = torch.empty(S, dtype=torch.int32, device=dev)
        iters = torch.empty((S, 2), dtype=torch.int32, device=dev)
        tr = torch.full((S, ntrace, 4), float("nan"), dtype=torch.float64, device=dev) if ntrace else None
        _lib.check(_lib.lib().alabi_ens_maximize(self._ens, _lib.ptr(c), S, maxiter, gtol, _lib.ptr(res.x), _lib.ptr(res.log_prob),
                                                 _lib.ptr(iters), _lib.ptr(res.status), _lib.ptr(res.grad_norm), _lib.ptr(tr), ntrace,
                                                 _lib.current_stream()), "alabi_ens_maximize")
        res.iterations, res.evaluations = iters[:, 0], iters[:, 1]
        if ntrace:
            res.trace = tr
            done = ~torch.isnan(tr[:, :, 1])
            res.trace_log_prob, res.trace_step = tr[:, :, 0], tr[:, :, 1]
            res.trace_held = torch.where(done, tr[:, :, 2].contiguous().view(torch.int64), torch.zeros_like(done, dtype=torch.int64))
            res.trace_updated = done & (tr[:, :, 3] == 1.0)
        return res

    def log_prob_hessian(self, coords):
        """The Hessian of the fused log-probability with respect to the coordinates at arbitrary points [M, d]: a device tensor
        [M, d, d], symmetric to the bit, closed form (the second derivatives of the GP mean through the scalers, the y map's
        chain rule, minus 1 / s_k^2 per normal-prior coordinate); NaN outside the open box.  At ``maximize``'s optimum, minus its
        inverse is the covariance an ``HMCMove`` or ``GaussianMove`` wants (``alabi_amd.laplace``).  Needs the fused
        log-probability (no host callables)."""
        if self.generic:
            raise ValueError("log_prob_hessian needs the fused log-probability: host callables (prior_fn / like_fn) have no gradient")
        self._ensure_ens()
        c = _to_dev(coords, 2)
        if c.ndim != 2 or c.shape[1] != self.ndim:
            raise ValueError("coords must have shape (M, ndim)")
        H = torch.empty((c.shape[0], self.ndim, self.ndim), dtype=torch.float64, device=c.device)
        _lib.check(_lib.lib().alabi_ens_log_prob_hessian(self._ens, _lib.ptr(c), int(c.shape[0]), _lib.ptr(H), _lib.current_stream()),
                   "alabi_ens_log_prob_hessian")
        return H

    def surrogate(self, points):
        """y_scaler^-1(GP mean) at arbitrary points [M,d] in the sampler's coordinates: no box gate, no prior (device tensor)."""
        self._ensure_ens()
        c = _to_dev(points, 2)
        out = torch.empty(c.shape[0], dtype=torch.float64, device=c.device)
        _lib.check(_lib.lib().alabi_ens_surrogate(self._ens, _lib.ptr(c), int(c.shape[0]), _lib.ptr(out), _lib.current_stream()),
                   "alabi_ens_surrogate")
        return out

    def _host_log_prob(self, q_dev, like_dev):
        """like (device values, or like_fn on the host) + prior_fn on the host for a batch of points; device tensor out.
        NaN raises as emcee does ("Probability function returned NaN")."""
        qh = q_dev.cpu().numpy()
        if like_dev is not None:
            lp = like_dev.cpu().numpy().copy()
        elif self.gate_box:                          # a host likelihood under the box prior: only evaluated inside the box
            inside = np.all((qh > self.bounds[:, 0]) & (qh < self.bounds[:, 1]), axis=1)
            lp = np.full(qh.shape[0], -np.inf)
            if inside.any():
                lp[inside] = np.asarray(self.like_fn_host(qh[inside]), dtype=np.float64).reshape(-1)
        else:
            lp = np.asarray(self.like_fn_host(qh), dtype=np.float64).reshape(-1).copy()
        if self.prior_fn_host is not None:
            lp = lp + np.asarray(self.prior_fn_host(qh), dtype=np.float64).reshape(-1)
        if lp.shape != (qh.shape[0],):
            raise ValueError("like_fn / prior_fn must return one value per point")
        if np.any(np.isnan(lp)):
            raise ValueError("Probability function returned NaN")
        return torch.as_tensor(lp, device=q_dev.device)

    def _run_generic(self, nsteps, thin_by, chain, chain_lp):
        """Half steps split around the host callables (alabi_ens_propose -> host -> alabi_ens_accept)."""
        lib, W, d = _lib.lib(), self.nwalkers, self.ndim
        n0 = (W + 1) // 2
        dev = self._coords.device
        stream = _lib.current_stream()
        want_like = self.like_fn_host is None
        if self.prior_fn_host is None and self.like_fn_host is None:
            raise RuntimeError("this sampler was set up with host callables (prior_fn / like_fn) that are not part of its "
                               "saved state: create a new sampler with them")
        # steps per draw: at most the library's draw-buffer chunk (4M / walkers, between 16 and 1024 steps)
        cap = max(16, min(1024, (4 << 20) // max(self.total_walkers, 1)))
        done = 0
        while done < nsteps:
            n = min(256, cap, nsteps - done)
            _lib.check(lib.alabi_ens_draw(self._ens, self._rng_step + done, n, self.a, stream), "alabi_ens_draw")
            for t in range(n):
                for split in (0, 1):
                    nS = n0 if split == 0 else W - n0
                    if nS == 0:
                        continue
                    q = torch.empty((nS, d), dtype=torch.float64, device=dev)
                    like = torch.empty(nS, dtype=torch.float64, device=dev) if want_like else None
                    _lib.check(lib.alabi_ens_propose(self._ens, _lib.ptr(self._coords), t, split, int(self.gate_box),
                                                     _lib.ptr(q), _lib.ptr(like), stream), "alabi_ens_propose")
                    lp_new = self._host_log_prob(q, like)
                    _lib.check(lib.alabi_ens_accept(self._ens, _lib.ptr(self._coords), _lib.ptr(self._logp), t, split,
                                                    _lib.ptr(q), _lib.ptr(lp_new), _lib.ptr(self._naccept), stream),
                               "alabi_ens_accept")
                k = done + t + 1
                if chain is not None and k % thin_by == 0:
                    chain[k // thin_by - 1].copy_(self._coords)
                    chain_lp[k // thin_by - 1].copy_(self._logp)
            done += n
        torch.cuda.current_stream().synchronize()

    def _run_mh(self, nsteps, thin_by, chain, chain_lp):
        """The host loop of an all-MHMove set: per step one move is drawn from the weights, the walkers travel to the host, the
        move's proposal function makes q and its log factors, the log-probability of q is evaluated on the device (or through
        the host callables) and a proposal is accepted where log(rng.rand(W)) < lp' - lp + lf.  One round trip per step."""
        ms, W, d = self._move_set, self.nwalkers, self.ndim
        if getattr(self, "_mh_rng", None) is None:
            self._mh_rng = np.random.RandomState(self.seed & 0xFFFFFFFF)
        rng = self._mh_rng
        dev = self._coords.device
        x = self._coords.cpu().numpy()
        lp = self._logp.cpu().numpy()
        nacc = np.zeros(W, dtype=np.int64)
        for t in range(nsteps):
            move = ms.moves[int(rng.choice(len(ms.moves), p=ms.weights))] if len(ms.moves) > 1 else ms.moves[0]
            q, lf = move.get_proposal(x, rng)
            q = np.asarray(q, dtype=np.float64)
            lf = np.asarray(lf, dtype=np.float64)
            if q.shape != (W, d) or lf.shape != (W,):
                raise ValueError(f"an MHMove's proposal function must return (q[{W}, {d}], log_factors[{W}]), got shapes "
                                 f"{q.shape} and {lf.shape}")
            lpq = self.compute_log_prob(torch.as_tensor(np.ascontiguousarray(q), device=dev)).cpu().numpy()
            if np.any(np.isnan(lpq)):
                raise ValueError("Probability function returned NaN")
            with np.errstate(invalid="ignore"):
                acc = np.log(rng.rand(W)) < lpq - lp + lf
            x = np.where(acc[:, None], q, x)
            lp = np.where(acc, lpq, lp)
            nacc += acc
            k = t + 1
            if chain is not None and k % thin_by == 0:
                chain[k // thin_by - 1].copy_(torch.as_tensor(x, device=dev))
                chain_lp[k // thin_by - 1].copy_(torch.as_tensor(lp, device=dev))
        self._coords = torch.as_tensor(np.ascontiguousarray(x), device=dev)
        self._logp = torch.as_tensor(np.ascontiguousarray(lp), device=dev)
        self._naccept += torch.as_tensor(nacc, device=dev)
        torch.cuda.current_stream().synchronize()

    def run_mcmc(self, initial_state, nsteps, thin_by=1, progress=False, store=True, skip_initial_state_check=False, **kw):
        nsteps = int(nsteps)
        thin_by = int(thin_by)
        if thin_by < 1:
            raise ValueError("thin_by must be a positive integer")
        if initial_state is None:
            if self._coords is None:
                raise ValueError("Cannot have `initial_state=None` if run_mcmc has never been called.")
        else:
            coords = initial_state.coords if isinstance(initial_state, State) else initial_state
            coords = _to_dev(coords, 2).clone()
            if coords.shape != (self.total_walkers, self.ndim):
                raise ValueError("incompatible input dimensions: initial state must be (nwalkers * n_ensembles, ndim)")
            if not skip_initial_state_check and self.nwalkers > 1:
                c = coords.cpu().numpy()
                c = c - c.mean(axis=0)
                smax = np.abs(c).max(axis=0)
                if np.any(smax == 0):
                    raise ValueError("Initial state has a large condition number. Make sure that your walkers are "
                                     "linearly independent for the best performance")
                if np.linalg.cond((c / smax).astype(float)) > 1e8:
                    raise ValueError("Initial state has a large condition number. Make sure that your walkers are "
                                     "linearly independent for the best performance")
            self._coords = coords
            self._logp = self.compute_log_prob(coords)
            if torch.isnan(self._logp).any():
                raise ValueError("The initial log_prob was NaN")
        self._ensure_ens()
        if self.shard:
            from .dist import ShardedRun, world_info
            if world_info(self.group)[1] > 1:
                t0s = time.perf_counter()
                nstore = nsteps // thin_by if store else 0
                if self._sharded is None or self._sharded.s is not self or self._sharded_ens is not self._ens:
                    self._sharded, self._sharded_ens = ShardedRun(self, self.group), self._ens
                ch, co, lp, nacc = self._sharded.run(self._coords, nsteps, step0=self._rng_step, a=self.a, thin_by=thin_by,
                                                     store=bool(nstore), logp0=self._logp)
                torch.cuda.current_stream().synchronize()
                self._coords, self._logp = co, lp
                self._naccept += nacc
                self.last_path = "sharded"
                self.last_run_seconds = time.perf_counter() - t0s
                self.iteration += nsteps
                self._rng_step += nsteps
                if nstore:
                    self._chains.append(ch); self._chain_lps.append(self._sharded.last_chain_logp); self._thins.append(thin_by)
                return State(self._coords.cpu().numpy(), self._logp.cpu().numpy())
        nstore = nsteps // thin_by if store else 0
        dev = self._coords.device
        chain = torch.empty((nstore, self.total_walkers, self.ndim), dtype=torch.float64, device=dev) if nstore else None
        chain_lp = torch.empty((nstore, self.total_walkers), dtype=torch.float64, device=dev) if nstore else None
        t0 = time.perf_counter()
        mh = self._move_set is not None and self._move_set.all_mh
        if self.generic or mh:
            if mh:
                self._run_mh(nsteps, thin_by, chain, chain_lp)
            else:
                self._run_generic(nsteps, thin_by, chain, chain_lp)
            self.last_path = "host-mh" if mh else "host-callback"
            self.last_run_seconds = time.perf_counter() - t0
            self.iteration += nsteps
            self._rng_step += nsteps
            if nstore:
                self._chains.append(chain); self._chain_lps.append(chain_lp); self._thins.append(thin_by)
            return State(self._coords.cpu().numpy(), self._logp.cpu().numpy())
        # no backup here: a persistent call saves (coords, logp, n_accept) itself, in the launch in front of its first kernel
        self._stream.wait_stream(torch.cuda.current_stream())

        def _run():
            with torch.cuda.stream(self._stream):
                return _lib.lib().alabi_ens_run(self._ens, _lib.ptr(self._coords), _lib.ptr(self._logp), self._rng_step,
                                                nsteps, thin_by, self.a, _lib.ptr(chain), _lib.ptr(chain_lp),
                                                _lib.ptr(self._naccept), C.c_void_p(self._stream.cuda_stream))

        st = _run()
        if st == _lib.TIMEOUT:
            # the persistent kernel gave up on a hand-off (e.g. the GPU was shared and its workgroups were not all
            # resident): restore the state and repeat the run with one launch per half step
            self._stream.synchronize()
            _lib.check(_lib.lib().alabi_ens_restore(self._ens, _lib.ptr(self._coords), _lib.ptr(self._logp), _lib.ptr(self._naccept),
                                                    C.c_void_p(self._stream.cuda_stream)), "alabi_ens_restore")
            _lib.check(_lib.lib().alabi_ens_set_stream(self._ens, 0), "alabi_ens_set_stream")
            self.stream_fallbacks = getattr(self, "stream_fallbacks", 0) + 1
            st = _run()
        _lib.check(st, "alabi_ens_run")
        path = C.c_int(0)
        _lib.lib().alabi_ens_last_path(self._ens, C.byref(path))
        self.last_path = {1: "stream", 3: "group", 4: "metropolis", 5: "hmc", 6: "nuts"}.get(path.value, "launch-per-half-step")
        self.last_stream_kernel = {1: "ens_stream_kernel", 3: "ens_group_kernel", 4: "ens_mh_kernel", 5: "ens_hmc_kernel",
                                   6: "ens_nuts_kernel"}.get(path.value)
        if path.value == 6:
            self._nuts_transitions = getattr(self, "_nuts_transitions", 0) + nsteps * self.total_walkers
        variant = C.c_int(0)                                  # path 1: one workgroup per list position, or a pair of them
        _lib.lib().alabi_ens_stream_variant(self._ens, C.byref(variant))
        self.last_stream_variant = {0: "single", 1: "pair"}[variant.value] if path.value == 1 else None
        self.group_plan = None
        if path.value == 3:                                   # which instantiation of ens_group_kernel ran (tests pin it)
            plan = (C.c_int * 8)()
            _lib.lib().alabi_ens_group_plan(self._ens, plan)
            self.group_plan = dict(zip(("Q", "G", "NG", "RT", "tpm", "ltw", "KS", "lds_bytes"), (int(v) for v in plan)))
        self._stream.synchronize()
        torch.cuda.current_stream().wait_stream(self._stream)
        self.last_run_seconds = time.perf_counter() - t0
        self.iteration += nsteps
        self._rng_step += nsteps
        if nstore:
            self._chains.append(chain)
            self._chain_lps.append(chain_lp)
            self._thins.append(thin_by)
        if path.value == 1:
            # the persistent call has read the walkers back with its time-out flag: no further copy, no synchronisation
            c = np.empty((self.total_walkers, self.ndim), dtype=np.float64)
            lp = np.empty(self.total_walkers, dtype=np.float64)
            _lib.check(_lib.lib().alabi_ens_last_state(self._ens, C.c_void_p(c.ctypes.data), C.c_void_p(lp.ctypes.data)),
                       "alabi_ens_last_state")
            return State(c, lp)
        return State(self._coords.cpu().numpy(), self._logp.cpu().numpy())

    def _hmc_adapt(self, nsteps, state, par, chain=None, accept_stat=None):
        """``nsteps`` warm-up steps of the walkers on ens_hmc_adapt_kernel (alabi_ens_hmc_adapt) from the draw counter, which
        advances; ``state`` [E W, 5] is the dual-averaging state (device, in / out), ``par`` (delta, gamma, t0, kappa)."""
        _lib.check(_lib.lib().alabi_ens_hmc_adapt(self._ens, _lib.ptr(self._coords), _lib.ptr(self._logp), self._rng_step, int(nsteps), 1,
                                                  _lib.ptr(state), _lib.host_doubles(par), _lib.ptr(chain), None, None,
                                                  _lib.ptr(accept_stat), _lib.current_stream()), "alabi_ens_hmc_adapt")
        self._rng_step += int(nsteps)

    def tune_hmc(self, initial_state, nwarmup=500, target_accept=0.8, metric="diag", gamma=0.05, t0=10, kappa=0.75):
        """Stan-style warm-up of the sampler's one ``HMCMove``: the step size by dual averaging per walker (Hoffman & Gelman 2014,
        algorithm 5, towards a mean acceptance statistic of ``target_accept``) on ``ens_hmc_adapt_kernel``, and, with ``metric``
        "diag" or "dense", the mass matrix from the pooled covariance of the walkers' positions in Stan's doubling windows
        (``alabi_amd.hmc_adapt``: an initial buffer, the windows, a terminal buffer; every one of them is ONE library call).
        ``metric=None`` adapts the step size only.  Dual averaging starts at the move's resolved step size e with mu = ln(10 e); at
        a window's end the new factor is installed and every walker restarts at the pooled step size.  Afterwards the sampler's move
        is ``HMCMove(cov, step_size)`` with what was found (``n_leapfrog`` and ``jitter`` kept), the library's table holds it, and
        ``hmc_tuning`` says what happened: ``step_size``, ``cov`` (None where the mass was not adapted), ``window_ends``,
        ``step_sizes`` (the pooled step size at every window's end), ``mean_accept_stat`` of the terminal buffer and ``last_path ==
        "hmc-adapt"``.  The warm-up steps consume the draw counter like ``run_mcmc``'s but are no part of the chain, of ``iteration``
        or of the acceptance counts.  Returns the ``State`` to continue from (``run_mcmc(None, n)`` continues there too).  A set
        that is not exactly one ``HMCMove``, host callables and ``shard=True`` raise ``ValueError``."""
        from . import hmc_adapt as ha
        from .moves import HMCMove
        if self._move_set is not None and self._move_set.has_nuts:
            raise ValueError("tune_hmc adapts an HMCMove, not a NUTSMove: a NUTSMove has tune_nuts (run_emcee: nuts_warmup).  The older "
                             "route still works -- tune an HMCMove with the same "
                             'cov, then pass NUTSMove(sm.hmc_tuning["cov"], step_size=sm.hmc_tuning["step_size"]) (hmc_tuning of the sampler, or of '
                             "the SurrogateModel after run_emcee with hmc_warmup)")
        if self.generic:
            raise ValueError("tune_hmc needs the gradient of the log-probability, which exists for the fused surrogate only: a Python "
                             "prior_fn or like_fn (the host-callback path) has none")
        if self.shard:
            raise ValueError("tune_hmc cannot run with shard=True: the sharded form of an HMCMove is not built")
        ms = self._move_set
        if ms is None or len(ms) != 1 or not isinstance(ms.moves[0], HMCMove):
            raise ValueError("tune_hmc adapts the step size and the mass matrix of exactly one HMCMove: mixtures of HMC moves under "
                             "adaptation are not built, and no other move has a step size to adapt")
        if metric not in (None, "diag", "dense"):
            raise ValueError("metric must be None, 'diag' or 'dense'")
        nwarmup = int(nwarmup)
        par = (float(target_accept), float(gamma), float(t0), float(kappa))
        if nwarmup < 1 or not (0.0 < par[0] < 1.0) or not par[1] > 0.0 or not par[2] >= 0.0 or not (0.5 < par[3] <= 1.0):
            raise ValueError("tune_hmc needs nwarmup >= 1, 0 < target_accept < 1, gamma > 0, t0 >= 0 and 0.5 < kappa <= 1")
        move = ms.moves[0]
        t_start = time.perf_counter()
        coords = initial_state.coords if isinstance(initial_state, State) else initial_state
        coords = _to_dev(coords, 2).clone()
        if coords.shape != (self.total_walkers, self.ndim):
            raise ValueError("incompatible input dimensions: initial state must be (nwalkers * n_ensembles, ndim)")
        self._coords = coords
        self._logp = self.compute_log_prob(coords)
        if torch.isnan(self._logp).any():
            raise ValueError("The initial log_prob was NaN")
        self._ensure_ens()
        dev, WT = coords.device, self.total_walkers
        state = torch.as_tensor(ha.initial_state(WT, move.resolved_step_size(self.ndim)), device=dev)
        segments = ha.warmup_segments(nwarmup, windows=metric is not None)
        cov, step_sizes, window_ends, stat = None, [], [], None
        for k, (first, end, is_window) in enumerate(segments):
            n = end - first
            scratch = torch.empty((n, WT, self.ndim), dtype=torch.float64, device=dev) if is_window else None
            last = k == len(segments) - 1
            stat = torch.zeros(WT, dtype=torch.float64, device=dev) if last else None
            self._hmc_adapt(n, state, par, chain=scratch, accept_stat=stat)
            if is_window:
                torch.cuda.current_stream().synchronize()
                cov = ha.regularised_covariance(scratch.reshape(-1, self.ndim), metric)
                move = HMCMove(cov, step_size=move.resolved_step_size(self.ndim), n_leapfrog=move.n_leapfrog, jitter=move.jitter)
                _lib.check(_lib.lib().alabi_ens_set_move_scale(self._ens, 0, _lib.host_doubles(move.scale_matrix(self.ndim).ravel()),
                                                               int(move.diagonal)), "alabi_ens_set_move_scale")
                pooled = ha.pooled_step_size(state[:, 3])
                step_sizes.append(pooled); window_ends.append(end)
                self._last_window_chain = scratch
                if not last:
                    state.copy_(torch.as_tensor(ha.restart_state(WT, pooled), device=dev))
        torch.cuda.current_stream().synchronize()
        eps = ha.pooled_step_size(state[:, 3])
        move = HMCMove(move.cov, step_size=eps, n_leapfrog=move.n_leapfrog, jitter=move.jitter)
        self._move_set = parse_moves(move, self.ndim)
        m = self._move_set
        _lib.check(_lib.lib().alabi_ens_set_move_scale(self._ens, 0, _lib.host_doubles(move.scale_matrix(self.ndim).ravel()),
                                                       int(move.diagonal)), "alabi_ens_set_move_scale")
        _lib.check(_lib.lib().alabi_ens_set_moves(self._ens, 1, (C.c_int * 1)(int(m.kind[0])), _lib.host_doubles(m.cum),
                                                  _lib.host_doubles(m.p0), _lib.host_doubles(m.p1)), "alabi_ens_set_moves")
        n_last = segments[-1][1] - segments[-1][0]
        self.hmc_tuning = dict(step_size=eps, cov=None if cov is None else np.array(cov, copy=True), window_ends=window_ends,
                               step_sizes=step_sizes, mean_accept_stat=float(stat.mean().item()) / n_last, nwarmup=nwarmup,
                               metric=metric, seconds=time.perf_counter() - t_start, last_path="hmc-adapt")
        self.last_path = "hmc-adapt"
        self.last_stream_kernel = "ens_hmc_adapt_kernel"
        return State(self._coords.cpu().numpy(), self._logp.cpu().numpy())

    # ------------------------------------------------------------------ NUTS warm-up
    def _grad_route_checks(self, route, cls, what):
        """The refusals that ``tune_nuts`` shares with ``tune_hmc``, mirrored; returns the one move."""
        if self.generic:
            raise ValueError(f"{route} needs the gradient of the log-probability, which exists for the fused surrogate only: a Python "
                             "prior_fn or like_fn (the host-callback path) has none")
        if self.shard:
            raise ValueError(f"{route} cannot run with shard=True: the sharded form of a {cls.__name__} is not built")
        ms = self._move_set
        if ms is None or len(ms) != 1 or not isinstance(ms.moves[0], cls):
            raise ValueError(f"{route} {what} of exactly one {cls.__name__}: mixtures under adaptation are not built, and no other "
                             "move has a step size to adapt" + (" (an HMCMove has tune_hmc)" if ms is not None and ms.has_hmc else ""))
        return ms.moves[0]

    def _search_ln_e(self, ln_e, k_move=0):
        """alabi_ens_find_step_size on the current walkers at the current draw counter (which does not advance): ``ln_e`` [E W]
        (device, in / out); returns the iteration counts (device, int32)."""
        iters = torch.zeros(self.total_walkers, dtype=torch.int32, device=ln_e.device)
        _lib.check(_lib.lib().alabi_ens_find_step_size(self._ens, _lib.ptr(self._coords), _lib.ptr(self._logp), self._rng_step, int(k_move),
                                                       _lib.ptr(ln_e), _lib.ptr(iters), _lib.current_stream()), "alabi_ens_find_step_size")
        return iters

    def find_step_size(self, coords=None, k_move=0):
        """Stan's initial step-size search for move ``k_move`` of a set of HMC moves or of NUTS moves, on ``ens_step_search_kernel``:
        per walker, from the move's resolved step size, one leapfrog step with a fresh momentum per iteration, the step size doubled
        (or halved) until the step's energy error crosses ln 0.8 -- at most 40 times.  ``coords`` [E W, ndim] (default: where the
        sampler stands) are not moved, and the draw counter does not advance.  Returns a dict: ``step_sizes`` [E W], ``step_size``
        (their geometric mean) and ``iters`` [E W] (the doublings or halvings made; 40: the cap was hit).  Any other move set, host
        callables and ``shard=True`` raise ``ValueError``."""
        from . import hmc_adapt as ha
        if self.generic:
            raise ValueError("find_step_size needs the gradient of the log-probability, which exists for the fused surrogate only: a "
                             "Python prior_fn or like_fn (the host-callback path) has none")
        if self.shard:
            raise ValueError("find_step_size cannot run with shard=True: the sharded form of an HMCMove or a NUTSMove is not built")
        ms = self._move_set
        if ms is None or not (ms.all_hmc or ms.all_nuts):
            raise ValueError("find_step_size searches the step size of an HMCMove or a NUTSMove: the move set must consist of HMC moves "
                             "or of NUTS moves")
        k_move = int(k_move)
        if not 0 <= k_move < len(ms):
            raise ValueError(f"find_step_size: k_move must be in 0 ... {len(ms) - 1}")
        if coords is None:
            if self._coords is None:
                raise ValueError("find_step_size needs coords before the sampler has run")
        else:
            c = _to_dev(coords.coords if isinstance(coords, State) else coords, 2).clone()
            if c.shape != (self.total_walkers, self.ndim):
                raise ValueError("incompatible input dimensions: coords must be (nwalkers * n_ensembles, ndim)")
            self._coords, self._logp = c, self.compute_log_prob(c)
        self._ensure_ens()
        ln_e = torch.full((self.total_walkers,), float(np.log(ms.moves[k_move].resolved_step_size(self.ndim))), dtype=torch.float64,
                          device=self._coords.device)
        iters = self._search_ln_e(ln_e, k_move)
        torch.cuda.current_stream().synchronize()
        return dict(step_sizes=np.exp(ln_e.cpu().numpy()), step_size=ha.pooled_step_size(ln_e), iters=iters.cpu().numpy())

    def _nuts_adapt(self, nsteps, state, par, counts, accept_sum, chain=None, accept_stat=None):
        """``nsteps`` warm-up transitions on ens_nuts_adapt_kernel (alabi_ens_nuts_adapt) from the draw counter, which advances;
        ``state`` [E W, 5] as ``_hmc_adapt``; ``counts`` [E W, 3] int64 and ``accept_sum`` [E W] take the transitions' sums."""
        _lib.check(_lib.lib().alabi_ens_nuts_adapt(self._ens, _lib.ptr(self._coords), _lib.ptr(self._logp), self._rng_step, int(nsteps), 1,
                                                   _lib.ptr(state), _lib.host_doubles(par), _lib.ptr(chain), None, None, _lib.ptr(counts),
                                                   _lib.ptr(accept_sum), _lib.ptr(accept_stat), _lib.current_stream()), "alabi_ens_nuts_adapt")
        self._rng_step += int(nsteps)

    def tune_nuts(self, initial_state, nwarmup=500, target_accept=0.8, metric="diag", init_step_size="search", gamma=0.05, t0=10,
                  kappa=0.75):
        """Stan-style warm-up of the sampler's one ``NUTSMove``, ``tune_hmc``'s structure on NUTS's own statistic: the step size by
        dual averaging per walker towards a mean of ``target_accept`` of a_t -- the mean over ALL leaves of a transition's tree of
        min(1, exp(-energy error)), 0 outside the box and for a divergent leaf -- on ``ens_nuts_adapt_kernel``, and, with ``metric``
        "diag" or "dense", the mass matrix from the pooled covariance of the walkers' positions in Stan's doubling windows
        (``alabi_amd.hmc_adapt``; every segment is ONE library call).  ``init_step_size="search"`` runs Stan's step-size search
        (``find_step_size``) before the first segment and again after every mass-matrix update, and every walker restarts from its own
        searched value; ``None`` starts at the move's resolved step size and restarts at the pooled one, exactly as ``tune_hmc``.
        Afterwards the sampler's move is ``NUTSMove(cov, step_size=pooled, max_depth, jitter)``, the library's table holds it, and
        ``nuts_tuning`` says what happened: ``step_size``, ``cov`` (None where the mass was not adapted), ``window_ends``,
        ``step_sizes`` (pooled, at every window's end), ``mean_accept_stat``, ``mean_depth`` and ``divergences`` of the terminal
        buffer, ``search_iters`` (per search, the walkers' iteration counts), ``nwarmup``, ``metric``, ``seconds`` and ``last_path ==
        "nuts-adapt"``.  Warm-up consumes the draw counter like ``run_mcmc`` but is no part of the chain, of ``iteration``, of the
        acceptance counts or of ``nuts_stats``.  Returns the ``State`` to continue from.  A set that is not exactly one ``NUTSMove``,
        host callables and ``shard=True`` raise ``ValueError``."""
        from . import hmc_adapt as ha
        from .moves import NUTSMove
        move = self._grad_route_checks("tune_nuts", NUTSMove, "adapts the step size and the mass matrix")
        if metric not in (None, "diag", "dense"):
            raise ValueError("metric must be None, 'diag' or 'dense'")
        if init_step_size not in (None, "search"):
            raise ValueError("init_step_size must be 'search' or None")
        nwarmup = int(nwarmup)
        par = (float(target_accept), float(gamma), float(t0), float(kappa))
        if nwarmup < 1 or not (0.0 < par[0] < 1.0) or not par[1] > 0.0 or not par[2] >= 0.0 or not (0.5 < par[3] <= 1.0):
            raise ValueError("tune_nuts needs nwarmup >= 1, 0 < target_accept < 1, gamma > 0, t0 >= 0 and 0.5 < kappa <= 1")
        search = init_step_size == "search"
        t_start = time.perf_counter()
        coords = initial_state.coords if isinstance(initial_state, State) else initial_state
        coords = _to_dev(coords, 2).clone()
        if coords.shape != (self.total_walkers, self.ndim):
            raise ValueError("incompatible input dimensions: initial state must be (nwalkers * n_ensembles, ndim)")
        self._coords = coords
        self._logp = self.compute_log_prob(coords)
        if torch.isnan(self._logp).any():
            raise ValueError("The initial log_prob was NaN")
        self._ensure_ens()
        dev, WT = coords.device, self.total_walkers
        search_iters = []

        def searched(eps):
            ln_e = torch.full((WT,), float(np.log(eps)), dtype=torch.float64, device=dev)
            iters = self._search_ln_e(ln_e)
            search_iters.append(iters.cpu().numpy())
            return torch.as_tensor(ha.searched_state(ln_e), device=dev)

        eps0 = move.resolved_step_size(self.ndim)
        state = searched(eps0) if search else torch.as_tensor(ha.initial_state(WT, eps0), device=dev)
        segments = ha.warmup_segments(nwarmup, windows=metric is not None)
        cov, step_sizes, window_ends, stat, counts = None, [], [], None, None
        for k, (first, end, is_window) in enumerate(segments):
            n = end - first
            scratch = torch.empty((n, WT, self.ndim), dtype=torch.float64, device=dev) if is_window else None
            last = k == len(segments) - 1
            counts = torch.zeros((WT, 3), dtype=torch.int64, device=dev)
            leaf_sum = torch.zeros(WT, dtype=torch.float64, device=dev)
            stat = torch.zeros(WT, dtype=torch.float64, device=dev) if last else None
            self._nuts_adapt(n, state, par, counts, leaf_sum, chain=scratch, accept_stat=stat)
            if is_window:
                torch.cuda.current_stream().synchronize()
                cov = ha.regularised_covariance(scratch.reshape(-1, self.ndim), metric)
                move = NUTSMove(cov, step_size=eps0, max_depth=move.max_depth, jitter=move.jitter)
                _lib.check(_lib.lib().alabi_ens_set_move_scale(self._ens, 0, _lib.host_doubles(move.scale_matrix(self.ndim).ravel()),
                                                               int(move.diagonal)), "alabi_ens_set_move_scale")
                pooled = ha.pooled_step_size(state[:, 3])
                step_sizes.append(pooled); window_ends.append(end)
                self._last_window_chain = scratch
                if not last:
                    state.copy_(searched(pooled) if search else torch.as_tensor(ha.restart_state(WT, pooled), device=dev))
        torch.cuda.current_stream().synchronize()
        eps = ha.pooled_step_size(state[:, 3])
        move = NUTSMove(move.cov, step_size=eps, max_depth=move.max_depth, jitter=move.jitter)
        self._move_set = parse_moves(move, self.ndim)
        m = self._move_set
        _lib.check(_lib.lib().alabi_ens_set_move_scale(self._ens, 0, _lib.host_doubles(move.scale_matrix(self.ndim).ravel()),
                                                       int(move.diagonal)), "alabi_ens_set_move_scale")
        _lib.check(_lib.lib().alabi_ens_set_moves(self._ens, 1, (C.c_int * 1)(int(m.kind[0])), _lib.host_doubles(m.cum),
                                                  _lib.host_doubles(m.p0), _lib.host_doubles(m.p1)), "alabi_ens_set_moves")
        n_last = segments[-1][1] - segments[-1][0]
        cn = counts.cpu().numpy()
        self.nuts_tuning = dict(step_size=eps, cov=None if cov is None else np.array(cov, copy=True), window_ends=window_ends,
                                step_sizes=step_sizes, mean_accept_stat=float(stat.mean().item()) / n_last,
                                mean_depth=float(cn[:, 1].sum()) / (n_last * WT), divergences=int(cn[:, 2].sum()),
                                search_iters=search_iters, nwarmup=nwarmup, metric=metric, seconds=time.perf_counter() - t_start,
                                last_path="nuts-adapt")
        self.last_path = "nuts-adapt"
        self.last_stream_kernel = "ens_nuts_adapt_kernel"
        return State(self._coords.cpu().numpy(), self._logp.cpu().numpy())

    def reset(self):
        """emcee's reset(): forget the chain and the acceptance counts.  The draw counter is NOT rewound."""
        self._chains, self._chain_lps, self._thins = [], [], []
        self._naccept.zero_()
        self.iteration = 0
        self._tau_memo = None
        self._diag_memo = None

    # -------------------------------------------------------------------------- results
    def get_chain_device(self, discard=0, thin=1, flat=False, log_prob=False):
        src = self._chain_lps if log_prob else self._chains
        if not src:
            raise AttributeError("you must run the sampler with 'store == True' before accessing the results")
        v = src[0] if len(src) == 1 else torch.cat(src, dim=0)
        v = v[discard + thin - 1::thin]
        if flat:
            v = v.reshape((-1,) + tuple(v.shape[2:]))
        return v

    def get_chain(self, discard=0, thin=1, flat=False):
        return self.get_chain_device(discard, thin, flat).cpu().numpy()

    def get_log_prob(self, discard=0, thin=1, flat=False):
        return self.get_chain_device(discard, thin, flat, log_prob=True).cpu().numpy()

    def get_last_sample(self):
        if self._coords is None:
            raise AttributeError("you must run the sampler before accessing the results")
        return State(self._coords.cpu().numpy(), self._logp.cpu().numpy())

    @property
    def acceptance_fraction(self):
        return self._naccept.cpu().numpy() / float(max(self.iteration, 1))

    def get_autocorr_time(self, discard=0, thin=1, **kwargs):
        # run_emcee asks twice for the same numbers (estimate_burnin, then the summary: mcmc_utils.py:45, core.py:2387): remembered
        # until the chain grows or is reset
        key = (self.iteration, len(self._chains), int(discard), int(thin), tuple(sorted(kwargs.items())))
        memo = getattr(self, "_tau_memo", None)
        if memo is not None and memo[0] == key:
            return memo[1].copy()
        x = self.get_chain_device(discard=discard, thin=thin)
        tau = thin * integrated_time(x, **kwargs)
        self._tau_memo = (key, np.array(tau, copy=True))
        return tau

    def diagnostics(self, discard=0, thin=1):
        """Rank-normalised split R-hat, bulk / tail / mean ESS and the MCSE of the mean of the stored chain (Vehtari et al. 2021;
        alabi_amd/diagnostics.py ``summary``): a dict of [ndim] arrays mean, sd, mcse_mean, ess_mean, ess_bulk, ess_tail, rhat, in
        the sampler's coordinates.  The discard / thin view of the chain is read in place on the device; the result is remembered
        until the chain grows or is reset.  Every walker counts as a chain: the walkers are independent under the metropolis, hmc
        and nuts moves; under the red-blue ensemble moves the walkers of one ensemble are coupled -- R-hat still detects
        disagreement, but the ESS formula assumes independent chains and is approximate there."""
        key = (self.iteration, len(self._chains), int(discard), int(thin))
        memo = getattr(self, "_diag_memo", None)
        if memo is None or memo[0] != key:
            memo = self._diag_memo = (key, diagnostics.summary(self.get_chain_device(discard=discard, thin=thin)))
        return {k: v.copy() for k, v in memo[1].items()}

    def get_rhat(self, discard=0, thin=1):
        return self.diagnostics(discard, thin)["rhat"]

    def get_ess(self, method="bulk", discard=0, thin=1):
        if method not in ("bulk", "tail", "mean"):
            raise ValueError("method must be 'bulk', 'tail' or 'mean'")
        return self.diagnostics(discard, thin)["ess_" + method]
