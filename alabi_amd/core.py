"""SurrogateModel: drop-in for alabi's orchestration class on the GP-surrogate + MCMC hot path.

Keeps the public surface of ``alabi.core.SurrogateModel`` that BASELINE.json's north_star names
(``init_samples`` / ``init_gp`` / ``active_train`` / ``run_emcee`` a.k.a. ``run_mcmc``,
``surrogate_log_likelihood``, ``create_cached_surrogate_likelihood``, ``lnprob``, ``theta()``,
``y()``, ``training_results`` keys, result attributes) -- reference: alabi/core.py:248-251
(ctor), :542 (init_samples), :736-764 (init_gp), :1097 (_fit_gp), :1163 (_opt_gp), :1446
(surrogate_log_likelihood), :1535, :1587 (find_next_point), :1670 (active_train), :2073
(lnprob), :2108 (run_emcee), :2417 (run_dynesty) -- and swaps the third-party engines behind it:
george.GP -> ``HipGP``, emcee.EnsembleSampler -> ``alabi_amd.sampler.EnsembleSampler`` and
dynesty's nested samplers -> ``alabi_amd.nested.NestedSampler``.

``run_pymultinest`` (:2790) runs the same sampler with MultiNest's move, uniform draws inside bounding ellipsoids, and
``run_ultranest`` (:3241) with UltraNest's MLFriends region over those ellipsoids.

Out of scope here: plotting, MPI / process pools, the
parallel-chain trainer.  Deliberate differences are listed in DESIGN.md ("Differences").
"""
from __future__ import annotations

import copy
import math
import os
import pickle
import time
import warnings
from functools import partial

import numpy as np
import scipy.optimize as op
import torch

from . import gp_utils, mcmc_utils
from . import posterior as post
from . import utility as ut
from .gp import HipGP, _dev
from .moves import parse_moves
from .sampler import EnsembleSampler

__all__ = ["SurrogateModel", "CachedSurrogateLikelihood"]

_KERNELS = ("ExpSquaredKernel", "RationalQuadraticKernel", "Matern32Kernel", "Matern52Kernel")


class CachedSurrogateLikelihood:
    """Picklable callable: GP factorised once, then mean(-and-variance) predictions per call
    (alabi/core.py:28-122)."""

    def __init__(self, gp_iter, _y_cond, theta_scaler, y_scaler, ndim, return_var=False):
        self.gp_iter = gp_iter
        self._y_cond = _y_cond
        self.theta_scaler = theta_scaler
        self.y_scaler = y_scaler
        self.ndim = ndim
        self.return_var = return_var

    def __call__(self, theta_xs):
        theta_xs = np.asarray(theta_xs)
        one = theta_xs.ndim == 1
        if one:
            theta_xs = theta_xs.reshape(1, -1)
        elif theta_xs.ndim != 2:
            raise ValueError(f"theta_xs must be 1D or 2D array, got {theta_xs.ndim}D")
        _t = np.atleast_2d(self.theta_scaler.transform(theta_xs))
        if _t.shape[0] == 1 and _t.shape[1] != self.ndim and _t.size == self.ndim:
            _t = _t.reshape(1, -1)
        if not self.return_var:
            _yp = self.gp_iter.predict(self._y_cond, _t, return_var=False, return_cov=False)
            yp = self.y_scaler.inverse_transform(_yp.reshape(-1, 1)).flatten()
            return yp[0] if one else yp
        _yp, _vp = self.gp_iter.predict(self._y_cond, _t, return_var=True, return_cov=False)
        yp = self.y_scaler.inverse_transform(_yp.reshape(-1, 1)).flatten()
        if getattr(self.y_scaler, "scale_", None) is not None:
            vp = _vp * self.y_scaler.scale_[0] ** 2
        else:
            eps = 1e-6
            tr = self.y_scaler.inverse_transform(np.array([[0.0], [eps]]))
            vp = _vp * ((tr[1] - tr[0]) / eps) ** 2
        return (yp[0], vp[0]) if one else (yp, vp)


class SurrogateModel(object):
    def __init__(self, lnlike_fn=None, bounds=None, param_names=None, cache=True, savedir="results/",
                 model_name="surrogate_model", verbose=True, ncore=1, pool_method="forkserver",
                 ignore_warnings=True, random_state=None):
        if lnlike_fn is None:
            raise ValueError("Must supply lnlike_fn to train GP surrogate model.")
        if bounds is None:
            raise ValueError("Must supply prior bounds.")
        if random_state is None:
            random_state = int(time.time() * 1000000) % (2 ** 32)
        self.random_state = random_state
        self._rng = np.random.RandomState(random_state)
        self.lnlike_fn = lnlike_fn
        self.true_log_likelihood = lnlike_fn
        self.bounds = np.array(bounds)
        self.ndim = len(self.bounds)
        self.prior_sampler = partial(ut.prior_sampler, bounds=self.bounds, sampler="uniform", random_state=None)
        if param_names is not None:
            if len(param_names) != len(bounds):
                raise ValueError("Length of param_names must match length of bounds.")
            self.param_names = param_names
            self.labels = param_names
        else:
            self.param_names = [r"$\theta_%s$" % (i) for i in range(self.ndim)]
            self.labels = [f"theta_{i}" for i in range(self.ndim)]
        self.cache = cache
        self.savedir = savedir
        if not os.path.exists(self.savedir):
            os.makedirs(self.savedir)
        self.model_name = model_name
        self.verbose = verbose
        if ignore_warnings:
            warnings.filterwarnings("ignore", category=UserWarning)
            warnings.filterwarnings("ignore", category=FutureWarning)
        self.pool_method = pool_method
        self.ncore = max(int(ncore), 1)   # process pools are not used: the parallel axis is the GPU
        self.mpi_is_active = False
        self.emcee_run = False
        self.dynesty_run = False
        self.pymultinest_run = False
        self.ultranest_run = False

    # ------------------------------------------------------------------------- persistence
    def __getstate__(self):
        state = self.__dict__.copy()
        state["pool"] = None
        state.pop("_map_sampler", None)                       # find_map(method="bfgs-gpu")'s device handle and its plan (closures):
        state.pop("_map_plan", None)                          # working state of one call, rebuilt by the next
        if state.get("_emcee_full_src") is not None:          # the saved model carries the array itself, as the reference's does
            state["_emcee_full"] = self.emcee_samples_full
            state["_emcee_full_src"] = None
        return state

    @property
    def emcee_samples_full(self):
        """The whole chain [nsteps, nwalkers, ndim] in theta coordinates (core.py:2377).  Materialised on first access: at the
        reference's default 5e4 steps x 256 walkers it is a 1 GB copy out of HBM plus an un-scaling pass on the host (0.5 s, three
        times the sampling itself), which run_emcee should not charge to callers that never look at it."""
        if getattr(self, "_emcee_full", None) is None and getattr(self, "_emcee_full_src", None) is not None:
            sampler, t_add, t_mult = self._emcee_full_src
            self._emcee_full = (np.asarray(sampler.get_chain()) - t_add) / t_mult
            self._emcee_full_src = None
        if getattr(self, "_emcee_full", None) is None:
            raise AttributeError("emcee_samples_full: run_emcee has not been called")
        return self._emcee_full

    @emcee_samples_full.setter
    def emcee_samples_full(self, value):
        self._emcee_full, self._emcee_full_src = value, None

    def save(self):
        """Pickle the model (write-to-temp then rename, alabi/core.py:371-392)."""
        file = os.path.join(self.savedir, self.model_name)
        tmp = file + ".pkl.tmp"
        try:
            with open(tmp, "wb") as f:
                pickle.dump(self, f)
            os.rename(tmp, file + ".pkl")
        except Exception:
            if os.path.exists(tmp):
                os.remove(tmp)
            raise

    def _seed(self):
        return int(self._rng.randint(0, 2 ** 31 - 1))

    # --------------------------------------------------------------------- data / scalers
    def _lnlike_fn(self, _theta):
        theta = self.theta_scaler.inverse_transform(_theta).flatten()
        y = np.asarray(self.true_log_likelihood(theta)).reshape(-1, 1)
        return self.y_scaler.transform(y).flatten()

    def theta(self):
        return self.theta_scaler.inverse_transform(self._theta)

    def y(self):
        return self.y_scaler.inverse_transform(self._y.reshape(-1, 1)).flatten()

    def refit_scalers(self, theta, y, theta_scaler=None, y_scaler=None):
        if theta_scaler is not None:
            self.theta_scaler = theta_scaler
        if y_scaler is not None:
            self.y_scaler = y_scaler
        # The identity scalers (``no_scaler``, the default) pass their input through: after their first fit the sklearn round trip
        # (parameter validation + check_array, ~0.15 ms per call) is skipped -- it was a tenth of a small active-learning iteration.
        def _identity(sc):
            return (getattr(sc, "func", None) is ut._ident and getattr(sc, "inverse_func", None) is ut._ident
                    and any(sc is f for f in self._scalers_fitted))
        if not hasattr(self, "_scalers_fitted"):
            self._scalers_fitted = []
        if _identity(self.theta_scaler):
            _theta = np.array(theta, dtype=np.float64)
        else:
            self.theta_scaler.fit(self.bounds.T)
            _theta = self.theta_scaler.transform(theta)
        if _identity(self.y_scaler):
            _y = np.array(y, dtype=np.float64).reshape(-1)
        else:
            _y = self.y_scaler.fit_transform(np.asarray(y).reshape(-1, 1)).flatten()
        for sc in (self.theta_scaler, self.y_scaler):
            if not any(sc is f for f in self._scalers_fitted):
                self._scalers_fitted.append(sc)
        for name, arr in (("theta_scaler", _theta), ("y_scaler", _y)):
            if np.any(np.isnan(arr)):
                raise ValueError(f"Refitted {name} produced NaN values!")
            if np.any(np.isinf(arr)):
                raise ValueError(f"Refitted {name} produced Inf values!")
        return _theta, _y

    def init_train(self, nsample=None, sampler="uniform", fname="initial_training_sample.npz"):
        if nsample is None:
            nsample = 50 * self.ndim
        theta = ut.prior_sampler(bounds=self.bounds, nsample=nsample, sampler=sampler, random_state=self._seed())
        y = np.array([self.true_log_likelihood(tt) for tt in theta], dtype=np.float64).reshape(-1, 1)
        for ii in range(len(y)):
            while not np.isfinite(y[ii, 0]):
                new_theta = ut.prior_sampler(bounds=self.bounds, nsample=1, sampler="uniform", random_state=self._seed())
                y[ii] = np.asarray(self.true_log_likelihood(new_theta[0])).reshape(-1)[0]
                theta[ii] = new_theta
        if self.cache:
            np.savez(f"{self.savedir}/{fname}", theta=theta, y=y)
        return theta, y

    def load_train(self, cache_file):
        sims = np.load(cache_file)
        theta, y = sims["theta"], sims["y"]
        if self.ndim != theta.shape[1]:
            raise ValueError(f"Dimension of bounds (n={self.ndim}) does not match dimension of training theta "
                             f"(n={theta.shape[1]})")
        return theta, y

    def _samples(self, n, sampler, file, default_name):
        if file is not None:
            path = file if os.path.exists(file) else f"{self.savedir}/{file}"
            try:
                theta, y = self.load_train(path)
                print(f"Loaded {len(theta)} samples from {path}.")
                return theta, y
            except Exception as e:  # noqa: BLE001
                print(f"Unable to reload {path} due to error: {e}. Computing new samples...")
                return self.init_train(nsample=n, sampler=sampler, fname=file)
        return self.init_train(nsample=n, sampler=sampler, fname=default_name)

    def init_samples(self, ntrain=100, ntest=0, sampler="uniform", train_file=None, test_file=None):
        theta, y = self._samples(ntrain, sampler, train_file, "initial_train_file_sample.npz")
        if ntest > 0:
            self.theta_test, self.y_test = self._samples(ntest, sampler, test_file, "initial_test_sample.npz")
            self.ntest = len(self.theta_test)
        else:
            self.theta_test, self.y_test, self.ntest = [], [], 0
        self.theta_train = theta
        self.y_train = y
        self.ninit_train = len(theta)
        self.ntrain = self.ninit_train
        self.nactive = 0

    # ------------------------------------------------------------------ hyper-parameters
    def set_hyperparam_prior_bounds(self):
        """Box for the hyper-parameter search (alabi/core.py:628-662).  The amplitude box is built from
        the LINEAR var(y) although the parameter is a log -- reference behaviour, kept."""
        pnames = self.param_names_optimized if self.uniform_scales else list(self.param_names_full)
        hp = [[None, None] for _ in pnames]
        if self.fit_mean:
            m, s = np.mean(self._y), np.std(self._y)
            hp[pnames.index("mean:value")] = [m - s, m + s]
        if self.fit_amp:
            v = np.var(self._y)
            hp[pnames.index(f"{self.kernel_amp_key}:log_constant")] = [v * 10 ** self.gp_amp_rng[0], v * 10 ** self.gp_amp_rng[1]]
        if self.fit_white_noise:
            hp[pnames.index("white_noise:value")] = [self.white_noise - 3, self.white_noise + 3]
        for ii, name in enumerate(pnames):       # RationalQuadraticKernel's shape parameter (the reference leaves it unbounded)
            if name.endswith(":log_alpha"):
                hp[ii] = [-3.0, 3.0]
        if self.uniform_scales:
            hp[pnames.index(f"{self.kernel_scale_key}:metric:log_M")] = list(self.gp_scale_rng)
        else:
            for ii in range(self.ndim):
                hp[pnames.index(f"{self.kernel_scale_key}:metric:log_M_{ii}_{ii}")] = list(self.gp_scale_rng)
        self.hp_bounds = np.array(hp)
        self.gp_hyper_prior = partial(ut.lnprior_uniform, bounds=self.hp_bounds)

    def expand_hyperparameter_vector(self, optimized_params):
        if optimized_params is None:
            raise ValueError("optimized_params cannot be None")
        if not self.uniform_scales:
            return optimized_params
        full = np.ones(len(self.param_names_full))
        names_f, names_o = list(self.param_names_full), self.param_names_optimized
        for key in ("mean:value", f"{getattr(self, 'kernel_amp_key', 'kernel:k1')}:log_constant", "white_noise:value"):
            if key in names_f and key in names_o:
                full[names_f.index(key)] = optimized_params[names_o.index(key)]
        for ii in range(self.ndim):
            full[names_f.index(f"{self.kernel_scale_key}:metric:log_M_{ii}_{ii}")] = \
                optimized_params[names_o.index(f"{self.kernel_scale_key}:metric:log_M")]
        return np.array(full)

    def set_hyperparameter_vector(self, tmp_gp, optimized_params):
        if optimized_params is None:
            raise ValueError("optimized_params cannot be None. Cannot set hyperparameters.")
        tmp_gp.set_parameter_vector(self.expand_hyperparameter_vector(optimized_params))
        return tmp_gp

    def get_hyperparameter_dict(self, gp):
        d = gp.get_parameter_dict()
        if self.uniform_scales:
            d[f"{self.kernel_scale_key}:metric:log_M"] = d.pop(f"{self.kernel_scale_key}:metric:log_M_0_0")
            for ii in range(1, self.ndim):
                del d[f"{self.kernel_scale_key}:metric:log_M_{ii}_{ii}"]
        return d

    def get_hyperparameter_vector(self, gp):
        return np.fromiter(self.get_hyperparameter_dict(gp).values(), dtype=float)

    # --------------------------------------------------------------------------- init_gp
    def init_gp(self, kernel="ExpSquaredKernel", fit_amp=True, fit_mean=True, fit_white_noise=True, white_noise=-12,
                gp_scale_rng=[-2, 2], gp_amp_rng=[-1, 1], uniform_scales=False, overwrite=False,
                theta_scaler=ut.no_scaler, y_scaler=ut.no_scaler, gp_opt_method="l-bfgs-b", gp_nopt=3,
                optimizer_kwargs={"maxiter": 100, "xatol": 1e-4, "fatol": 1e-3, "adaptive": True},
                hyperopt_method="cv", regularize=True, amp_0=1.0, mu_0=1.0, sigma_0=2.0, cv_folds=5,
                cv_scoring="mse", cv_n_candidates=100, cv_stage2_candidates=50, cv_stage2_width=0.5,
                cv_stage3_candidates=25, cv_stage3_width=0.25, cv_weighted_factor=1.0, multi_proc=True):
        if hasattr(self, "gp") and not overwrite:
            raise AssertionError("GP kernel already assigned. Use overwrite=True to re-assign the kernel.")
        if kernel not in _KERNELS:
            raise ValueError(f"Kernel '{kernel}' is not a valid option. Valid options: ExpSquaredKernel, "
                             "Matern32Kernel, Matern52Kernel, RationalQuadraticKernel")
        self.fit_amp, self.fit_mean, self.fit_white_noise = fit_amp, fit_mean, fit_white_noise
        self.white_noise = white_noise
        self.uniform_scales = uniform_scales
        self.gp_opt_method = gp_opt_method
        self.gp_nopt = gp_nopt
        self.opt_gp_kwargs = {"hyperopt_method": hyperopt_method, "regularize": regularize, "amp_0": amp_0,
                              "mu_0": mu_0, "sigma_0": sigma_0, "optimizer_kwargs": optimizer_kwargs,
                              "cv_folds": cv_folds, "cv_scoring": cv_scoring, "cv_n_candidates": cv_n_candidates,
                              "cv_stage2_candidates": cv_stage2_candidates, "cv_stage2_width": cv_stage2_width,
                              "cv_stage3_candidates": cv_stage3_candidates, "cv_stage3_width": cv_stage3_width,
                              "cv_weighted_factor": cv_weighted_factor, "multi_proc": multi_proc}
        self.theta_scaler = theta_scaler
        self.theta_scaler.fit(self.bounds.T)
        self._bounds = self.theta_scaler.transform(self.bounds.T).T
        self._prior_sampler = partial(ut.prior_sampler, bounds=self._bounds, sampler="uniform", random_state=None)
        self.y_scaler = y_scaler
        self._theta, self._y = self.refit_scalers(self.theta_train, self.y_train)
        if self.ntest > 0:
            self._theta_test = self.theta_scaler.transform(self.theta_test)
            self._y_test = self.y_scaler.transform(np.asarray(self.y_test).reshape(-1, 1)).flatten()
        self._theta_train, self._y_train = self._theta, self._y
        self.training_results = {k: [] for k in (
            "iteration", "gp_hyperparameters", "gp_hyperparameter_opt_iteration", "gp_hyperparam_opt_time",
            "training_mse", "test_mse", "training_scaled_mse", "test_scaled_mse", "gp_kl_divergence",
            "gp_train_time", "obj_fn_opt_time", "acquisition_optimizer_niter")}
        self.gp_scale_rng, self.gp_amp_rng = gp_scale_rng, gp_amp_rng
        self.kernel_name = kernel
        gp = None
        for attempt in range(1, 11):  # reference: up to 10 random initial length scales (core.py:980-1048)
            log_ls = self._rng.uniform(min(gp_scale_rng), max(gp_scale_rng), self.ndim)
            self.kernel = {"name": kernel, "log_M": log_ls.copy(), "log_constant": 0.0, "log_alpha": 1.0}
            gp = gp_utils.configure_gp(self._theta, self._y, self.kernel, fit_amp=fit_amp, fit_mean=fit_mean,
                                       fit_white_noise=fit_white_noise, white_noise=white_noise)
            if gp is not None:
                if self.verbose:
                    print(f"Successfully initialized GP on attempt {attempt}")
                break
            print("Warning: configure_gp returned None. Retrying with new initial scale length...")
        if gp is None:
            raise RuntimeError(f"Failed to initialize GP after 10 attempts. Check your data, kernel choice, and "
                               f"scale bounds. Current settings: kernel={kernel}, gp_scale_rng={gp_scale_rng}")
        self.gp = gp
        self.param_names_full = self.gp.get_parameter_names(include_frozen=False)
        self.kernel_scale_key = [x for x in self.param_names_full if "metric:log_M" in x][0].split(":metric:log_M")[0]
        self.param_names_optimized = []
        if fit_mean:
            self.param_names_optimized.append("mean:value")
        if fit_amp:      # without the amplitude the model has no log_constant parameter at all (core.py:1057-1059)
            self.kernel_amp_key = [x for x in self.param_names_full if "log_constant" in x][0].split(":log_constant")[0]
            self.param_names_optimized.append(f"{self.kernel_amp_key}:log_constant")
        if fit_white_noise:
            self.param_names_optimized.append("white_noise:value")
        if uniform_scales:
            self.param_names_optimized.append(f"{self.kernel_scale_key}:metric:log_M")
        else:
            self.param_names_optimized += [f"{self.kernel_scale_key}:metric:log_M_{ii}_{ii}" for ii in range(self.ndim)]
        self.hp_length_indices = [i for i, n in enumerate(self.param_names_full) if "metric:log_m" in n.lower()]
        self.hp_other_indices = [i for i, n in enumerate(self.param_names_full) if "metric:log_m" not in n.lower()]
        if uniform_scales:
            self.hp_length_index = [self.param_names_optimized.index(f"{self.kernel_scale_key}:metric:log_M")]
        self.initial_gp_hyperparameters = self.get_hyperparameter_vector(self.gp)
        self.gp, _ = self._opt_gp(**self.opt_gp_kwargs)
        if self.ntest > 0:
            _yt = self.gp.predict(self._y, self._theta_test, return_cov=False, return_var=False)
            yt = self.y_scaler.inverse_transform(_yt.reshape(-1, 1)).flatten()
            yt_true = self.y_scaler.inverse_transform(self._y_test.reshape(-1, 1)).flatten()
            return np.mean((yt_true - yt) ** 2)
        return None

    def _new_gp(self, _y):
        log_const = np.log(np.var(_y) / self.ndim) if self.fit_amp else self.kernel.get("log_constant", 0.0)
        return HipGP(self.ndim, mean=np.median(_y), white_noise=self.white_noise, log_constant=log_const,
                     log_M=self.kernel["log_M"], fit_mean=self.fit_mean, fit_white_noise=self.fit_white_noise,
                     kernel=self.kernel.get("name", "ExpSquaredKernel"), log_alpha=self.kernel.get("log_alpha", 1.0),
                     fit_amp=self.fit_amp)

    def _fit_gp(self, _theta=None, _y=None, hyperparameters=None):
        """New GP on (_theta, _y) with the carried hyper-parameter vector, factorised (core.py:1097-1160)."""
        _theta = self._theta if _theta is None else _theta
        _y = self._y if _y is None else _y
        t0 = time.time()
        self.set_hyperparam_prior_bounds()
        if not np.all(np.isfinite(_theta)):
            raise ValueError("_theta contains NaN or Inf values")
        if not np.all(np.isfinite(_y)):
            raise ValueError(f"_y contains NaN or Inf values: {_y[~np.isfinite(_y)]}")
        y_var = np.var(_y)
        if not np.isfinite(np.median(_y)):
            raise ValueError("median(_y) is not finite")
        if not np.isfinite(y_var) or y_var == 0:
            raise ValueError(f"var(_y) is not finite or zero: {y_var}")
        gp = self._new_gp(_y)
        if hyperparameters is not None and not np.all(np.isfinite(np.atleast_1d(hyperparameters))):
            print("Warning: Hyperparameters contain NaN or Inf. Reoptimizing hyperparameters from scratch...")
            gp, _ = self._opt_gp(**self.opt_gp_kwargs, _theta=_theta, _y=_y)
            if not np.all(np.isfinite(gp.get_parameter_vector())):
                raise ValueError("Reoptimized GP still has invalid parameters")
            return gp, time.time() - t0
        gp = self.set_hyperparameter_vector(gp, hyperparameters)
        # one more training point, same kernel hyper-parameters: extend the previous factor instead of refactorising
        gp.compute_from(getattr(self, "gp", None), _theta)
        return gp, time.time() - t0

    def _opt_gp(self, hyperopt_method="ml", regularize=True, amp_0=1.0, mu_0=1.0, sigma_0=2.0,
                optimizer_kwargs={"maxiter": 100, "xatol": 1e-4, "fatol": 1e-3, "adaptive": True},
                cv_folds=5, cv_scoring="mse", cv_n_candidates=20, multi_proc=True, cv_stage2_candidates=None,
                cv_stage2_width=0.5, cv_stage3_candidates=None, cv_stage3_width=0.2,
                cv_weighted_mse_method="exponential", cv_weighted_factor=1.0, _theta=None, _y=None,
                theta_scaler=None, y_scaler=None):
        """Hyper-parameter selection: marginal likelihood ("ml") or staged k-fold CV ("cv") (core.py:1163-1403)."""
        t0 = time.time()
        _theta = self._theta if _theta is None else _theta
        _y = self._y if _y is None else _y
        if hyperopt_method.lower() not in ("ml", "cv"):
            print(f"Invalid method '{hyperopt_method}'. Must be 'ml' or 'cv'. Defaulting to 'ml'.")
            hyperopt_method = "ml"
        self.set_hyperparam_prior_bounds()
        op_gp = None
        if hyperopt_method.lower() == "ml":
            gp = self.gp
            gp.compute(_theta)

            def make_objective(gp):
                """(nll, grad_nll) bound to one GP handle: restarts run concurrently on their own copies."""
                def nll(p_opt):
                    p = self.expand_hyperparameter_vector(p_opt)
                    self.set_hyperparameter_vector(gp, p_opt)
                    v = -gp.log_likelihood(_y, quiet=True)
                    if regularize:
                        v += gp_utils.regularization_term(p, self.hp_length_indices, amp_0=amp_0, mu_0=mu_0, sigma_0=sigma_0)
                    return v if np.isfinite(v) else 1e25

                def grad_nll(p_opt):
                    """-d logL/dp from the device's analytic gradient (+ the regulariser's), assembled exactly as the
                    reference does (core.py:1255-1277): with uniform_scales the shared length-scale entry receives the MEAN
                    of the per-dimension gradients.  Zeros, without the regulariser's part, where the objective is the constant
                    1e25 (K not positive definite)."""
                    p = self.expand_hyperparameter_vector(p_opt)
                    self.set_hyperparameter_vector(gp, p_opt)
                    try:
                        if not gp.recompute(quiet=True):
                            return np.zeros(len(p_opt))      # K not positive definite: nll is the constant 1e25 there
                        grad_lnlike = -gp.grad_log_likelihood(_y, quiet=True)
                    except (np.linalg.LinAlgError, RuntimeError):
                        return np.zeros(len(p_opt))
                    if not np.all(np.isfinite(grad_lnlike)):
                        return np.zeros(len(p_opt))
                    if self.uniform_scales:
                        gll = np.zeros(len(p_opt))
                        gll[self.hp_length_index] = np.mean(grad_lnlike[self.hp_length_indices])
                        gll[self.hp_other_indices] = grad_lnlike[self.hp_other_indices]
                    else:
                        gll = grad_lnlike
                    if regularize:
                        reg_grad = gp_utils.regularization_gradient(p, self.hp_length_indices, amp_0=amp_0, mu_0=mu_0,
                                                                    sigma_0=sigma_0)
                        if self.uniform_scales:
                            gll[self.hp_length_index] += np.mean(reg_grad[self.hp_length_indices])
                        else:
                            gll = gll + reg_grad
                    return gll
                return nll, grad_nll

            nll, grad_nll = make_objective(gp)

            use_grad = self.gp_opt_method in ("newton-cg", "l-bfgs-b")
            opts = dict(optimizer_kwargs)
            if self.gp_opt_method == "l-bfgs-b":
                opts = {k: v for k, v in opts.items() if k in ("maxiter", "ftol", "gtol", "maxcor", "maxfun", "maxls")}

            def _run(x0, f=nll, g=grad_nll):
                return op.minimize(fun=f, x0=x0, jac=g if use_grad else None, method=self.gp_opt_method,
                                   bounds=self.hp_bounds, options=opts)

            current = self.get_hyperparameter_vector(gp)
            if self.gp_nopt <= 1:
                res = _run(current)
            else:
                p0 = ut.prior_sampler(bounds=self.hp_bounds, nsample=self.gp_nopt, sampler="lhs", random_state=self._seed())
                p0[0] = current
                nthreads = max(1, min(self.gp_nopt, int(os.environ.get("ALABI_ML_THREADS", self.gp_nopt))))
                if nthreads <= 1:
                    res = min((_run(p) for p in p0), key=lambda r: r.fun)
                else:
                    # The restarts are independent: each gets its own GP handle, HIP stream and host thread (every objective call
                    # is a chain of small launches with read-backs that fills only part of the chip; ctypes releases the GIL).
                    # The reference runs them one after the other (core.py:1287-1305); same optimum, ties broken by start order.
                    from concurrent.futures import ThreadPoolExecutor

                    def _restart(x0):
                        g_i = copy.deepcopy(gp)
                        with torch.cuda.stream(torch.cuda.Stream()):
                            g_i.compute(_theta)
                            f_i, d_i = make_objective(g_i)
                            r = _run(x0, f_i, d_i)
                            torch.cuda.current_stream().synchronize()
                        return r

                    torch.cuda.current_stream().synchronize()
                    with ThreadPoolExecutor(max_workers=nthreads) as pool:
                        results = list(pool.map(_restart, list(p0)))
                    res = min(results, key=lambda r: r.fun)
            best = res.x
            if not (np.all(np.isfinite(best)) and np.isfinite(res.fun) and res.fun < 1e25):
                # e.g. the incumbent lies outside the reference's amplitude box (built from the linear var(y),
                # core.py:654) and every point inside it overflows: keep the incumbent, as the CV branch does
                print("Warning: ML hyper-parameter search found no valid point; keeping current hyperparameters.")
                best = current
            op_gp = self.set_hyperparameter_vector(gp, best)
            if not op_gp.compute(_theta, quiet=True):
                op_gp = self.set_hyperparameter_vector(gp, current)
                op_gp.compute(_theta)
            if self.verbose:
                print(f"GP ML fit: -logL(+reg) {nll(current):.4f} -> {nll(best):.4f} in {res.nit} iterations")
                self.set_hyperparameter_vector(gp, best)
                gp.compute(_theta)
        else:
            if self.verbose:
                print(f"\nOptimizing GP hyperparameters using {cv_folds}-fold cross-validation...")
            try:
                cands = ut.prior_sampler(bounds=self.hp_bounds, nsample=cv_n_candidates, sampler="lhs",
                                         random_state=self._seed())
                if hasattr(self, "gp"):
                    cands[0] = self.get_hyperparameter_vector(self.gp)
                if self.uniform_scales:
                    cands = np.array([self.expand_hyperparameter_vector(c) for c in cands])
                # several ranks (one process per GPU, torch.distributed initialised) and multi_proc: the candidates of every
                # stage are dealt over the ranks -- the reference maps them over its process pool (gp_utils.py:640-700) -- and the
                # partial score vectors (+inf elsewhere) are combined with one MIN all-reduce; every rank then picks the same winner
                from . import dist as adist
                rank, world = adist.world_info()
                shard_kw = {}
                if world > 1 and multi_proc:
                    shard_kw = dict(ranks=(rank, world), reduce_scores=lambda sc: adist.allreduce_array(sc, "min"))
                op_gp = gp_utils.optimize_gp_kfold_cv(
                    self.gp, _theta, _y, cands, self.y_scaler, k_folds=cv_folds, scoring=cv_scoring,
                    stage2_candidates=cv_stage2_candidates, stage2_width=cv_stage2_width,
                    stage3_candidates=cv_stage3_candidates, stage3_width=cv_stage3_width,
                    weighted_mse_method=cv_weighted_mse_method, weighted_mse_factor=cv_weighted_factor,
                    verbose=self.verbose, random_state=self._seed(), **shard_kw)
            except Exception as e:  # noqa: BLE001
                print(f"Warning: CV hyperparameter optimization failed: {e}")
                op_gp = None
        if op_gp is None:
            if hasattr(self, "gp"):
                op_gp = self.gp
                op_gp.compute(_theta)
            else:
                op_gp = self._new_gp(_y)
                op_gp.compute(_theta)
        timing = time.time() - t0
        self.training_results["gp_hyperparam_opt_time"].append(timing)
        return op_gp, timing

    # ------------------------------------------------------------------ surrogate likelihood
    def eval_gp_at_iteration(self, iter, return_var=False):
        """predict-callable of the GP as it stood at active-learning iteration ``iter`` (core.py:1406-1443).

        The reference re-factorises on every call; here the current GP is reused for iter == -1 (it already
        holds the latest data and hyper-parameters) and other iterations are factorised once and memoised."""
        res = self.training_results
        n_it = len(res["iteration"])
        if iter == -1 or iter == n_it:
            if n_it > 0:
                want = np.asarray(res["gp_hyperparameters"][-1])
                if not np.array_equal(want, self.gp.get_parameter_vector()):
                    self.gp.set_parameter_vector(want)
                    self.gp.compute(self._theta)
            gp_iter, _y_cond = self.gp, self._y
        else:
            if iter == 0 or n_it == 0:
                n_cond = self.ninit_train
                hp = res["gp_hyperparameters"][0] if n_it > 0 else self.initial_gp_hyperparameters
            elif 0 < iter < n_it:
                n_cond = self.ninit_train + iter
                hp = res["gp_hyperparameters"][iter]
            else:
                raise ValueError(f"Iteration {iter} exceeds available training iterations ({res['iteration'][-1]}).")
            memo = self.__dict__.setdefault("_gp_iter_memo", {})
            key = (iter, self.ntrain)
            if key not in memo:
                g = self._new_gp(self._y[:n_cond])
                g.set_parameter_vector(hp)
                g.compute(self._theta[:n_cond])
                memo.clear()
                memo[key] = g
            gp_iter, _y_cond = memo[key], self._y[:n_cond]

        def gp_predict(x):
            x = np.atleast_2d(x)
            if x.shape[1] != self.ndim and x.size == self.ndim:
                x = x.reshape(1, -1)
            return gp_iter.predict(_y_cond, x, return_var=return_var, return_cov=False)

        return gp_predict

    def surrogate_log_likelihood(self, theta_xs, iter=-1, return_var=False):
        """GP surrogate of the log-likelihood at theta_xs ([d] -> scalar, [M,d] -> array) (core.py:1446-1508)."""
        theta_xs = np.asarray(theta_xs)
        one = theta_xs.ndim == 1
        if one:
            theta_xs = theta_xs.reshape(1, -1)
        elif theta_xs.ndim != 2:
            raise ValueError(f"theta_xs must be 1D or 2D array, got {theta_xs.ndim}D")
        _t = self.theta_scaler.transform(theta_xs)
        if hasattr(self, "training_results") and len(self.training_results["iteration"]) > 0:
            gp_ii = self.eval_gp_at_iteration(iter, return_var=return_var)
        else:
            gp_ii = lambda x: self.gp.predict(self._y, x, return_var=return_var, return_cov=False)  # noqa: E731
        if not return_var:
            yp = self.y_scaler.inverse_transform(gp_ii(_t).reshape(-1, 1)).flatten()
            return yp[0] if one else yp
        _yp, _vp = gp_ii(_t)
        yp = self.y_scaler.inverse_transform(_yp.reshape(-1, 1)).flatten()
        vp = self.y_scaler.inverse_transform(_vp.reshape(-1, 1)).flatten()   # reference quirk (core.py:1502)
        return (yp[0], vp[0]) if one else (yp, vp)

    def surrogate_likelihood(self, theta_xs):
        """Predictive probability (not log) of the GP at theta_xs (core.py:1511-1533)."""
        return np.exp(self.surrogate_log_likelihood(theta_xs))

    def create_cached_surrogate_likelihood(self, iter=-1, return_var=False):
        """Factorise once, return a picklable callable (core.py:1535-1584)."""
        if hasattr(self, "training_results") and len(self.training_results["iteration"]) > 0:
            n_cond = len(self._theta) if iter == -1 else self.ninit_train + iter
            hp = self.training_results["gp_hyperparameters"][-1]
        else:
            n_cond = len(self._theta)
            hp = self.gp.get_parameter_vector()
        _tc, _yc = self._theta[:n_cond], self._y[:n_cond]
        gp_iter = gp_utils.configure_gp(_tc, _yc, self.kernel, fit_amp=self.fit_amp, fit_mean=self.fit_mean,
                                        fit_white_noise=self.fit_white_noise, white_noise=self.white_noise,
                                        hyperparameters=hp)
        if gp_iter is None:
            raise np.linalg.LinAlgError("create_cached_surrogate_likelihood: GP factorisation failed")
        return CachedSurrogateLikelihood(gp_iter, _yc, self.theta_scaler, self.y_scaler, self.ndim, return_var=return_var)

    # ---------------------------------------------------------------------- active learning
    def find_next_point(self, nopt=3, optimizer_kwargs={}):
        """Next training point = arg-min of the acquisition function (core.py:1587-1667).

        obj_opt_method "scan" (default here): ``ncand`` uniform candidates in the scaled box are scored in
        one batched HIP pass (predict mean+variance -> utility -> arg-min), then ``refine`` zoom stages of
        ``nrefine`` candidates each around the ``ntop`` best; then the incumbent is polished by
        a projected L-BFGS with the closed-form GPU gradient (``optimizer_kwargs={"polish": maxiter}``, default 30, 0 = off;
        ``"polish_method": "scipy"`` runs scipy's L-BFGS-B around the same evaluations instead).  Any scipy method name keeps
        the reference's multistart local optimisation with one GP prediction per objective call."""
        t0 = time.time()
        y_best = float(np.max(self._y))
        method = str(self.obj_opt_method).lower()
        kw = dict(optimizer_kwargs or {})
        if method == "scan":
            ncand = int(kw.get("ncand", 16384))
            gen = torch.Generator(device=_dev())
            gen.manual_seed(self._seed())
            lo = torch.as_tensor(self._bounds[:, 0], device=_dev())
            hi = torch.as_tensor(self._bounds[:, 1], device=_dev())
            cand = lo + (hi - lo) * torch.rand((ncand, self.ndim), dtype=torch.float64, device=_dev(), generator=gen)
            nref, nper, ntop = int(kw.get("refine", 4)), int(kw.get("nrefine", 4096)), int(kw.get("ntop", 32))
            from . import dist as adist
            rank, world = adist.world_info()
            if world > 1 and getattr(self, "allow_opt_multiproc", True) and ncand >= world:
                # several ranks: every rank holds the same GP and draws the same candidates; it scores ITS contiguous slice, one
                # (value, index) pair and the slices' best `ntop` are exchanged, and every rank goes on from the same incumbent
                # and the same centres (BASELINE config C5: 1e6 candidates over 8 GPUs).  The reference
                # spreads its scipy restarts over a process pool instead (alabi/utility.py:1030-1163, allow_opt_multiproc).
                b0, e0 = adist.slice_bounds(ncand, world, rank)
                out = ut.utility_scan(self.gp, self._y, cand[b0:e0], self._bounds, algorithm=self.algorithm, y_best=y_best,
                                      return_all=nref > 0)
                gi_local = b0 + int(out[2]) if out[2] >= 0 and np.isfinite(out[1]) else -1
                u_best, idx = adist.reduce_min_index(out[1] if gi_local >= 0 else np.inf, gi_local)
                _thetaN = cand[idx].cpu().numpy() if idx >= 0 else np.nan
                centers = None
                if idx >= 0 and nref > 0:
                    u_loc = torch.where(torch.isfinite(out[3]), out[3], torch.full_like(out[3], float("inf")))
                    kk = min(ntop, e0 - b0)
                    top = torch.topk(-u_loc, kk)
                    mine = np.full((ntop, 2), [np.inf, -1.0])
                    mine[:kk, 0] = (-top.values).cpu().numpy()
                    mine[:kk, 1] = (top.indices + b0).cpu().numpy()
                    allp = adist.allgather_rows(mine)
                    allp = allp[allp[:, 1] >= 0]
                    keep = allp[np.lexsort((allp[:, 1], allp[:, 0]))][:min(ntop, ncand)]      # ascending value, ties to the lower index
                    centers = cand[torch.as_tensor(keep[:, 1].astype(np.int64), device=_dev())]
            else:
                out = ut.utility_scan(self.gp, self._y, cand, self._bounds, algorithm=self.algorithm, y_best=y_best,
                                      return_all=nref > 0, best_on_device=True)
                _thetaN, u_best, idx = out[:3]              # (the incumbent stays on the device through the zoom stages)
                centers = None
                if idx >= 0 and nref > 0:
                    u_all = torch.nan_to_num(out[3], nan=float("inf"), posinf=float("inf"), neginf=float("inf"))
                    centers = cand[torch.topk(u_all, min(ntop, ncand), largest=False).indices]
            # Zoom stages (stand in for the reference's local optimiser, utility.py:1030-1163, at batched-scan cost):
            # Gaussian clouds of shrinking width around the best candidates so far, scored in one pass each.
            if idx >= 0 and nref > 0:
                # (few launches per stage: at small N a stage is launch latency -- one fused multiply-add for the cloud, one clamp
                # against precomputed inner bounds, nan_to_num instead of isfinite / full_like / where, topk on the values themselves)
                width = 0.08 * (hi - lo)
                lo_in, hi_in = lo + 1e-12 * (hi - lo), hi - 1e-12 * (hi - lo)
                for _ in range(nref):
                    rep = centers[torch.randint(0, centers.shape[0], (nper,), device=_dev(), generator=gen)]
                    cloud = torch.addcmul(rep, torch.randn((nper, self.ndim), dtype=torch.float64, device=_dev(), generator=gen), width)
                    cloud = torch.clamp(cloud, min=lo_in, max=hi_in)
                    cloud[0] = torch.as_tensor(_thetaN, device=_dev())          # the incumbent can only be improved on
                    o2 = ut.utility_scan(self.gp, self._y, cloud, self._bounds, algorithm=self.algorithm, y_best=y_best,
                                         return_all=True, best_on_device=True)
                    if o2[2] >= 0 and o2[1] <= u_best:
                        _thetaN, u_best = o2[0].clone(), o2[1]
                    u2 = torch.nan_to_num(o2[3], nan=float("inf"), posinf=float("inf"), neginf=float("inf"))
                    centers = cloud[torch.topk(u2, min(ntop, nper), largest=False).indices]
                    width = 0.3 * width
            if isinstance(_thetaN, torch.Tensor):
                _thetaN = _thetaN.cpu().numpy()
            # optional continuous polish of the incumbent: L-BFGS-B with the closed-form GPU gradient
            npolish = int(kw.get("polish", 30))
            if idx >= 0 and npolish > 0:
                th_p, u_p = ut.polish_point(self.gp, self._y, _thetaN, self._bounds, algorithm=self.algorithm, y_best=y_best,
                                            maxiter=npolish, method=str(kw.get("polish_method", "native")))
                if u_p < u_best:
                    _thetaN, u_best = th_p, u_p
            self.last_acquisition_value = float(u_best) if idx >= 0 else np.nan
            if idx < 0:
                _thetaN = np.nan
        else:
            predict_gp = lambda _x: self.gp.predict(self._y, _x, return_var=True)  # noqa: E731
            if self.algorithm == "jones":
                obj_fn = partial(self.utility, predict_gp=predict_gp, bounds=self._bounds, y_best=y_best)
            else:
                obj_fn = partial(self.utility, predict_gp=predict_gp, bounds=self._bounds)
            for k in ("ncand", "polish", "polish_method", "refine", "nrefine", "ntop"):
                kw.pop(k, None)
            grad_obj_fn = None           # analytic gradient on the GPU (reference: core.py:1618-1625 passes grad_utility)
            if getattr(self, "use_grad_opt", True) and getattr(self, "grad_utility", None) is not None:
                grad_obj_fn = partial(self.grad_utility, gp=self.gp, bounds=self._bounds)
            _thetaN, _ = ut.minimize_objective(obj_fn, bounds=self._bounds, nopt=nopt, ps=self._prior_sampler,
                                               method=self.obj_opt_method, options=kw or None, grad_obj_fn=grad_obj_fn)
        opt_timing = time.time() - t0
        if not np.all(np.isfinite(_thetaN)):
            print("Warning: Acquisition function optimization failed. Falling back to random sampling.")
            _thetaN = ut.prior_sampler(bounds=self._bounds, nsample=1, random_state=self._seed()).flatten()
        thetaN = self.theta_scaler.inverse_transform(np.asarray(_thetaN).reshape(1, -1))
        yN = np.asarray(self.true_log_likelihood(thetaN.flatten()), dtype=np.float64).reshape(-1)
        if not np.all(np.isfinite(thetaN)) or not np.all(np.isfinite(yN)):
            print(f"New point is not finite: theta={thetaN}, y={yN}")
            return None, None, opt_timing
        theta_prop = np.append(self.theta(), thetaN, axis=0)
        y_prop = np.append(self.y(), yN)
        _theta_prop, _y_prop = self.refit_scalers(theta_prop, y_prop)
        if _theta_prop.shape[0] != _y_prop.shape[0]:
            return None, None, opt_timing
        return _theta_prop, _y_prop, opt_timing

    def active_train(self, niter=100, algorithm="bape", gp_opt_freq=20, save_progress=False,
                     obj_opt_method="scan", nopt=5, optimizer_kwargs={}, use_grad_opt=True,
                     show_progress=True, allow_opt_multiproc=True, max_attempts=10):
        """Active-learning loop: pick a point, evaluate the true function, refit (core.py:1670-1865)."""
        self.algorithm = str(algorithm).lower()
        self.utility, self.grad_utility = ut.assign_utility(self.algorithm)
        if not use_grad_opt:
            self.grad_utility = None
        if self.algorithm not in ("bape", "agp", "jones"):
            self.algorithm = "bape"
        self.gp_opt_freq = gp_opt_freq
        self.obj_opt_method = obj_opt_method
        self.use_grad_opt = bool(use_grad_opt)
        self.allow_opt_multiproc = bool(allow_opt_multiproc)    # several ranks: shard the candidate scan of find_next_point
        res = self.training_results
        first_iter = res["iteration"][-1] if len(res["iteration"]) else 0
        if self.verbose:
            print(f"Running {niter} active learning iterations using {self.algorithm}...")
        for ii in range(1, niter + 1):
            attempts, success = 0, False
            while not success:
                _theta_prop, _y_prop, opt_timing = self.find_next_point(nopt=nopt, optimizer_kwargs=optimizer_kwargs)
                if _theta_prop is None or _y_prop is None:
                    attempts += 1
                    if attempts >= max_attempts:
                        raise RuntimeError(f"Failed to find a valid training point after {max_attempts} attempts. "
                                           "Check your likelihood function and training data for issues or "
                                           "increase max_attempts.")
                    continue
                self.gp, fit_gp_timing = self._fit_gp(_theta=_theta_prop, _y=_y_prop,
                                                      hyperparameters=self.gp.get_parameter_vector())
                success = True
            self._theta, self._y = _theta_prop, _y_prop
            self.__dict__.pop("_gp_iter_memo", None)
            if (ii + first_iter) % self.gp_opt_freq == 0:
                self.gp, _ = self._opt_gp(**self.opt_gp_kwargs)
                res["gp_hyperparameter_opt_iteration"].append(ii + first_iter)
                if save_progress:
                    self.save()
            y_now = var_y_now = None                        # (self.y() un-scales the whole training set: once per iteration)
            try:
                _yp = self.gp.predict(_y_prop, _theta_prop, return_cov=False, return_var=False)
                yp = self.y_scaler.inverse_transform(_yp.reshape(-1, 1)).flatten()
                y_now = self.y(); var_y_now = np.var(y_now)
                training_mse = np.mean((y_now - yp) ** 2)
                training_scaled_mse = training_mse / var_y_now
            except Exception as e:  # noqa: BLE001
                print(f"Warning: Error evaluating GP training error at iteration {ii + first_iter}: {e}")
                training_mse = training_scaled_mse = np.nan
            test_mse = test_scaled_mse = np.nan
            if self.ntest > 0:
                try:
                    _yt = self.gp.predict(self._y, self._theta_test, return_cov=False, return_var=False)
                    yt = self.y_scaler.inverse_transform(_yt.reshape(-1, 1)).flatten()
                    yt_true = self.y_scaler.inverse_transform(self._y_test.reshape(-1, 1)).flatten()
                    test_mse = np.mean((yt_true - yt) ** 2)
                    test_scaled_mse = test_mse / (var_y_now if var_y_now is not None else np.var(self.y()))
                except Exception as e:  # noqa: BLE001
                    print(f"Warning: Error evaluating GP test error at iteration {ii + first_iter}: {e}")
            res["iteration"].append(ii + first_iter)
            res["gp_hyperparameters"].append(self.gp.get_parameter_vector())
            res["training_mse"].append(training_mse)
            res["test_mse"].append(test_mse)
            res["training_scaled_mse"].append(training_scaled_mse)
            res["test_scaled_mse"].append(test_scaled_mse)
            res["gp_kl_divergence"].append(np.nan)
            res["gp_train_time"].append(fit_gp_timing)
            res["obj_fn_opt_time"].append(opt_timing)
            self.ntrain = len(self._theta)
            self.nactive = self.ntrain - self.ninit_train
        if self.cache:
            self.save()

    # -------------------------------------------------------------------------------- MCMC
    def lnprob(self, theta):
        """log-posterior = like_fn(theta) + prior_fn(theta) (core.py:2073-2100)."""
        if getattr(self, "like_fn_name", "surrogate") == "surrogate" and not hasattr(self, "gp"):
            raise NameError("GP has not been trained")
        if not hasattr(self, "prior_fn"):
            raise NameError("prior_fn has not been specified")
        if not hasattr(self, "like_fn"):
            self.like_fn = self.surrogate_log_likelihood
        theta = np.asarray(theta).reshape(1, -1)
        return self.like_fn(theta) + self.prior_fn(theta)

    def find_map(self, theta0=None, prior_fn=None, method="nelder-mead", nRestarts=15, options=None):
        """Maximum of like_fn + prior_fn (alabi/core.py:2103; called by run_emcee(opt_init=True), core.py:2290-2294).

        The reference declares this entry point and raises NotImplementedError("Not implemented.") in its body, so
        ``opt_init=True`` cannot run there; here it works: ``nRestarts`` local optimisations (scipy ``method``) of
        -lnprob from the best points of a batched scan of the posterior (surrogate evaluated on the GPU, 4096 prior
        draws) and from ``theta0`` if given.  Sets ``self.map_theta`` / ``self.map_lnprob`` and returns the walker start
        positions run_emcee passes to the sampler: [nwalkers, ndim] in a ball of 1e-3 of the box width around the MAP,
        clipped into the open box.

        ``method="bfgs-gpu"`` (opt-in) runs every restart at once on the device instead: the starts -- the best ``nRestarts``
        points of the same scan, and ``theta0`` -- go to ``EnsembleSampler.maximize``, a projected BFGS ascent on the fused
        log-probability's closed-form gradient, one workgroup per start and all of it in one launch; the best converged result
        is taken (the best of any status, with a warning, if none converged).  It needs the fused log-probability of
        ``run_emcee`` (surrogate likelihood, box or shipped normal prior, foldable scalers) and raises ``ValueError`` naming what
        does not fuse otherwise.  ``options``: ``maxiter`` (200) and ``gtol`` (1e-8).  Sets ``map_status`` (0 converged, 1
        ``maxiter``, 2 no ascent) and ``map_evaluations`` (log-probability evaluations over all starts) as well."""
        if str(method).lower() == "bfgs-gpu":
            return self._find_map_gpu(theta0, prior_fn, nRestarts, options)
        prior_fn = prior_fn if prior_fn is not None else getattr(self, "prior_fn", None)
        if prior_fn is None:
            prior_fn = partial(ut.lnprior_uniform, bounds=self.bounds)
        like_fn = getattr(self, "like_fn", None) or self.surrogate_log_likelihood
        lo, hi = self.bounds[:, 0].astype(float), self.bounds[:, 1].astype(float)

        def lnp(th):
            th = np.asarray(th, dtype=np.float64).reshape(1, -1)
            pr = float(np.asarray(prior_fn(th)).reshape(-1)[0])
            if not np.isfinite(pr):
                return -np.inf
            v = float(np.asarray(like_fn(th)).reshape(-1)[0]) + pr
            return v if np.isfinite(v) else -np.inf

        cand = ut.prior_sampler(bounds=self.bounds, nsample=4096, sampler="uniform", random_state=self._seed())
        if like_fn != self.surrogate_log_likelihood:     # row by row on the host; the surrogate: one batched GPU predict
            cand = cand[:256]
        like_c = post.host_likelihood(like_fn, self.surrogate_log_likelihood, (1, -1))(cand)
        post_c = like_c + post.host_rows(prior_fn, (1, -1))(cand)
        post_c = np.where(np.isfinite(post_c), post_c, -np.inf)
        starts = [cand[i] for i in np.argsort(-post_c)[:max(int(nRestarts), 1)]]
        if theta0 is not None:
            starts.insert(0, np.asarray(theta0, dtype=np.float64).reshape(-1))
        best_x, best_f = starts[0], lnp(starts[0])
        eps = 1e-9 * (hi - lo)
        use_bounds = method.lower() in ("nelder-mead", "l-bfgs-b", "tnc", "powell", "slsqp", "trust-constr")
        for x0 in starts[:max(int(nRestarts), 1)]:
            try:
                res = op.minimize(lambda x: (lambda v: -v if np.isfinite(v) else 1e25)(lnp(x)), x0, method=method, options=options,
                                  bounds=list(zip(lo + eps, hi - eps)) if use_bounds else None)
            except Exception:  # noqa: BLE001
                continue
            f = lnp(res.x)
            if np.isfinite(f) and f > best_f:
                best_x, best_f = np.asarray(res.x, dtype=np.float64), f
        self.map_theta, self.map_lnprob = best_x, best_f
        nw = int(getattr(self, "nwalkers", 10 * self.ndim))
        ball = best_x + 1e-3 * (hi - lo) * self._rng.standard_normal((nw, self.ndim))
        return np.minimum(np.maximum(ball, lo + 1e-9 * (hi - lo)), hi - 1e-9 * (hi - lo))

    def _find_map_gpu(self, theta0, prior_fn, nRestarts, options):
        """find_map(method="bfgs-gpu"): see there.  Leaves the sampler and its plan in ``_map_sampler`` / ``_map_plan`` and the
        maximum in the sampler's coordinates in ``_map_coords`` for ``laplace_approximation``."""
        if not hasattr(self, "gp"):
            raise NameError("GP has not been trained")
        like_fn = getattr(self, "like_fn", None) or self.surrogate_log_likelihood
        like_host = None if like_fn == self.surrogate_log_likelihood else like_fn
        prior_fn = prior_fn if prior_fn is not None else getattr(self, "prior_fn", None)
        plan = post.plan_ensemble(like_host, self.surrogate_log_likelihood, prior_fn, self.bounds,
                                  getattr(self, "theta_scaler", None), getattr(self, "y_scaler", None), getattr(self, "_y", None))
        if not plan.fused:
            why = []
            if plan.host_like is not None:
                why.append("the likelihood runs on the host (like_fn is not the surrogate, or a scaler cannot be folded into the kernels)")
            if plan.host_prior is not None:
                why.append("prior_fn is a host callable (only the box and the shipped lnprior_normal fuse)")
            raise ValueError('find_map(method="bfgs-gpu") needs the fused log-probability: host callables (prior_fn / like_fn) have no '
                             "gradient -- " + "; ".join(why))
        opts = dict(options or {})
        lo, hi = self.bounds[:, 0].astype(float), self.bounds[:, 1].astype(float)
        cand = ut.prior_sampler(bounds=self.bounds, nsample=4096, sampler="uniform", random_state=self._seed())
        post_c = np.asarray(self.surrogate_log_likelihood(cand), dtype=np.float64).reshape(-1)
        if prior_fn is not None and plan.normal_prior is not None:   # (the box prior is 0 at every draw)
            post_c = post_c + post.host_rows(prior_fn, (1, -1))(cand)
        post_c = np.where(np.isfinite(post_c), post_c, -np.inf)
        starts = [cand[i] for i in np.argsort(-post_c)[:max(int(nRestarts), 1)]]
        if theta0 is not None:
            starts.insert(0, np.asarray(theta0, dtype=np.float64).reshape(-1))
        gp_obj, y_obj = self._handle_owner()
        sampler = EnsembleSampler(2, self.ndim, gp_obj, y_obj, plan.box, logp_affine=plan.logp_affine, normal_prior=plan.normal_prior,
                                  logp_map=plan.logp_map, live_dangerously=True, seed=0)
        res = sampler.maximize(np.asarray(starts) * plan.t_mult + plan.t_add, maxiter=int(opts.get("maxiter", 200)),
                               gtol=float(opts.get("gtol", 1e-8)))
        status, lp, x = res.status.cpu().numpy(), res.log_prob.cpu().numpy(), res.x.cpu().numpy()
        usable = np.isfinite(lp) & (status != 3)
        if not usable.any():
            raise RuntimeError('find_map(method="bfgs-gpu"): no start lies inside the prior box with a finite log-probability')
        pick = usable & (status == 0)
        if not pick.any():
            warnings.warn('find_map(method="bfgs-gpu"): no restart converged (statuses %s); taking the best point reached'
                          % sorted(set(status[usable].tolist())), UserWarning, stacklevel=3)
            pick = usable
        best = int(np.flatnonzero(pick)[np.argmax(lp[pick])])
        self._map_sampler, self._map_plan, self._map_coords = sampler, plan, x[best].copy()
        self.map_theta = np.asarray(plan.to_theta(x[best][None, :]), dtype=np.float64).reshape(-1)
        self.map_lnprob = float(lp[best])
        self.map_status = int(status[best])
        self.map_evaluations = int(res.evaluations.sum().item())
        nw = int(getattr(self, "nwalkers", 10 * self.ndim))
        ball = self.map_theta + 1e-3 * (hi - lo) * self._rng.standard_normal((nw, self.ndim))
        return np.minimum(np.maximum(ball, lo + 1e-9 * (hi - lo)), hi - 1e-9 * (hi - lo))

    def laplace_approximation(self, theta0=None, nRestarts=64, prior_fn=None):
        """The Laplace approximation of the surrogate posterior: ``find_map(method="bfgs-gpu")`` from ``nRestarts`` starts (and
        ``theta0``), then ONE closed-form Hessian of the fused log-probability at the maximum
        (``EnsembleSampler.log_prob_hessian``), then ``alabi_amd.laplace``.  Sets

        * ``map_theta``, ``map_lnprob``, ``map_status``, ``map_evaluations`` as ``find_map`` does;
        * ``map_hessian`` [d, d] in theta, ``map_cov`` = (-map_hessian)^-1 in theta, and ``map_cov_scaled``, the same covariance
          in the sampler's coordinates -- the form ``GaussianMove`` / ``HMCMove`` take:
          ``sm.run_emcee(sampler_kwargs={"moves": HMCMove(sm.map_cov_scaled, n_leapfrog=4)})``;
        * ``laplace_logz`` = lp + (d / 2) ln 2 pi - ln det(-H) / 2 - sum ln width over the coordinates under the uniform prior
          (``lnprior_uniform`` is 0 in the box, ``run_dynesty``'s prior transform is normalised): a cross-check of
          ``run_dynesty``'s log Z in a few milliseconds (NOTES.md "MAP and Laplace");
        * ``map_on_bound``, a boolean mask of the coordinates the maximum holds on a wall of the box.

        Where a coordinate is held on a bound, or -H is not positive definite there, the covariances and ``laplace_logz`` are
        None and a ``UserWarning`` says which: a Gaussian at a wall is not a Laplace approximation.  Returns ``laplace_logz``."""
        from . import laplace as lap
        self.find_map(theta0=theta0, prior_fn=prior_fn, method="bfgs-gpu", nRestarts=nRestarts)
        plan, xc = self._map_plan, self._map_coords
        H = self._map_sampler.log_prob_hessian(xc[None, :])[0].cpu().numpy()
        w = plan.box[:, 1] - plan.box[:, 0]
        self.map_on_bound = (xc <= plan.box[:, 0] + 1e-9 * w) | (xc >= plan.box[:, 1] - 1e-9 * w)
        self.map_hessian = lap.hessian_to_theta(H, plan.t_mult)
        self.map_cov = self.map_cov_scaled = self.laplace_logz = None
        if self.map_on_bound.any():
            warnings.warn("laplace_approximation: the maximum holds coordinate(s) %s on a wall of the prior box; no covariance and no "
                          "evidence estimate are set" % np.flatnonzero(self.map_on_bound).tolist(), UserWarning, stacklevel=2)
            return None
        cov = lap.laplace_covariance(H)
        if cov is None:
            warnings.warn("laplace_approximation: minus the Hessian at the point found is not positive definite (status %d: not a "
                          "maximum); no covariance and no evidence estimate are set" % self.map_status, UserWarning, stacklevel=2)
            return None
        uniform = np.ones(self.ndim, dtype=bool) if plan.normal_prior is None else \
            ~(np.isfinite(plan.normal_prior[0]) & np.isfinite(plan.normal_prior[1]) & (plan.normal_prior[1] > 0))
        widths = (plan.theta_box[:, 1] - plan.theta_box[:, 0])[uniform]
        self.map_cov_scaled = cov
        self.map_cov = lap.covariance_to_theta(cov, plan.t_mult)
        self.laplace_logz = lap.laplace_log_evidence(self.map_lnprob, self.map_hessian, widths)
        return self.laplace_logz

    # ---- what run_emcee and run_dynesty share
    def _handle_owner(self):
        """(gp, y) a sampler is built on: ``self.gp`` carrying the latest hyper-parameters / data, or -- like_fn="true" before any GP
        exists -- a bare HipGP, because the device handle needs an owner only."""
        if not hasattr(self, "gp"):
            return HipGP(self.ndim), np.zeros(1)
        if len(self.training_results["iteration"]) > 0:
            self.eval_gp_at_iteration(-1)
        return self.gp, self._y

    def _write_samples(self, sampler, samples, samples_file, **more):
        """After a sampler run (the caller lets rank 0 only through): the cached model, quietly, and the .npz of samples (and of
        ``more`` arrays), whose name is returned."""
        if self.cache:
            try:
                self.save()
            except Exception:  # noqa: BLE001
                pass
        if samples_file is not None:
            fname = f"{self.savedir}/{samples_file}"
        elif self.like_fn_name == "true":
            fname = f"{self.savedir}/{sampler}_samples_final_{self.like_fn_name}.npz"
        else:
            res = getattr(self, "training_results", {"iteration": []})
            it = res["iteration"][-1] if len(res["iteration"]) else 0
            fname = f"{self.savedir}/{sampler}_samples_final_{self.like_fn_name}_iter_{it}.npz"
        np.savez(fname, samples=samples, **more)
        return fname

    def run_emcee(self, like_fn=None, prior_fn=None, nwalkers=None, nsteps=int(5e4), sampler_kwargs={}, run_kwargs={},
                  opt_init=False, multi_proc=True, prior_fn_comment=None, burn=None, thin=None, samples_file=None,
                  min_ess=int(1e4)):
        """Ensemble MCMC on the posterior like_fn + prior_fn, on the GPU (core.py:2108-2414).

        * Fused path (the reference's defaults and the priors it ships): like_fn None / "surrogate" / "gp", prior_fn None,
          ``partial(lnprior_uniform, bounds=...)`` or ``partial(lnprior_normal, bounds=..., data=...)``, affine theta
          scaler, y scaler affine or one of the shipped ``nlog_scaler`` / ``log_scaler``: the whole log-probability is
          evaluated inside the ensemble kernels.
        * Any other ``prior_fn`` callable (core.py:2253-2280; docstring example :2236-2239): the device proposes and
          evaluates the surrogate part of every half step, the host adds ``prior_fn(theta)`` per proposal, the device
          does the accept test (alabi_ens_propose / alabi_ens_accept).
        * ``like_fn="true"`` or a callable, or scalers that are neither of the above: the same split with the
          likelihood evaluated on the host as well (walkers then move in the original theta coordinates).
        ``opt_init=True`` starts the walkers around ``find_map()``.

        ``sampler_kwargs["moves"]`` (the reference's "Custom proposal moves", core.py:2144): None for the stretch move, or
        ``alabi_amd.moves.StretchMove`` / ``DEMove`` objects (emcee's own are recognised) or ``alabi_amd.moves.SnookerMove``
        (the snooker update of ter Braak & Vrugt 2008; ``nwalkers >= 6``), a list of them, or a list of (move, weight) pairs --
        one move is chosen per step.  Multimodal posteriors want ``[(DEMove(), 0.9), (DEMove(gamma0=1.0), 0.1)]``: the stretch
        move alone does not cross between separated modes; the usual companion of DE is ``[(DEMove(), 0.8), (SnookerMove(),
        0.2)]``.  ``alabi_amd.moves.WalkMove(s=None)`` and ``KDEMove(bw_method=None)`` (emcee's own are recognised) use the whole
        complementary half: a KDE move hops between modes in one step, ``[(KDEMove(), 0.3), (DEMove(), 0.7)]``, and wants many
        walkers per dimension (``nwalkers >= 2 ndim + 2`` at the least; a warning below ``8 (ndim + 1)``).
        ``alabi_amd.moves.GaussianMove(cov, mode="vector", factor=None)`` is emcee's Gaussian Metropolis move -- ``cov`` a scalar, a
        vector of variances or a matrix, e.g. ``map_cov_scaled`` of ``laplace_approximation()`` (the inverse Hessian at the MAP:
        ``run_emcee(sampler_kwargs={"moves": HMCMove(sm.map_cov_scaled, n_leapfrog=4)})``) or the covariance of an earlier chain: a set of
        Gaussian moves alone runs the walkers as independent random-walk Metropolis chains on the surrogate, any number of them,
        all steps of a call in one kernel launch; it mixes with the red-blue moves too.  ``alabi_amd.moves.MHMove(fn)`` and any
        object with a callable ``get_proposal`` (emcee's own ``MHMove`` / ``GaussianMove``) run a Python proposal function on a
        host-driven loop, one round trip per step: slow by nature.  ``alabi_amd.moves.HMCMove(cov, step_size=None, n_leapfrog=8,
        jitter=None)`` runs Hamiltonian Monte Carlo on the surrogate's closed-form gradient (``n_leapfrog=1``: MALA), alone or as
        a mixture of HMC moves; ``cov`` is given in the sampler's (scaled) coordinates like a ``GaussianMove``'s; it needs the
        surrogate likelihood with a prior that fuses (none, uniform or normal) and cannot be sharded.  With a single ``HMCMove``,
        ``sampler_kwargs["hmc_warmup"] = n`` (optionally ``"hmc_target_accept"``, default 0.8, and ``"hmc_metric"``: "diag", "dense" or
        None) runs ``EnsembleSampler.tune_hmc`` for n steps in front of the run -- Stan-style warm-up of the step size and the mass
        matrix; what it found is ``sm.hmc_tuning`` --; with any other move set these keys raise ``ValueError``.  ``alabi_amd.moves.NUTSMove(cov,
        step_size=None, max_depth=8, jitter=None)`` is the No-U-Turn sampler on the same gradient under the same restrictions: the
        trajectory length is chosen per transition; ``sm.nuts_stats`` says afterwards how deep the trees went.  With a single ``NUTSMove``,
        ``sampler_kwargs["nuts_warmup"] = n`` (optionally ``"nuts_target_accept"``, default 0.8, ``"nuts_metric"``: "diag", "dense" or None,
        and ``"nuts_init_step_size"``: "search" or None) runs ``EnsembleSampler.tune_nuts`` for n transitions in front of the run --
        Stan's step-size search, dual averaging on the tree's mean acceptance statistic and the windowed mass matrix; what it found
        is ``sm.nuts_tuning`` --; with any other move set these keys raise ``ValueError``, as the ``hmc_*`` keys do with a ``NUTSMove``.  Any other emcee move raises ``NotImplementedError`` -- in
        particular emcee's ``DESnookerMove``, whose arithmetic is not the published rule; none of ``DEMove``, ``SnookerMove``,
        ``WalkMove``, ``KDEMove``, ``GaussianMove``, ``MHMove`` can be combined with ``"shard": True``.

        Several GPUs (the reference's parallel axis is a process pool handed to emcee, core.py:2300, :2322, built at :349-369;
        ``ncore`` / ``pool_method`` have no meaning here): run one process per GPU under ``torch.distributed`` (e.g.
        ``python -m torch.distributed.run --nproc-per-node 8 script.py``, backend "nccl" = RCCL) and have every rank make the
        same calls.  With ``multi_proc=True`` and more than one rank
          * default -- REPLICAS: every rank runs its own ensemble of ``nwalkers`` walkers (sampler seed + rank, its own start
            points), no communication inside the run; after each run the flattened samples of all ranks are concatenated on
            every rank (``emcee_samples`` is identical everywhere) and ``min_ess`` counts the samples of all ranks;
          * ``sampler_kwargs={"shard": True}`` -- ONE ensemble whose active half is partitioned over the ranks, an RCCL
            all-gather of the new walker rows per half step (alabi_amd.dist.ShardedRun); every rank holds the same chain.
        Files (the .npz of samples, the cached model) are written by rank 0 only."""
        from . import dist as adist
        rank, world = adist.world_info()
        kw = dict(sampler_kwargs)
        move_set = parse_moves(kw.get("moves"), self.ndim)       # unsupported moves fail here, before anything runs
        # HMC warm-up (EnsembleSampler.tune_hmc) in front of every run: popped here, the sampler's constructor does not know them
        hmc_warmup = kw.pop("hmc_warmup", None)
        hmc_tune_kw = {name: kw.pop(key) for key, name in (("hmc_target_accept", "target_accept"), ("hmc_metric", "metric")) if key in kw}
        if hmc_warmup is not None or hmc_tune_kw:
            if move_set is not None and move_set.has_nuts:
                raise ValueError('sampler_kwargs "hmc_warmup", "hmc_target_accept" and "hmc_metric" adapt an HMCMove, not a NUTSMove: a '
                                 'NUTSMove has "nuts_warmup" (EnsembleSampler.tune_nuts).  The older route still works -- tune an HMCMove '
                                 'first, then pass NUTSMove(sm.hmc_tuning["cov"], step_size=sm.hmc_tuning["step_size"])')
            if move_set is None or len(move_set) != 1 or not move_set.all_hmc:
                raise ValueError('sampler_kwargs "hmc_warmup", "hmc_target_accept" and "hmc_metric" need sampler_kwargs["moves"] to be '
                                 'a single HMCMove: its step size and mass matrix are what the warm-up adapts')
            if hmc_warmup is None or int(hmc_warmup) < 1:
                raise ValueError('sampler_kwargs["hmc_warmup"] must be a positive number of warm-up steps')
            hmc_warmup = int(hmc_warmup)
        # NUTS warm-up (EnsembleSampler.tune_nuts), likewise
        nuts_warmup = kw.pop("nuts_warmup", None)
        nuts_tune_kw = {name: kw.pop(key) for key, name in (("nuts_target_accept", "target_accept"), ("nuts_metric", "metric"),
                                                            ("nuts_init_step_size", "init_step_size")) if key in kw}
        if nuts_warmup is not None or nuts_tune_kw:
            if move_set is None or len(move_set) != 1 or not move_set.all_nuts:
                raise ValueError('sampler_kwargs "nuts_warmup", "nuts_target_accept", "nuts_metric" and "nuts_init_step_size" need '
                                 'sampler_kwargs["moves"] to be a single NUTSMove: its step size and mass matrix are what the warm-up '
                                 'adapts (an HMCMove has "hmc_warmup")')
            if nuts_warmup is None or int(nuts_warmup) < 1:
                raise ValueError('sampler_kwargs["nuts_warmup"] must be a positive number of warm-up transitions')
            nuts_warmup = int(nuts_warmup)
        if kw.get("shard", False) and move_set is not None and (move_set.has_gauss or move_set.all_mh):
            raise ValueError('sampler_kwargs={"shard": True} cannot run a GaussianMove or an MHMove: a Metropolis proposal reads no '
                             'other walker, so there is nothing to exchange -- run replicas instead')
        if kw.get("shard", False) and move_set is not None and (move_set.has_hmc or move_set.has_nuts):
            raise ValueError('sampler_kwargs={"shard": True} cannot run an HMCMove or a NUTSMove: the sharded form is not built -- run '
                             'replicas instead')
        if kw.get("shard", False) and move_set is not None and move_set.multi_partner:
            raise ValueError('sampler_kwargs={"shard": True} cannot run a DEMove or a SnookerMove: the sharded ensemble links one '
                             'partner row per proposal')
        shard = bool(kw.pop("shard", False)) and bool(multi_proc) and world > 1
        replicas = bool(multi_proc) and world > 1 and not shard
        # ---- likelihood
        if like_fn is None or (isinstance(like_fn, str) and like_fn.lower() in ("surrogate", "gp")):
            self.like_fn_name, self.like_fn = "surrogate", self.surrogate_log_likelihood
            if not hasattr(self, "gp"):
                raise NameError("GP has not been trained")
        elif isinstance(like_fn, str) and like_fn.lower() == "true":
            self.like_fn_name, self.like_fn = "true", self.true_log_likelihood
        elif callable(like_fn):
            self.like_fn_name, self.like_fn = "likelihood", like_fn
        else:
            raise ValueError("like_fn must be None, 'surrogate', 'gp', 'true' or a callable")
        like_host = None if self.like_fn_name == "surrogate" else self.like_fn     # on theta; None: the device surrogate
        # ---- plan: None (uniform box) or one of the two shipped priors fuse into the kernel; anything else is a host call
        plan = post.plan_ensemble(like_host, self.surrogate_log_likelihood, prior_fn, self.bounds,
                                  getattr(self, "theta_scaler", None), getattr(self, "y_scaler", None), getattr(self, "_y", None))
        sampler_extra = {} if plan.fused else dict(prior_fn=plan.host_prior, like_fn=plan.host_like,
                                                   gate_box=plan.host_prior is None)
        self.prior_fn = partial(ut.lnprior_uniform, bounds=self.bounds) if prior_fn is None else prior_fn
        self.prior_fn_comment = ("Default uniform prior. \nPrior function: ut.prior_fn_uniform\n"
                                 f"\twith bounds {self.bounds}") if prior_fn_comment is None else prior_fn_comment
        self.nwalkers = int(10 * self.ndim) if nwalkers is None else int(nwalkers)
        self.nsteps = int(nsteps)
        gp_obj, y_obj = self._handle_owner()
        if shard and not plan.fused:
            raise ValueError('sampler_kwargs={"shard": True} needs the fused log-probability (surrogate likelihood, shipped priors '
                             'and scalers); host callables run as replicas')
        if opt_init:
            p0 = self.find_map(prior_fn=self.prior_fn)           # core.py:2290-2292
        else:
            p0_seed = self._seed()                               # (drawn on every rank alike: the model's stream stays in step)
            p0 = ut.prior_sampler(nsample=self.nwalkers, bounds=plan.theta_box, sampler="uniform",
                                  random_state=p0_seed + (1000003 * rank if replicas else 0))
        p0 = p0 * plan.t_mult + plan.t_add         # walkers live in scaled coordinates
        if self.verbose:
            print(f"Running emcee-style ensemble on the GPU with {self.nwalkers} walkers for {self.nsteps} steps...")
        self.emcee_runtime = 0.0
        kw.setdefault("seed", self._seed())
        if replicas:
            kw["seed"] = int(kw["seed"]) + rank
        if shard:
            kw["shard"] = True

        def run(run_number):
            start = p0
            if run_number > 1:
                start = self.emcee_sampler.get_last_sample().coords
                kw["seed"] = self._seed() + (rank if replicas else 0)
            t0 = time.time()
            self.emcee_sampler = EnsembleSampler(self.nwalkers, self.ndim, gp_obj, y_obj, plan.box, logp_affine=plan.logp_affine,
                                                 normal_prior=plan.normal_prior, logp_map=plan.logp_map, **sampler_extra, **kw)
            if hmc_warmup is not None:
                start = self.emcee_sampler.tune_hmc(start, nwarmup=hmc_warmup, **hmc_tune_kw).coords
                self.hmc_tuning = self.emcee_sampler.hmc_tuning
            if nuts_warmup is not None:
                start = self.emcee_sampler.tune_nuts(start, nwarmup=nuts_warmup, **nuts_tune_kw).coords
                self.nuts_tuning = self.emcee_sampler.nuts_tuning
            self.emcee_sampler.run_mcmc(start, self.nsteps, **run_kwargs)
            self.nuts_stats = getattr(self.emcee_sampler, "nuts_stats", None)      # None without a NUTSMove
            self.emcee_runtime += time.time() - t0
            self.iburn, self.ithin = mcmc_utils.estimate_burnin(self.emcee_sampler, verbose=self.verbose)
            self.burn = burn if burn is not None else self.iburn
            self.thin = thin if thin is not None else self.ithin
            cur = plan.to_theta(self.emcee_sampler.get_chain(discard=self.burn, thin=self.thin, flat=True))
            return adist.gather_replicas(cur) if replicas else cur   # every rank's kept samples, in rank order, on every rank

        self.emcee_samples = post.run_until_min_ess(run, min_ess, (lambda total: f" (total {total})") if self.verbose else None)
        self._emcee_full, self._emcee_full_src = None, (self.emcee_sampler, plan.t_add, plan.t_mult)   # emcee_samples_full: lazily
        self._emcee_affine = (plan.t_add, plan.t_mult)                # mcmc_diagnostics reports in theta coordinates
        if self.like_fn_name == "true":
            self.emcee_samples_true = self.emcee_samples
        elif self.like_fn_name == "surrogate":
            self.emcee_samples_gp = self.emcee_samples
        self.acc_frac = np.mean(self.emcee_sampler.acceptance_fraction)
        self.autcorr_time = np.mean(self.emcee_sampler.get_autocorr_time(tol=0))
        if replicas:                                             # the same numbers on every rank: the mean over the ensembles
            both = adist.allreduce_array([self.acc_frac, self.autcorr_time], "sum") / world
            self.acc_frac, self.autcorr_time = float(both[0]), float(both[1])
        self.emcee_ranks = world if (replicas or shard) else 1
        self.emcee_mode = "replicas" if replicas else ("sharded" if shard else "single")
        if self.verbose:
            print(f"Total samples: {self.emcee_samples.shape[0]}")
            print("Mean acceptance fraction: {0:.3f}".format(self.acc_frac))
            print("Mean autocorrelation time: {0:.3f} steps".format(self.autcorr_time))
        self.emcee_run = True
        if (replicas or shard) and rank != 0:
            return                                               # files are rank 0's
        self._write_samples("emcee", self.emcee_samples, samples_file)

    run_mcmc = run_emcee  # BASELINE.json's name for the same entry point

    def mcmc_diagnostics(self, discard=None, thin=1):
        """Chain diagnostics of the last run_emcee (Vehtari et al. 2021; alabi_amd/diagnostics.py): a dict of [ndim] arrays mean,
        sd, mcse_mean (in theta coordinates), ess_mean, ess_bulk, ess_tail and rhat of the chain after ``discard`` steps (None:
        ``self.burn``), every ``thin``-th step; also stored as ``self.emcee_diagnostics``.  The chain is judged where it lies, on
        the device.  Every walker counts as a chain: walkers are independent under the metropolis, hmc and nuts moves; under the
        red-blue ensemble moves (the default stretch move among them) the walkers of one ensemble are coupled -- R-hat still
        detects disagreement, but the ESS formula assumes independent chains and is approximate there."""
        if not getattr(self, "emcee_run", False) or getattr(self, "emcee_sampler", None) is None:
            raise AttributeError("mcmc_diagnostics: run_emcee has not been called")
        out = self.emcee_sampler.diagnostics(discard=int(self.burn if discard is None else discard), thin=int(thin))
        t_add, t_mult = self._emcee_affine                         # sampler coordinates = t_mult * theta + t_add
        out["mean"] = (out["mean"] - t_add) / t_mult
        out["sd"] = out["sd"] / np.abs(t_mult)
        out["mcse_mean"] = out["mcse_mean"] / np.abs(t_mult)
        self.emcee_diagnostics = out
        return out

    # ------------------------------------------------------------------------ nested sampling
    def _nested_setup(self, like_fn, prior_transform, prior_transform_comment):
        """What run_dynesty and run_pymultinest share: resolves ``like_fn`` and ``prior_transform`` as the reference does
        (core.py:2533-2598, :2977-3025) into ``like_fn_name`` / ``like_fn`` / ``prior_transform`` / ``prior_transform_comment``, and
        returns (plan, gp, y): fused device likelihood, or the host evaluates like_fn(prior_transform(u))."""
        # ---- likelihood (core.py:2533-2573)
        if like_fn is None or (isinstance(like_fn, str) and like_fn.lower() in ("surrogate", "gp", "surrogate_log_likelihood")) \
                or (callable(like_fn) and like_fn == self.surrogate_log_likelihood):
            self.like_fn_name, self.like_fn = "surrogate", self.surrogate_log_likelihood
        elif (isinstance(like_fn, str) and like_fn.lower() in ("true", "true_log_likelihood")) or \
                (callable(like_fn) and like_fn == self.true_log_likelihood):
            self.like_fn_name, self.like_fn = "true", self.true_log_likelihood
        elif callable(like_fn):
            self.like_fn_name, self.like_fn = "custom", like_fn
        elif isinstance(like_fn, str):
            raise ValueError(f"Unknown string identifier for like_fn: '{like_fn}'. "
                             "Valid options: 'surrogate', 'true', 'gp', 'surrogate_log_likelihood', 'true_log_likelihood'")
        else:
            raise TypeError(f"like_fn must be None, a string, or a callable function. Received type: {type(like_fn)}")
        if self.like_fn_name == "surrogate" and not hasattr(self, "gp"):
            raise NameError("GP has not been trained")
        # ---- prior transform (core.py:2575-2598)
        if prior_transform is None:
            self.prior_transform = partial(ut.prior_transform_uniform, bounds=self.bounds)
            self.prior_transform_comment = ("Default uniform prior transform. \nPrior function: ut.prior_transform_uniform\n"
                                            f"\twith bounds {self.bounds}")
        else:
            self.prior_transform = prior_transform
            self.prior_transform_comment = prior_transform_comment
            if prior_transform_comment is None:
                self.prior_transform_comment = ("User defined prior transform."
                                                f"Prior function: {getattr(prior_transform, '__name__', 'unrecorded')}")
        plan = post.plan_nested(self.like_fn, self.surrogate_log_likelihood, self.prior_transform, self.bounds,
                                getattr(self, "theta_scaler", None), getattr(self, "y_scaler", None), getattr(self, "_y", None))
        return plan, *self._handle_owner()

    def _nested_runs(self, name, label, setup, seed, make_sampler, run_args, min_ess, note, collect, t0, samples_file,
                     file_fields=(), custom_is_surrogate=True, checkpoint=None):
        """The runs and the tail of run_dynesty / run_pymultinest / run_ultranest, whose attributes start with ``name``.  Run k takes
        the seed (``seed`` + 1000003 (k - 1), or the model's seed stream when None) + rank, builds a GPUWalkBackend from ``setup``
        (the result of ``_nested_setup``) and ``make_sampler(backend, seed)`` on it, runs ``run_nested(**run_args)`` and resamples to
        equal weights; ``collect(results, samples)`` keeps what the front end combines over its runs (it sets the log Z attributes
        from the runs so far), ``checkpoint(sampler, k)`` makes run_dynesty's ``save_iter`` callable.  Runs repeat until ``min_ess``
        samples exist.  Rank 0 then writes the samples with the ``name``_``file_fields`` attributes."""
        from . import dist as adist
        from .nested import GPUWalkBackend
        rank, _ = adist.world_info()
        plan, gp_obj, y_obj = setup
        normal = {} if plan.normal_prior is None else {"normal_prior": plan.normal_prior}     # Gaussian prior coordinates

        def run(run_number):
            s = (self._seed() if seed is None else int(seed) + 1000003 * (run_number - 1)) + rank
            backend = GPUWalkBackend(gp_obj, y_obj, plan.box, seed=s, to_theta=plan.to_theta, logp_affine=plan.logp_affine,
                                     logp_map=plan.logp_map, host_loglike=plan.host_like, **normal)
            sampler = make_sampler(backend, s)
            setattr(self, f"{name}_sampler", sampler)
            cp = checkpoint(sampler, run_number) if checkpoint is not None and rank == 0 else None
            res = sampler.run_nested(**run_args, **({} if checkpoint is None else {"checkpoint": cp}))
            if cp is not None:
                cp.write(res)
            backend.close()
            setattr(self, f"{name}_results", res)
            setattr(self, f"{name}_path", backend.path)
            eq = res.samples_equal(np.random.default_rng(s))
            collect(res, eq)
            return eq

        samples = post.run_until_min_ess(run, min_ess, note if self.verbose else None)
        setattr(self, f"{name}_samples", samples)
        if self.like_fn_name == "true":
            setattr(self, f"{name}_samples_true", samples)
        elif self.like_fn_name == "surrogate" or custom_is_surrogate:
            setattr(self, f"{name}_samples_surrogate", samples)
        setattr(self, f"{name}_run", True)
        setattr(self, f"{name}_runtime", time.time() - t0)
        if rank != 0:
            return                                   # files are rank 0's
        fname = self._write_samples(name, samples, samples_file, **{k: getattr(self, f"{name}_{k}") for k in file_fields})
        if self.verbose:
            print(f"Saved {label} samples to {fname}")

    def run_dynesty(self, like_fn=None, prior_transform=None, mode="dynamic", sampler_kwargs={}, run_kwargs={},
                    multi_proc=False, save_iter=None, prior_transform_comment=None, samples_file=None, min_ess=int(1e4)):
        """Nested sampling of the posterior and its evidence log Z on the GPU (core.py:2417-2787); the sampler is
        alabi_amd.nested.NestedSampler (its docstring states the algorithm) in place of dynesty's.

        * Fused path: the surrogate likelihood (like_fn None / "surrogate" / "gp"), prior_transform None,
          ``partial(ut.prior_transform_uniform, bounds=...)`` or ``partial(ut.prior_transform_normal, bounds=..., data=...)``
          (Gaussian priors: the inverse normal CDF inside the kernels, not truncated to the bounds, as in the reference),
          affine theta scaler, affine / nlog / log y scaler: every walk step evaluates the GP mean inside ``ns_walk_kernel``.
        * Otherwise (like_fn "true" or a callable, any other prior_transform, scalers the kernel cannot fold) the device proposes
          and accepts, and the host evaluates ``like_fn(prior_transform(u))`` row by row with 1-D arrays of shape (d,), as
          dynesty calls them (the surrogate under exotic scalers takes the whole batch in one call, and so does the
          ``prior_transform_normal`` partial).
        sampler_kwargs: ``nlive`` (50 ndim), ``sample`` ("auto" / "rwalk": ``walks`` (25) Metropolis steps per walk; "rslice":
        ``slices`` (3 (3 + ndim)) random-direction slice updates per walk, 5-15 times the likelihood evaluations of the random
        walk), ``batch`` (ceil(nlive / 4)), ``seed``.  Above ndim = 20 pass ``sample="rslice"``: 25 random-walk steps no longer
        forget the start point there, and log Z comes out too high by several logzerr ("auto" stays the random walk at every
        dimension).  ``sample="unif"`` is not reached from here (it raises ``NotImplementedError``): uniform draws inside bounding
        ellipsoids are ``run_pymultinest``'s move, and ``alabi_amd.nested.NestedSampler(sample="unif")`` directly.
        ``bound``, ``pool``, ``queue_size`` and ``multi_proc`` have no effect.  run_kwargs: ``dlogz`` (0.5),
        ``maxiter`` (5e4), ``maxcall``, and for mode="dynamic" ``dlogz_init`` (0.5), ``nlive_init``, ``nlive_batch``,
        ``maxbatch`` (10), ``n_effective`` (1e4), ``wt_kwargs`` / ``stop_kwargs`` (pfrac = 1.0 only).  Under
        ``torch.distributed`` every rank runs its own sampler (seed + rank) and rank 0 writes the files."""
        from .nested import NestedSampler, PickleCheckpoint
        dynesty_t0 = time.time()
        # ---- sampler / run settings (core.py:2603-2649)
        skw = dict(sampler_kwargs)
        nlive = int(skw.pop("nlive", 50 * self.ndim))
        sample = skw.pop("sample", "auto")
        if sample not in ("auto", "rwalk", "rslice"):
            raise NotImplementedError(f"sample={sample!r}: only the random walk ('auto' / 'rwalk') and random-direction slice "
                                      "sampling ('rslice') are built")
        walks = int(skw.pop("walks", 25))
        slices = skw.pop("slices", None)
        move = {"sample": "rslice", "slices": slices} if sample == "rslice" else {}     # the random walk: the sampler's defaults
        batch = skw.pop("batch", None)
        seed = skw.pop("seed", None)
        for k in ("bound", "pool", "queue_size", "first_update", "update_interval", "bootstrap", "enlarge"):
            skw.pop(k, None)                         # bounding / process-pool settings: no effect here
        if skw:
            raise TypeError(f"run_dynesty: unsupported sampler_kwargs {sorted(skw)}")
        if mode not in ("dynamic", "static"):
            raise ValueError(f"mode {mode} is not a valid option. Choose 'dynamic' or 'static'.")
        rkw = {"wt_kwargs": {"pfrac": 1.0}, "stop_kwargs": {"pfrac": 1.0}, "maxiter": int(5e4), "dlogz_init": 0.5}
        rkw.update(run_kwargs)
        rkw.pop("print_progress", None)
        if mode == "static":                         # dynamic-only settings (the reference hands them to dynesty in both modes)
            for k in ("wt_kwargs", "stop_kwargs", "dlogz_init", "nlive_init", "nlive_batch", "maxbatch", "n_effective"):
                rkw.pop(k, None)
        allowed = {"dlogz", "maxiter", "maxcall", "dlogz_init", "nlive_init", "nlive_batch", "maxbatch", "n_effective",
                   "wt_kwargs", "stop_kwargs"}
        if set(rkw) - allowed:
            raise TypeError(f"run_dynesty: unsupported run_kwargs {sorted(set(rkw) - allowed)}")
        # ---- likelihood, prior transform and the plan: fused walks, or the host evaluates like_fn(prior_transform(u))
        setup = self._nested_setup(like_fn, prior_transform, prior_transform_comment)
        if self.verbose:
            print(f"Running nested sampling ({mode}, {'fused GPU walks' if setup[0].fused else 'host likelihood'}) with {nlive} live "
                  "points...")
        all_logz = []

        def collect(res, eq):                        # the reference keeps the largest log evidence of the runs
            all_logz.append(float(res.logz[-1]))
            self.dynesty_logz, self.dynesty_logz_err = max(all_logz), float(res.logzerr[-1])

        def checkpoint(sampler, run_number):
            if save_iter is not None:
                pkl = os.path.join(self.savedir, f"dynesty_sampler_{self.like_fn_name}_run{run_number}.pkl")
                return PickleCheckpoint(sampler, pkl, save_iter)

        self._nested_runs("dynesty", "dynesty", setup, seed,
                          lambda backend, s: NestedSampler(backend, nlive, dynamic=(mode == "dynamic"), walks=walks, batch=batch,
                                                           seed=s, **move),
                          rkw, min_ess, lambda total: f", logZ = {all_logz[-1]:.3f}", collect, dynesty_t0, samples_file,
                          custom_is_surrogate=False, checkpoint=checkpoint)

    _PYMULTINEST_DEFAULTS = {"n_live_points": 1000, "evidence_tolerance": 0.5, "sampling_efficiency": 0.8,
                             "n_iter_before_update": 100, "null_log_evidence": -1e90, "max_modes": 100, "mode_tolerance": -1e90,
                             "seed": -1, "verbose": True, "importance_nested_sampling": True, "multimodal": True,
                             "const_efficiency_mode": False, "max_iter": 0, "batch": None}

    def run_pymultinest(self, like_fn=None, prior_transform=None, sampler_kwargs={}, multi_proc=True,
                        prior_transform_comment=None, samples_file=None, prefix=None, resume=False,
                        n_clustering_params=None, outputfiles_basename=None, min_ess=int(1e4)):
        """MultiNest's algorithm on the GPU (core.py:2790-3238): static nested sampling whose replacement points are drawn
        uniformly inside ellipsoids around the live points (``alabi_amd.nested.NestedSampler(sample="unif")``; its module
        docstring states the algorithm).  Independent points without a walk length or step scale, 2-4 likelihood evaluations per
        dead point where the random walk of ``run_dynesty`` spends 25, and one ellipsoid per separated mode.

        ``like_fn`` / ``prior_transform`` and the fused / host-callback paths are those of ``run_dynesty``.  sampler_kwargs (the
        reference's defaults): ``n_live_points`` (1000), ``evidence_tolerance`` (0.5; the dlogz stop), ``sampling_efficiency``
        (0.8; every ellipsoid's volume is enlarged by 1 / efficiency), ``multimodal`` (True: up to ``min(max_modes, 32)``
        ellipsoids by recursive 2-means; False: one), ``max_modes`` (100), ``seed`` (-1: the model's seed stream), ``max_iter``
        (0: no limit), and ``batch`` (dead points per iteration, an extension; ceil(nlive / 4)).  ``n_iter_before_update``,
        ``null_log_evidence``, ``mode_tolerance``, ``verbose`` and ``importance_nested_sampling`` are accepted and have no effect:
        log Z is the plain nested-sampling estimate.  ``const_efficiency_mode=True`` and ``resume=True`` raise
        ``NotImplementedError``; any other key raises ``TypeError``.  ``multi_proc``, ``prefix``, ``n_clustering_params`` and
        ``outputfiles_basename`` have no effect (no MultiNest text files are written; ``pymultinest_analyzer`` is None).
        Use at least 50 live points per dimension: ellipsoids fitted to fewer can cut the likelihood contour and bias log Z high
        (a ``UserWarning`` says so).  Runs repeat until ``min_ess`` samples exist (at most 10) and are combined as the reference
        does: log Z averaged with sample-count weights, its error the root of the weighted mean square.  Under
        ``torch.distributed`` every rank runs its own sampler (seed + rank) and rank 0 writes the file."""
        from .nested import NestedSampler
        skw = dict(self._PYMULTINEST_DEFAULTS)
        unknown = set(sampler_kwargs) - set(skw)
        if unknown:
            raise TypeError(f"run_pymultinest: unsupported sampler_kwargs {sorted(unknown)}")
        skw.update(sampler_kwargs)
        if skw["const_efficiency_mode"]:
            raise NotImplementedError("run_pymultinest: const_efficiency_mode=True is not built")
        if resume:
            raise NotImplementedError("run_pymultinest: resume=True is not built (no MultiNest output files are written)")
        nlive = int(skw["n_live_points"])
        eff = float(skw["sampling_efficiency"])
        if not 0.0 < eff <= 1.0:
            raise ValueError("sampling_efficiency must lie in (0, 1]")
        bound = "multi" if skw["multimodal"] else "single"
        max_ell = max(1, min(int(skw["max_modes"]), 32))
        seed = None if int(skw["seed"]) < 0 else int(skw["seed"])
        maxiter = None if int(skw["max_iter"]) <= 0 else int(skw["max_iter"])
        t0 = time.time()
        setup = self._nested_setup(like_fn, prior_transform, prior_transform_comment)
        if self.verbose:
            print(f"Running ellipsoidal nested sampling ({'fused GPU draws' if setup[0].fused else 'host likelihood'}) with {nlive} "
                  "live points...")
        logz, logz_err, counts = [], [], []
        self.pymultinest_analyzer = None

        def collect(res, eq):                        # core.py:3175-3190: log Z averaged with sample-count weights
            logz.append(float(res.logz[-1])); logz_err.append(float(res.logzerr[-1])); counts.append(eq.shape[0])
            w = np.asarray(counts, dtype=np.float64) / float(np.sum(counts))
            self.pymultinest_weights = np.ones(int(np.sum(counts)))
            self.pymultinest_logz = float(np.average(logz, weights=w))
            self.pymultinest_logz_err = float(np.sqrt(np.average(np.square(logz_err), weights=w)))

        self._nested_runs("pymultinest", "PyMultiNest", setup, seed,
                          lambda backend, s: NestedSampler(backend, nlive, dynamic=False, batch=skw["batch"], seed=s, sample="unif",
                                                           bound=bound, enlarge=1.0 / eff, max_ellipsoids=max_ell),
                          {"dlogz": float(skw["evidence_tolerance"]), "maxiter": maxiter}, min_ess,
                          lambda total: f", logZ = {logz[-1]:.3f} +/- {logz_err[-1]:.3f}", collect, t0, samples_file,
                          file_fields=("weights", "logz", "logz_err"))

    # the reference's defaults (core.py:3490-3522); the keys without an entry in the docstring are accepted and have no effect
    _ULTRANEST_SAMPLER_DEFAULTS = {"derived_param_names": [], "wrapped_params": None, "num_test_samples": 2, "draw_multiple": True,
                                   "num_bootstraps": 30, "vectorized": False, "ndraw_min": 128, "ndraw_max": 65536,
                                   "storage_backend": "hdf5", "warmstart_max_tau": -1, "resume": "subfolder", "run_num": None,
                                   "seed": -1, "batch": None}
    _ULTRANEST_RUN_DEFAULTS = {"update_interval_volume_fraction": 0.8, "update_interval_ncall": None, "log_interval": None,
                               "show_status": True, "viz_callback": False, "dlogz": 0.5, "dKL": 0.5, "frac_remain": 0.01,
                               "Lepsilon": 0.001, "min_ess": 400, "max_iters": None, "max_ncalls": None,
                               "max_num_improvement_loops": 1, "min_num_live_points": 400, "cluster_num_live_points": 40,
                               "insertion_test_zscore_threshold": 4, "insertion_test_window": 10, "region_class": None,
                               "widen_before_initial_plateau_num_warn": 10000, "widen_before_initial_plateau_num_max": None}

    def run_ultranest(self, like_fn=None, prior_transform=None, sampler_kwargs={}, run_kwargs={}, multi_proc=False,
                      prior_transform_comment=None, samples_file=None, log_dir=None, resume="overwrite", min_ess=int(1e4),
                      slice_steps=0):
        """UltraNest's algorithm on the GPU (core.py:3241-3690): nested sampling whose replacement points are drawn uniformly in
        the MLFriends region -- the union of the bounding ellipsoids of ``run_pymultinest``, cut down to the points within a
        bootstrapped radius of some live point (``alabi_amd.nested.NestedSampler(sample="mlfriends")``; its module docstring states
        the algorithm).  The balls follow a curved likelihood contour that ellipsoids cannot.

        ``like_fn`` / ``prior_transform`` and the fused / host-callback paths are those of ``run_dynesty``.  sampler_kwargs:
        ``num_bootstraps`` (30), and the extensions ``seed`` (-1: the model's seed stream) and ``batch`` (dead points per iteration;
        ceil(nlive / 4)); a non-empty ``derived_param_names`` and a ``wrapped_params`` with any True raise ``NotImplementedError``;
        the reference's other keys are accepted and have no effect.  run_kwargs: ``min_num_live_points`` (400: nlive),
        ``frac_remain`` (0.01; the run stops when Z_live / Z < frac_remain, i.e. at dlogz = log1p(frac_remain)), ``max_iters``,
        ``max_ncalls``, ``max_num_improvement_loops`` (1; 0: a static run, n > 0: up to n dynamic batches, negative: 10),
        ``min_ess`` (400: the effective sample size the dynamic batches aim at); ``region_class`` other than None raises
        ``NotImplementedError``; the reference's other keys (``dlogz``, ``dKL``, ``Lepsilon``, the insertion test, ...) are accepted
        and have no effect.  An unknown key in either raises ``TypeError``.  ``slice_steps`` > 0 replaces the region draws by
        ``slice_steps`` random-direction slice updates per point (``sample="rslice"``), where the reference swaps in a slice step
        sampler.  ``log_dir`` and ``resume`` are accepted: nothing is logged and no directory is created; ``multi_proc`` is ignored.
        Use at least 50 live points per dimension, as for ``run_pymultinest``.  Runs repeat until the argument ``min_ess`` samples
        exist (at most 10) and are combined as the reference does: samples stacked, each run's weights 1 / (its sample count), log Z
        and its error those of the run with the largest log Z.  Under ``torch.distributed`` every rank runs its own sampler
        (seed + rank) and rank 0 writes the file."""
        from .nested import NestedSampler
        skw, rkw = dict(self._ULTRANEST_SAMPLER_DEFAULTS), dict(self._ULTRANEST_RUN_DEFAULTS)
        for name, given, known in (("sampler_kwargs", sampler_kwargs, skw), ("run_kwargs", run_kwargs, rkw)):
            if set(given) - set(known):
                raise TypeError(f"run_ultranest: unsupported {name} {sorted(set(given) - set(known))}")
            known.update(given)
        if skw["derived_param_names"] is not None and len(skw["derived_param_names"]) > 0:
            raise NotImplementedError("run_ultranest: derived_param_names (derived parameters) are not built")
        if skw["wrapped_params"] is not None and np.any(skw["wrapped_params"]):
            raise NotImplementedError("run_ultranest: wrapped_params (circular parameters) are not built")
        if rkw["region_class"] is not None:
            raise NotImplementedError("run_ultranest: region_class is not built; the region is MLFriends over bounding ellipsoids")
        nlive = int(rkw["min_num_live_points"])
        frac = float(rkw["frac_remain"])
        if not frac > 0.0:
            raise ValueError("frac_remain must be > 0")
        dlogz = math.log1p(frac)
        loops = int(rkw["max_num_improvement_loops"])
        dynamic, maxbatch = loops != 0, (loops if loops > 0 else 10)
        seed = None if int(skw["seed"]) < 0 else int(skw["seed"])
        if int(slice_steps) > 0:
            move = {"sample": "rslice", "slices": int(slice_steps)}
        else:
            move = {"sample": "mlfriends", "num_bootstraps": int(skw["num_bootstraps"])}
        run_args = {"dlogz": dlogz, "maxiter": rkw["max_iters"], "maxcall": rkw["max_ncalls"]}
        if dynamic:
            run_args.update(dlogz_init=dlogz, maxbatch=maxbatch, n_effective=rkw["min_ess"])
        t0 = time.time()
        setup = self._nested_setup(like_fn, prior_transform, prior_transform_comment)
        if self.verbose:
            print(f"Running MLFriends nested sampling ({'fused GPU draws' if setup[0].fused else 'host likelihood'}) with {nlive} "
                  "live points...")
        logz, logz_err, weights = [], [], []

        def collect(res, eq):                        # core.py:3629-3642: the run with the highest log evidence
            logz.append(float(res.logz[-1])); logz_err.append(float(res.logzerr[-1]))
            weights.append(np.full(eq.shape[0], 1.0 / eq.shape[0]))
            best = int(np.argmax(logz))
            self.ultranest_weights = np.concatenate(weights)
            self.ultranest_logz, self.ultranest_logz_err = logz[best], logz_err[best]

        self._nested_runs("ultranest", "UltraNest", setup, seed,
                          lambda backend, s: NestedSampler(backend, nlive, dynamic=dynamic, batch=skw["batch"], seed=s, **move),
                          run_args, min_ess, lambda total: f", logZ = {logz[-1]:.3f} +/- {logz_err[-1]:.3f}", collect, t0,
                          samples_file, file_fields=("weights", "logz", "logz_err"))
