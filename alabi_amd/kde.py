"""DeviceKDE: scipy.stats.gaussian_kde with its evaluation on the GPU (alabi_amd/csrc/kde.hip).

The reference measures a surrogate's convergence with ``gaussian_kde`` (alabi/metrics.py:210-336).  The bandwidth --
weights, effective sample size, factor, data covariance, its Cholesky factor and log-determinant -- is host math that follows
scipy's ``gaussian_kde.__init__`` / ``_compute_covariance`` step by step (``kde_bandwidth``, testable without a GPU).  The
density itself, a weighted sum of N Gaussians at each of M points, is the library's ``alabi_kde_*``: one preparation of the
whitened samples per KDE, then matrix-core exponents and a log-domain tail for every evaluation.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from scipy import linalg

from . import _lib

__all__ = ["DeviceKDE", "kde_weights", "kde_factor", "kde_bandwidth"]

_SINGULAR = ("The data appears to lie in a lower-dimensional subspace of the space in which it is expressed. This has "
             "resulted in a singular data covariance matrix, which cannot be treated using the algorithms implemented in "
             "`gaussian_kde`. Consider performing principal component analysis / dimensionality reduction and using "
             "`gaussian_kde` with the transformed data.")


def kde_weights(weights, n):
    """(weights normalised to sum 1, neff) as gaussian_kde computes them."""
    if weights is None:
        w = np.ones(n) / n
    else:
        w = np.atleast_1d(np.asarray(weights)).astype(float)
        w /= np.sum(w)
        if w.ndim != 1:
            raise ValueError("`weights` input should be one-dimensional.")
        if len(w) != n:
            raise ValueError("`weights` input should be of length n")
    return w, 1 / np.sum(w ** 2)


def kde_factor(bw_method, kde):
    """The bandwidth factor of gaussian_kde.set_bandwidth: 'scott' (default), 'silverman', a scalar, or a callable of the KDE.
    ``kde`` needs ``d`` and ``neff`` (and whatever a callable reads)."""
    if bw_method is None or (isinstance(bw_method, str) and bw_method == "scott"):
        return np.power(kde.neff, -1. / (kde.d + 4))
    if isinstance(bw_method, str) and bw_method == "silverman":
        return np.power(kde.neff * (kde.d + 2.0) / 4.0, -1. / (kde.d + 4))
    if np.isscalar(bw_method) and not isinstance(bw_method, str):
        return bw_method
    if callable(bw_method):
        return bw_method(kde)
    raise ValueError("`bw_method` should be 'scott', 'silverman', a scalar or a callable.")


def kde_bandwidth(data_covariance, factor):
    """(covariance, cho_cov, log_det) from the data covariance and the factor, as gaussian_kde._compute_covariance.
    A singular data covariance raises LinAlgError (a ValueError), as scipy's constructor does."""
    data_covariance = np.atleast_2d(data_covariance)
    try:
        data_cho = linalg.cholesky(data_covariance, lower=True)
    except linalg.LinAlgError as e:
        raise linalg.LinAlgError(_SINGULAR) from e
    covariance = data_covariance * factor ** 2
    cho_cov = (data_cho * factor).astype(np.float64)
    log_det = 2 * np.log(np.diag(cho_cov * np.sqrt(2 * np.pi))).sum()
    return covariance, cho_cov, log_det


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError("DeviceKDE needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


class DeviceKDE:
    """Gaussian KDE of ``dataset`` (d, n) -- a NumPy array, or a float64 torch tensor on the GPU, which then never leaves it.

    Same attributes as scipy.stats.gaussian_kde (``dataset``, ``d``, ``n``, ``neff``, ``weights``, ``factor``, ``covariance``,
    ``cho_cov``, ``log_det``) and the same methods (``evaluate`` = ``pdf`` = ``__call__``, ``logpdf``, ``set_bandwidth``,
    ``scotts_factor``, ``silverman_factor``, ``covariance_factor``).  Points are (d, m) arrays (a (d,) vector is one point, as in
    scipy); a torch tensor in gives a torch tensor out, on the device."""

    def __init__(self, dataset, bw_method=None, weights=None):
        self._on_device = isinstance(dataset, torch.Tensor)
        if self._on_device:
            ds = dataset if dataset.ndim >= 2 else dataset.reshape(1, -1)
            self.dataset = ds.to(device=_dev(), dtype=torch.float64)
        else:
            self.dataset = np.atleast_2d(np.asarray(dataset))
        size = self.dataset.numel() if self._on_device else self.dataset.size
        if not size > 1:
            raise ValueError("`dataset` input should have multiple elements.")
        self.d, self.n = (int(v) for v in self.dataset.shape)
        if self.d > _lib.MAX_DIM:
            raise ValueError(f"DeviceKDE supports up to {_lib.MAX_DIM} dimensions, got {self.d}")
        if isinstance(weights, torch.Tensor):
            weights = weights.detach().cpu().numpy()
        self._weighted = weights is not None
        self._weights, self._neff = kde_weights(weights, self.n)
        if self.d > self.n:
            raise ValueError("Number of dimensions is greater than number of samples. This results in a singular data "
                             "covariance matrix, which cannot be treated using the algorithms implemented in `gaussian_kde`. "
                             "Note that `gaussian_kde` interprets each *column* of `dataset` to be a point; consider "
                             "transposing the input to `dataset`.")
        self._handle = None
        h = C.c_void_p()
        _lib.check(_lib.lib().alabi_kde_create(self.d, C.byref(h)), "alabi_kde_create")
        self._handle = h
        dev = _dev()
        if self._on_device:
            self._x_dev = self.dataset.t().contiguous()
        else:
            self._x_dev = torch.as_tensor(np.ascontiguousarray(self.dataset.T, dtype=np.float64), device=dev)
        if self._weighted:
            with np.errstate(divide="ignore"):
                self._logw_dev = torch.as_tensor(np.log(self._weights), device=dev)
        else:
            self._logw_dev = None
        self.set_bandwidth(bw_method)

    # ------------------------------------------------------------------------ scipy's attributes
    @property
    def weights(self):
        return self._weights

    @property
    def neff(self):
        return self._neff

    def scotts_factor(self):
        return np.power(self.neff, -1. / (self.d + 4))

    def silverman_factor(self):
        return np.power(self.neff * (self.d + 2.0) / 4.0, -1. / (self.d + 4))

    def covariance_factor(self):
        return kde_factor(self._bw_method, self)

    def _data_cov(self):
        if self._on_device:
            aw = torch.as_tensor(self._weights, device=self.dataset.device) if self._weighted else None
            return np.atleast_2d(torch.cov(self.dataset, correction=1, aweights=aw).cpu().numpy())
        return np.atleast_2d(np.cov(self.dataset, rowvar=1, bias=False, aweights=self._weights))

    def set_bandwidth(self, bw_method=None):
        """gaussian_kde.set_bandwidth: recompute the factor, the covariance and the device copy of the whitened samples."""
        self._bw_method = bw_method
        self.factor = self.covariance_factor()
        if not hasattr(self, "_data_covariance"):
            self._data_covariance = self._data_cov()
        self.covariance, self.cho_cov, self.log_det = kde_bandwidth(self._data_covariance, self.factor)
        L = np.ascontiguousarray(self.cho_cov, dtype=np.float64)
        st = _lib.lib().alabi_kde_set_data(self._handle, _lib.ptr(self._x_dev), _lib.ptr(self._logw_dev), self.n,
                                           L.ctypes.data_as(C.POINTER(C.c_double)), _lib.current_stream())
        _lib.check(st, "alabi_kde_set_data")

    # ------------------------------------------------------------------------ evaluation
    def _points(self, points):
        """(device tensor [m, d] contiguous, torch_in)."""
        torch_in = isinstance(points, torch.Tensor)
        if torch_in:
            p = points.to(device=_dev(), dtype=torch.float64)
            p = p.reshape(1, -1) if p.ndim < 2 else p
        else:
            p = np.atleast_2d(np.asarray(points, dtype=np.float64))
        d, m = p.shape
        if d != self.d:
            if d == 1 and m == self.d:                   # a row vector: one point
                p = p.reshape(self.d, 1)
            else:
                raise ValueError(f"points have dimension {d}, dataset has dimension {self.d}")
        if torch_in:
            return p.t().contiguous(), True
        return torch.as_tensor(np.ascontiguousarray(p.T), device=_dev()), False

    def _run(self, points, fn):
        q, torch_in = self._points(points)
        m = q.shape[0]
        out = torch.empty(m, dtype=torch.float64, device=q.device)
        _lib.check(getattr(_lib.lib(), fn)(self._handle, _lib.ptr(q), m, _lib.ptr(out), _lib.current_stream()), fn)
        return out if torch_in else out.cpu().numpy()

    def evaluate(self, points):
        """The density at points (d, m) -> (m,)."""
        return self._run(points, "alabi_kde_pdf")

    __call__ = evaluate

    def pdf(self, x):
        return self.evaluate(x)

    def logpdf(self, x):
        """The log-density at points (d, m) -> (m,); finite where the density underflows (scipy's log-sum-exp)."""
        return self._run(x, "alabi_kde_logpdf")

    def plan(self, m):
        """(parts, samples per part) of the sample-axis split an evaluation of m points uses."""
        parts, pts = C.c_int(), C.c_int()
        _lib.check(_lib.lib().alabi_kde_plan(self._handle, int(m), C.byref(parts), C.byref(pts)), "alabi_kde_plan")
        return parts.value, pts.value

    # ------------------------------------------------------------------------ lifetime
    def _release(self):
        _lib.destroy(getattr(self, "_handle", None), "alabi_kde_destroy", sync=True)
        self._handle = None

    def __del__(self):
        self._release()
