"""Host side of the HMC warm-up (``EnsembleSampler.tune_hmc``): Stan's window schedule, the pooled step size and the shrunk
covariance estimate that becomes the mass matrix.  Pure NumPy / torch: no library call, no GPU needed to import or to call with
NumPy arrays.  The step size itself is adapted on the device, per walker, by ``ens_hmc_adapt_kernel`` (dual averaging, Hoffman &
Gelman 2014, algorithm 5); what is here runs between its calls.  tests/hmc_adapt_numpy.py is the CPU statement of the whole.
"""
from __future__ import annotations

import numpy as np

__all__ = ["warmup_windows", "warmup_segments", "pooled_step_size", "regularised_covariance", "initial_state", "restart_state",
           "searched_state", "DA_DEFAULTS", "DA_WORDS"]

DA_WORDS = 5                                  # m, H-bar, ln e, ln e-bar, mu per walker
DA_DEFAULTS = (0.8, 0.05, 10.0, 0.75)         # delta, gamma, t0, kappa (Stan's)
INIT_BUFFER, TERM_BUFFER, BASE_WINDOW = 75, 50, 25


def _schedule(nwarmup):
    """(initial buffer, end indices of the slow windows) of Stan's warm-up of ``nwarmup`` steps."""
    n = int(nwarmup)
    if n < 0:
        raise ValueError("nwarmup must not be negative")
    if n < 20:
        return n, []
    init, term, size = INIT_BUFFER, TERM_BUFFER, BASE_WINDOW
    if init + size + term > n:
        init, term = int(0.15 * n), int(0.1 * n)
        size = n - init - term
    term_start = n - term
    ends, start = [], init
    while start < term_start:
        end = start + size
        if end + 2 * size > term_start:       # the window after this one would not fit: this one takes the rest
            end = term_start
        ends.append(end)
        start, size = end, 2 * size
    return init, ends


def warmup_windows(nwarmup):
    """End indices of the slow (mass-matrix) windows of Stan's warm-up schedule: an initial buffer of 75 steps, a terminal buffer
    of 50, a first window of 25 and every next one twice as long, a window stretched to the start of the terminal buffer when the
    one after it would not fit.  Where 75 + 25 + 50 exceed ``nwarmup``: 15 % and 10 % of it as buffers and one window with the rest;
    below 20 steps no window (the step size alone is adapted).  1000 -> [100, 150, 250, 450, 950]."""
    return _schedule(nwarmup)[1]


def warmup_segments(nwarmup, windows=True):
    """[(first step, end, is_window)] covering 0 ... nwarmup: the initial buffer, the slow windows, the terminal buffer (empty
    ones left out).  ``windows=False``: one segment, the step size alone."""
    n = int(nwarmup)
    init, ends = _schedule(n)
    if not windows or not ends:
        return [(0, n, False)] if n > 0 else []
    segs = [(0, init, False)] if init > 0 else []
    start = init
    for end in ends:
        segs.append((start, end, True))
        start = end
    if start < n:
        segs.append((start, n, False))
    return segs


def pooled_step_size(log_eps_bar):
    """exp(mean ln e-bar) over all walkers of all ensembles: the move table carries one step size."""
    v = np.asarray(log_eps_bar.detach().cpu().numpy() if hasattr(log_eps_bar, "detach") else log_eps_bar, dtype=np.float64)
    return float(np.exp(np.mean(v)))


def regularised_covariance(samples, metric="diag"):
    """The sample covariance of ``samples`` [n, d] (a window's stored positions, pooled over steps and walkers, in the sampler's
    frame; a NumPy array or a torch tensor on any device), shrunk as Stan does: n / (n + 5) S + 1e-3 * 5 / (n + 5) I.  ``metric``
    "diag" returns the d variances, "dense" the matrix (NumPy, float64)."""
    if metric not in ("diag", "dense"):
        raise ValueError("metric must be 'diag' or 'dense'")
    if hasattr(samples, "detach"):
        import torch
        x = samples.detach().reshape(-1, samples.shape[-1]).to(torch.float64)
        n, d = int(x.shape[0]), int(x.shape[1])
        if n < 2:
            raise ValueError("a covariance needs at least two samples")
        S = (torch.var(x, dim=0, unbiased=True) if metric == "diag" else torch.cov(x.T).reshape(d, d)).cpu().numpy()
    else:
        x = np.asarray(samples, dtype=np.float64)
        x = x.reshape(-1, x.shape[-1])
        n, d = x.shape
        if n < 2:
            raise ValueError("a covariance needs at least two samples")
        S = np.var(x, axis=0, ddof=1) if metric == "diag" else np.cov(x.T).reshape(d, d)
    a, b = n / (n + 5.0), 1e-3 * 5.0 / (n + 5.0)
    if metric == "diag":
        return a * S + b
    S = a * S + b * np.eye(d)
    return 0.5 * (S + S.T)


def initial_state(n_walkers, step_size):
    """The dual-averaging state [n_walkers, 5] at the start of warm-up: m = 0, H-bar = 0, ln e = ln step_size, ln e-bar = 0,
    mu = ln(10 step_size)."""
    st = np.zeros((int(n_walkers), DA_WORDS))
    st[:, 2] = np.log(float(step_size))
    st[:, 4] = np.log(10.0 * float(step_size))
    return st


def restart_state(n_walkers, pooled):
    """The state every walker restarts from at a window's end: m = 0, H-bar = 0, ln e = ln e-bar = ln pooled, mu = ln 10 + ln pooled."""
    st = np.zeros((int(n_walkers), DA_WORDS))
    st[:, 2] = st[:, 3] = np.log(float(pooled))
    st[:, 4] = np.log(10.0) + np.log(float(pooled))
    return st


def searched_state(ln_e):
    """The state each walker starts from after the step-size search (``EnsembleSampler.find_step_size``), ``ln_e`` [n_walkers] its
    own searched value: m = 0, H-bar = 0, ln e = ln e-bar = ln e_w, mu = ln 10 + ln e_w."""
    v = np.asarray(ln_e.detach().cpu().numpy() if hasattr(ln_e, "detach") else ln_e, dtype=np.float64).reshape(-1)
    st = np.zeros((len(v), DA_WORDS))
    st[:, 2] = st[:, 3] = v
    st[:, 4] = np.log(10.0) + v
    return st
