"""Chain diagnostics of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021), "Rank-normalization, folding, and localization:
an improved R-hat for assessing convergence of MCMC": rank-normalised split R-hat, bulk and tail effective sample size, the
effective sample size and the Monte-Carlo standard error of the mean -- what a user of Stan, PyMC or ArviZ reads first.

``summary(chain)`` takes a chain [n_t, n_w, n_d] (1-D and 2-D are promoted as ``integrated_time`` does) and returns a dict of
[n_d] NumPy arrays: mean, sd, mcse_mean, ess_mean, ess_bulk, ess_tail, rhat.  Every walker is split into its first and its last
n_t // 2 steps (m = 2 n_w chains); per parameter

  rhat       max(R-hat(z(x)), R-hat(z(|x - median|)))     z: normal scores of the average ranks of the pooled draws
  ess_bulk   ESS(z(x))        ess_tail  min(ESS(1[x <= q_0.05]), ESS(1[x <= q_0.95]))        ess_mean  ESS(x)
  mcse_mean  sd(pooled, ddof 1) / sqrt(ess_mean)

with R-hat = sqrt(var+ / W), rho_l = 1 - (W - mean_c gamma_c(l)) / var+ and Geyer's initial monotone sequence (``_geyer``).

A chain that lives on the GPU stays there: per parameter the pooled draws are sorted (torch.sort), average ranks come from the run
lengths of the sorted values, and the library's ``alabi_chain_split_stats`` (alabi_amd/csrc/chain_acf.hip: the four-step
transforms in LDS of ``alabi_chain_autocorr``) returns per-chain moments and the chain-averaged autocovariance of five passes:
z-scores, folded z-scores (moments only), the raw values and the two tail indicators -- the last three read the caller's
(possibly strided: discard / thin) view in place for all parameters at once, the transform applied on load.  Only
[m, n_d] moments and [n_d, n] autocovariances come to the host, where the truncation runs.  Host arrays take a NumPy path.

Walkers are independent chains under the ``metropolis``, ``hmc`` and ``nuts`` moves.  Under the red-blue ensemble moves (stretch,
DE, snooker, walk, KDE) the walkers of one ensemble are coupled: R-hat still detects chains that disagree, but the ESS formula
assumes independent chains and is approximate there.

Not provided: the ``rank``-only and ``identity`` R-hat variants, ESS of quantiles or of the sd, and the MCSE of quantiles.
"""
from __future__ import annotations

import numpy as np
import torch

__all__ = ["rhat", "ess", "mcse_mean", "summary"]

KEYS = ("mean", "sd", "mcse_mean", "ess_mean", "ess_bulk", "ess_tail", "rhat")


def _promote(chain):
    if not isinstance(chain, torch.Tensor):
        chain = np.atleast_1d(np.asarray(chain, dtype=np.float64))
    if chain.ndim == 1:
        chain = chain[:, None, None]
    if chain.ndim == 2:
        chain = chain[:, :, None]
    if chain.ndim != 3:
        raise ValueError("chain must be [n_t], [n_t, n_w] or [n_t, n_w, n_d]")
    return chain


# ------------------------------------------------------------------------------------------------ host half (both paths)
def _geyer(rho, m, n):
    """ESS = m n / tau from rho[0 .. n): pair sums P_k = rho_2k + rho_2k+1, cut at the first that is not > 0 (or not finite),
    made monotone, tau = -1 + 2 sum_{k < K} P_k + max(rho_2K, 0), at least 1 / log10(m n)."""
    npairs = n // 2
    P = rho[0:2 * npairs:2] + rho[1:2 * npairs:2]
    bad = ~(np.isfinite(P) & (P > 0.0))
    K = int(np.argmax(bad)) if bad.any() else npairs
    tau = -1.0 + 2.0 * float(np.sum(np.minimum.accumulate(P[:K]))) if K else -1.0
    if 2 * K < n:
        tau += max(float(rho[2 * K]), 0.0)
    tau = max(tau, 1.0 / np.log10(m * n))
    return m * n / tau


def _between_within(mean_c, var_c, n):
    W = float(np.mean(var_c))
    Bn = float(np.var(mean_c, ddof=1)) if mean_c.size > 1 else 0.0
    return W, (n - 1.0) / n * W + Bn


def _rhat_from(mean_c, var_c, n):
    W, varp = _between_within(mean_c, var_c, n)
    with np.errstate(all="ignore"):
        return float(np.sqrt(varp / W))


def _ess_from(mean_c, var_c, acov):
    """mean_c, var_c [m] (ddof 1), acov [n]: the mean over the chains of the biased autocovariance."""
    m, n = mean_c.size, acov.size
    W, varp = _between_within(mean_c, var_c, n)
    with np.errstate(all="ignore"):
        rho = 1.0 - (W - acov) / varp
    rho[0] = 1.0
    return _geyer(rho, m, n)


def _pooled(mean_c, var_c, n):
    """Mean and sd (ddof 1) of the pooled draws of m chains of equal length n from the chains' own moments."""
    m = mean_c.size
    mu = float(np.mean(mean_c))
    ss = (n - 1.0) * float(np.sum(var_c)) + n * float(np.sum((mean_c - mu) ** 2))
    return mu, float(np.sqrt(ss / (m * n - 1.0)))


def _assemble(out, k, m, n, z, folded, raw, ind05, ind95):
    """Fill parameter k from the five passes: (mean_c, var_c, acov) each, acov None for the folded pass."""
    out["mean"][k], out["sd"][k] = _pooled(raw[0], raw[1], n)
    out["rhat"][k] = max(_rhat_from(z[0], z[1], n), _rhat_from(folded[0], folded[1], n))
    out["ess_bulk"][k] = _ess_from(*z)
    out["ess_mean"][k] = _ess_from(*raw)
    out["ess_tail"][k] = min(_ess_from(*ind05), _ess_from(*ind95))
    out["mcse_mean"][k] = out["sd"][k] / np.sqrt(out["ess_mean"][k])


def _constant(out, k, value, m, n):
    out["mean"][k], out["sd"][k], out["mcse_mean"][k] = value, 0.0, 0.0
    out["ess_mean"][k] = out["ess_bulk"][k] = out["ess_tail"][k] = m * n


# ------------------------------------------------------------------------------------------------ NumPy path
def _split_host(x):
    n_t = x.shape[0]
    n = n_t // 2
    return np.concatenate([x[:n].T, x[n_t - n:].T], axis=0)                     # [2 n_w, n], chain c = half * n_w + w


def _stats_host(y, acov=True):
    m, n = y.shape
    mean_c, var_c = y.mean(axis=1), y.var(axis=1, ddof=1)
    if not acov:
        return mean_c, var_c, None
    size = 1
    while size < n:
        size *= 2
    f = np.fft.rfft(y - mean_c[:, None], n=2 * size, axis=1)
    g = np.fft.irfft(f * np.conjugate(f), n=2 * size, axis=1)[:, :n] / n
    return mean_c, var_c, g.mean(axis=0)


def _rank_z_host(y):
    v = y.ravel()
    order = np.argsort(v, kind="stable")
    s = v[order]
    start = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    count = np.diff(np.concatenate([start, [s.size]]))
    r = np.empty(v.size)
    r[order] = np.repeat(start + (count + 1) / 2.0, count)
    from scipy.special import ndtri
    return ndtri((r - 0.375) / (v.size + 0.25)).reshape(y.shape)


def _summary_host(x):
    n_t, n_w, n_d = x.shape
    out = {key: np.full(n_d, np.nan) for key in KEYS}
    if n_t < 4:
        return out
    for k in range(n_d):
        if not np.all(np.isfinite(x[:, :, k])):
            continue
        y = _split_host(x[:, :, k])
        m, n = y.shape
        if np.all(y == y.flat[0]):
            _constant(out, k, float(y.flat[0]), m, n)
            continue
        ind = [(y <= np.quantile(y, p)).astype(np.float64) for p in (0.05, 0.95)]
        _assemble(out, k, m, n, _stats_host(_rank_z_host(y)), _stats_host(_rank_z_host(np.abs(y - np.median(y))), acov=False),
                  _stats_host(y), _stats_host(ind[0]), _stats_host(ind[1]))
    return out


# ------------------------------------------------------------------------------------------------ device path
def _split_stats(x, n_split, transform=0, par=None, acov=True):
    """alabi_chain_split_stats on a device chain x[n_t, n_w, n_d] whose walkers and parameters are contiguous (any step stride):
    (chain_mean [m, n_d], chain_var [m, n_d], acov_mean [n_d, n] or None) as device tensors."""
    from . import _lib
    n_t, n_w, n_d = x.shape
    m, n = n_split * n_w, n_t // n_split
    mean_c = torch.empty((m, n_d), dtype=torch.float64, device=x.device)
    var_c = torch.empty_like(mean_c)
    g = torch.empty((n_d, n), dtype=torch.float64, device=x.device) if acov else None
    _lib.check(_lib.lib().alabi_chain_split_stats(_lib.ptr(x), n_t, x.stride(0), n_w, n_d, n_split, transform, _lib.ptr(par),
                                                  _lib.ptr(mean_c), _lib.ptr(var_c), _lib.ptr(g), _lib.current_stream()),
               "alabi_chain_split_stats")
    return mean_c, var_c, g


def _strided_view(x):
    """x itself if element (t, w, k) lies at t * stride + w * n_d + k with stride >= n_w n_d (what a discard / thin view of the
    sampler's chain is); a contiguous copy otherwise."""
    n_t, n_w, n_d = x.shape
    if x.stride(2) == 1 and x.stride(1) == n_d and x.stride(0) >= n_w * n_d:
        return x
    return x.contiguous()


def _rank_z_device(v):
    """Normal scores of the average ranks of a flat device tensor, in the order of v; also the sorted values."""
    s, order = torch.sort(v)
    _, inverse, count = torch.unique_consecutive(s, return_inverse=True, return_counts=True)
    last = torch.cumsum(count, 0).to(torch.float64)                              # rank of the last member of every run
    r = (last - (count.to(torch.float64) - 1.0) / 2.0)[inverse]
    z = torch.empty_like(v)
    # a device divisor: torch turns a division by a host scalar into a multiplication by its reciprocal, one rounding more, and
    # in the tails an ulp of the probability is 1 / pdf(z) ulps of z
    size = torch.tensor(v.numel() + 0.25, dtype=torch.float64, device=v.device)
    z[order] = torch.special.ndtri((r - 0.375) / size)
    return z, s


def _quantile_sorted(s, p):
    """NumPy's default (linear) quantile of an ascending device tensor: a 0-dim device tensor."""
    pos = (s.numel() - 1) * p
    lo = int(np.floor(pos))
    t = pos - lo
    a, b = s[lo], s[min(lo + 1, s.numel() - 1)]
    return b - (b - a) * (1.0 - t) if t >= 0.5 else a + (b - a) * t


def _median_sorted(s):
    S = s.numel()
    return (s[(S - 1) // 2] + s[S // 2]) / 2.0


def _summary_device(x, timings=None):
    import time
    n_t, n_w, n_d = x.shape
    out = {key: np.full(n_d, np.nan) for key in KEYS}
    if n_t < 4:
        return out
    x = _strided_view(x.to(torch.float64))
    h = n_t // 2
    m, n = 2 * n_w, h
    finite = np.zeros(n_d, dtype=bool)

    def clock(name, t0):
        if timings is not None:
            torch.cuda.synchronize()
            timings[name] = timings.get(name, 0.0) + time.perf_counter() - t0

    q05 = torch.zeros(n_d, dtype=torch.float64, device=x.device)
    q95 = torch.zeros_like(q05)
    constant = np.zeros(n_d, dtype=bool)
    z_pass, f_pass = [None] * n_d, [None] * n_d
    for k in range(n_d):
        t0 = time.perf_counter()
        finite[k] = bool(torch.isfinite(x[:, :, k]).all().item())
        if not finite[k]:
            continue
        pooled = torch.cat([x[:h, :, k], x[n_t - h:, :, k]], dim=0)              # [2 h, n_w]: one parameter's surviving draws
        z, s = _rank_z_device(pooled.reshape(-1))
        constant[k] = bool((s[0] == s[-1]).item())
        if constant[k]:
            clock("sort_rank", t0)
            continue
        q05[k], q95[k] = _quantile_sorted(s, 0.05), _quantile_sorted(s, 0.95)
        zf, _ = _rank_z_device((pooled - _median_sorted(s)).abs_().reshape(-1))
        clock("sort_rank", t0)
        t0 = time.perf_counter()
        z_pass[k] = _split_stats(z.reshape(2 * h, n_w, 1), 2)
        f_pass[k] = _split_stats(zf.reshape(2 * h, n_w, 1), 2, acov=False)
        clock("split_stats", t0)
    t0 = time.perf_counter()
    raw = _split_stats(x, 2)                                                     # in place, every parameter at once
    ind05 = _split_stats(x, 2, transform=1, par=q05)
    ind95 = _split_stats(x, 2, transform=1, par=q95)
    clock("split_stats", t0)
    raw, ind05, ind95 = ([a.cpu().numpy() for a in p] for p in (raw, ind05, ind95))

    def column(p, k):
        return p[0][:, k], p[1][:, k], p[2][k]

    for k in range(n_d):
        if not finite[k]:
            continue
        if constant[k]:
            _constant(out, k, float(raw[0][0, k]), m, n)
            continue
        zk = [a.cpu().numpy() for a in z_pass[k]]
        fk = [a.cpu().numpy() for a in f_pass[k][:2]]
        _assemble(out, k, m, n, (zk[0][:, 0], zk[1][:, 0], zk[2][0]), (fk[0][:, 0], fk[1][:, 0], None),
                  column(raw, k), column(ind05, k), column(ind95, k))
    return out


# ------------------------------------------------------------------------------------------------ public
def summary(chain, timings=None):
    """dict of [n_d] arrays -- mean, sd, mcse_mean, ess_mean, ess_bulk, ess_tail, rhat -- of a chain [n_t, n_w, n_d].

    n_t < 4: NaN everywhere.  A NaN or inf anywhere in a parameter: NaN for that parameter only.  A parameter whose draws are all
    equal: rhat NaN, every ESS = m n, mcse_mean 0.  Walkers count as independent chains (module docstring: under the red-blue
    ensemble moves the ESS figures are approximate).  ``timings``: a dict that receives the seconds spent in the device path's
    sort / rank part and in alabi_chain_split_stats (synchronising; for measurement only)."""
    x = _promote(chain)
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            return _summary_device(x, timings)
        x = x.detach().numpy().astype(np.float64, copy=False)
    return _summary_host(x)


def rhat(chain):
    """Rank-normalised split R-hat, the larger of the bulk and the folded value, per parameter."""
    return summary(chain)["rhat"]


def ess(chain, method="bulk"):
    """Effective sample size per parameter: "bulk" (rank-normalised), "tail" (5 % / 95 % indicators) or "mean"."""
    if method not in ("bulk", "tail", "mean"):
        raise ValueError("method must be 'bulk', 'tail' or 'mean'")
    return summary(chain)["ess_" + method]


def mcse_mean(chain):
    """Monte-Carlo standard error of the posterior mean per parameter."""
    return summary(chain)["mcse_mean"]
