"""Chain diagnostics of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021) in plain NumPy / SciPy: rank-normalised split
R-hat, bulk and tail effective sample size, the effective sample size and the Monte-Carlo standard error of the mean.  The model
that alabi_amd/diagnostics.py (host and device paths) and alabi_chain_split_stats are held to; nothing is imported from alabi_amd.

A chain is x[t, w, k] (n_t steps, n_w walkers, n_d parameters); everything is done per parameter.

  split         h = n_t // 2; every walker yields the chains [0, h) and [n_t - h, n_t) (odd n_t: the middle step is dropped);
                chain c = half * n_w + w, m = 2 n_w chains of length n = h.
  plain R-hat   W = mean_c s2_c (ddof 1), B/n = var_c(mean_c) (ddof 1; 0 for m = 1), var+ = (n - 1)/n W + B/n, sqrt(var+ / W).
  ESS           gamma_c(l) = (1/n) sum_{t < n - l} (y[t] - mean_c)(y[t + l] - mean_c) (biased), rho_0 = 1,
                rho_l = 1 - (W - mean_c gamma_c(l)) / var+; Geyer's initial monotone sequence over P_k = rho_2k + rho_2k+1 (geyer()).
  rank z        average ranks r of the pooled S = m n draws, z = Phi^-1((r - 3/8) / (S + 1/4)).
  rhat          max(R-hat(z(x)), R-hat(z(|x - median|)));  ess_bulk = ESS(z(x));  ess_tail = min over p in (0.05, 0.95) of
                ESS(1[x <= q_p]);  ess_mean = ESS(x);  mcse_mean = sd(pooled, ddof 1) / sqrt(ess_mean).

Two autocovariance routes: ``acov_fft`` (zero-padded real FFT) and ``acov_direct`` (the sums as written, in np.longdouble, for
n <= 1100)."""
from __future__ import annotations

import numpy as np
from scipy.special import ndtri

LD = np.longdouble
KEYS = ("mean", "sd", "mcse_mean", "ess_mean", "ess_bulk", "ess_tail", "rhat")
PASSES = ("z", "folded", "raw", "ind05", "ind95")


def promote(chain):
    x = np.asarray(chain, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None, None]
    if x.ndim == 2:
        x = x[:, :, None]
    return x


def split(x, n_split=2):
    """x[n_t, n_w] -> y[n_split * n_w, n_t // n_split] (chain c = half * n_w + w)."""
    n_t = x.shape[0]
    n = n_t // n_split
    if n_split == 1:
        return np.ascontiguousarray(x.T)
    return np.concatenate([x[:n].T, x[n_t - n:].T], axis=0)


def acov_fft(y):
    """gamma[c, l] of y[c, t] through a zero-padded FFT."""
    m, n = y.shape
    size = 1
    while size < n:
        size *= 2
    yc = y - y.mean(axis=1, keepdims=True)
    f = np.fft.rfft(yc, n=2 * size, axis=1)
    return np.fft.irfft(f * np.conjugate(f), n=2 * size, axis=1)[:, :n] / n


def acov_direct(y):
    """The same sums as they are written, in extended precision (rounded to fp64 at the end)."""
    m, n = y.shape
    assert n <= 1100
    yl = y.astype(LD)
    yc = yl - yl.sum(axis=1, keepdims=True) / LD(n)
    out = np.empty((m, n), dtype=LD)
    for lag in range(n):
        out[:, lag] = (yc[:, :n - lag] * yc[:, lag:]).sum(axis=1) / LD(n)
    return out.astype(np.float64)


def moments(y):
    return y.mean(axis=1), y.var(axis=1, ddof=1)


def plain_rhat(y):
    m, n = y.shape
    mu, s2 = moments(y)
    W = s2.mean()
    Bn = mu.var(ddof=1) if m > 1 else 0.0
    with np.errstate(all="ignore"):
        return float(np.sqrt(((n - 1.0) / n * W + Bn) / W))


def geyer(rho, m, n):
    """(ESS, the pair sums that were examined: P_0 .. P_K, up to and including the first one that is not > 0)."""
    npairs = n // 2                                        # k with 2 k + 1 <= n - 1
    P = [rho[2 * k] + rho[2 * k + 1] for k in range(npairs)]
    K = npairs
    for k in range(npairs):
        if not (np.isfinite(P[k]) and P[k] > 0.0):
            K = k
            break
    examined = np.array(P[:min(K + 1, npairs)])
    for k in range(1, K):
        P[k] = min(P[k], P[k - 1])
    tau = -1.0 + 2.0 * sum(P[:K])
    if 2 * K < n:
        tau += max(rho[2 * K], 0.0)
    tau = max(tau, 1.0 / np.log10(m * n))
    return m * n / tau, examined


def ess(y, acov=acov_fft, detail=False):
    m, n = y.shape
    mu, s2 = moments(y)
    W = s2.mean()
    Bn = mu.var(ddof=1) if m > 1 else 0.0
    varp = (n - 1.0) / n * W + Bn
    g = acov(y).mean(axis=0)
    with np.errstate(all="ignore"):
        rho = 1.0 - (W - g) / varp
    rho[0] = 1.0
    e, examined = geyer(rho, m, n)
    return (e, examined) if detail else e


def average_ranks(v):
    """Ranks 1 .. S of a flat array, ties sharing the mean of their ranks."""
    order = np.argsort(v, kind="stable")
    s = v[order]
    start = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    count = np.diff(np.concatenate([start, [s.size]]))
    r_sorted = np.repeat(start + (count + 1) / 2.0, count)
    r = np.empty(v.size)
    r[order] = r_sorted
    return r


def rank_z(y):
    r = average_ranks(y.ravel())
    return ndtri((r - 0.375) / (y.size + 0.25)).reshape(y.shape)


def summary(chain, acov=acov_fft, detail=False):
    """dict of [n_d] arrays (KEYS); with detail also "pairs": {pass: [per parameter the examined pair sums]} and "rhat_parts"."""
    x = promote(chain)
    n_t, n_w, n_d = x.shape
    out = {k: np.full(n_d, np.nan) for k in KEYS}
    pairs = {p: [np.zeros(0)] * n_d for p in PASSES}
    parts = np.full((n_d, 2), np.nan)
    for k in range(n_d):
        if n_t < 4 or not np.all(np.isfinite(x[:, :, k])):
            continue
        y = split(x[:, :, k])
        m, n = y.shape
        out["mean"][k] = y.mean()
        out["sd"][k] = y.std(ddof=1)
        if np.all(y == y.flat[0]):
            for key in ("ess_mean", "ess_bulk", "ess_tail"):
                out[key][k] = m * n
            out["mcse_mean"][k] = 0.0
            continue
        z = rank_z(y)
        zf = rank_z(np.abs(y - np.median(y)))
        parts[k] = plain_rhat(z), plain_rhat(zf)
        out["rhat"][k] = max(parts[k])
        out["ess_bulk"][k], pairs["z"][k] = ess(z, acov, True)
        pairs["folded"][k] = np.zeros(0)                   # moments only: no truncation in that pass
        out["ess_mean"][k], pairs["raw"][k] = ess(y, acov, True)
        tails = []
        for name, p in (("ind05", 0.05), ("ind95", 0.95)):
            e, pairs[name][k] = ess((y <= np.quantile(y, p)).astype(np.float64), acov, True)
            tails.append(e)
        out["ess_tail"][k] = min(tails)
        out["mcse_mean"][k] = out["sd"][k] / np.sqrt(out["ess_mean"][k])
    if detail:
        out["pairs"] = pairs
        out["rhat_parts"] = parts
    return out


def margin(detail_summary):
    """The smallest |P_k| over every examined pair sum of every pass and parameter (inf when nothing was examined)."""
    best = np.inf
    for per_param in detail_summary["pairs"].values():
        for e in per_param:
            if e.size:
                best = min(best, float(np.min(np.abs(e))))
    return best
