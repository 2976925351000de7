"""Extended-precision truth for the Gaussian KDE (alabi_amd/csrc/kde.hip) and the counted-rounding bound its logpdf and pdf are
held to (tests/test_kde_reference_host.py, tests/test_gpu_kde_truth.py).  Plain NumPy (mpmath where ``np.longdouble`` is only a
double, as tests/kernel_sum_reference.py); no GPU, nothing imported from alabi_amd.

Inputs are the library's own fp64 numbers, taken as exact: the samples X [N, d], the Cholesky factor L = cho_cov [d, d] (bit-equal
to scipy's), the fp64 ``log w`` array the class hands to alabi_kde_set_data (``fl(-log N)`` for every sample when unweighted; -inf
or NaN = weight zero) and the queries Q [M, d].

Truth.   logpdf_m = logsumexp_n(log w_n - |L^-1 (q_m - x_n)|^2 / 2) - sum_k log(L_kk sqrt(2 pi)),   pdf_m = exp(logpdf_m).
  ``truth(..., direct=True)`` runs the forward substitution on every difference q_m - x_n itself (N M d^2 / 2 extended operations:
  the small cases, and the cross-check of the fast route).  The default route uses the linearity of the substitution about an
  anchor a = X[0] -- a data point, NOT the mean: y_mn = L^-1 (q_m - a) - L^-1 (x_n - a), N M d operations.  The differences from the
  anchor are formed in extended precision (exact or 2^-64 relative, whatever common offset the data carries), so this route owes
  nothing to the centring either; its own rounding is 2^-64 relative to |L^-1 (q - a)| and |L^-1 (x - a)| per component, i.e.
  2^-11 of what ONE of the d + 4 fp64 roundings counted below costs.  The host test holds the two routes and a 50-digit mpmath
  evaluation (at which the linearity costs nothing) together.  pdf is exactly 0 only where the extended result is below 2^-1074.

Bound (``tolerance_logpdf``, ``tolerance_pdf``), u = 2^-53, per query m.  c is the plain fp64 mean of the samples,
z_n = L^-1 (x_n - c), u_m = L^-1 (q_m - c) (fp64 is ample for a magnitude), p_mn the truth's softmax weights of the N terms.

  exponent of term (m, n), absolute error e_mn = u [ C A_mn + (d + 2) H_mn ] + W_mn:
    C A_mn   the augmented product (q' . s') ln2/256 carries C roundings of at most u A_mn each,
             A_mn = sum_k |u_k z_k| + |u|^2/2 + |z|^2/2 + |log w_n|:
             d + 3, the figure kernel_sum_reference.py uses for this form (the d + 2 accumulations of the matrix core and the
             scaling of the query row by 256/ln2), plus 1 for logpdf: the tail pass subtracts the shift from slot d + 1 of the query
             row, one rounding of a number no larger than A_mn 256/ln2 (the shift is the negative of min_n(r^2/2 - log w) <= A_mn).
             C = d + 4 for logpdf, d + 3 for pdf.
    (d+2) H  H_mn = |u|^2/2 + |z|^2/2 + |log w_n|: the two half norms are d fmas each (u |z|^2 / 2 per fma at most), then
             fma(-0.5, zz, log w) and -0.5 uu 256/ln2 round once more each.
    W_mn     the whitening.  Forward substitution with at most d roundings per component (k fmas and a division in row k) has the
             componentwise backward error d u |L|; the right-hand sides x - c and q - c round once per coordinate.  So
               dz_n = |L^-1| (d u |L| |z_n| + u |x_n - c|),   du_m = |L^-1| (d u |L| |u_m| + u |q_m - c|)
             and, because -|u|^2/2 and -|z|^2/2 are formed from the same rounded vectors, the exponent the device forms is
             -|u^ - z^|^2 / 2 and differs from the truth's by  W_mn = sum_k |u_k - z_k| (du_k + dz_k) + (|du| + |dz|)^2 / 2.
             The centre itself: the device's mean of N samples differs from c by at most dc = u ((N - 1) mean_n |x_n| + |c|) per
             coordinate (N - 1 additions in any order and the division).  Samples and queries are centred on the SAME number, so
             this moves no difference u - z; it moves the magnitudes, and |u|, |z| in A, H and dz, du are enlarged by |L^-1| dc.
  term   relative error expm1(e_mn + E u), E = 10: exp2s_tab256 at its documented 2.2 ulp (gp_device.hpp), twice that rounded up,
         plus 4, the figure kernel_sum_reference.py uses for this exponential.
  sum    N - 1 additions of positive terms in any order (parts, DPP folds, the combine): relative (N - 1) u.
         rho_m = sum_n p_mn expm1(e_mn + E u) + (N - 1) u  is the relative error of the sum, -log1p(-rho_m) that of its logarithm.
  logpdf   tol = -log1p(-rho) + T + G
         T  roundings after the sum.  First pass (largest exponent mx >= -650): log at 1 ulp, 2 u |log s|, s = the sum, and the add
            of log_norm, u |logpdf|.  Tail pass (mx < -650): 2 u |log s'| of the shifted sum (1 <= s' <= N up to rho), u |mx| for
            the rounding of the constant ln2/256 the shift is scaled back with, u |mx + log_norm| for the fma and u |logpdf| for
            the add.  Within 1 of the threshold the larger of the two is charged.
         G  log_norm = -sum_k log(L_kk sqrt(2 pi)) in fp64: per k the rounding of sqrt(2 pi), the multiply, the logarithm at
            1 ulp and the addition:  u sum_k (2 + 2 |g_k|) + (d - 1) u sum_k |g_k|,  g_k = log(L_kk sqrt(2 pi)).
  pdf    tol = pdf (rho + (2 d + 4) u) + 2^-1074 (1 + N norm):  norm = (2 pi)^(-d/2) / prod L_kk costs the rounding of 2 pi raised
         to the power d/2 (d/2 u), pow at 1 ulp (2 u), d divisions and the final multiply: at most (3 d / 2 + 3) u, charged as
         (2 d + 4) u; terms in the denormal range (and those exp2s_tab256 clamps to 0) are rounded to a multiple of 2^-1074 before
         norm scales them.

No constant here is fitted to device output.  The counts are worst cases of honest fp64 arithmetic, all errors first order in u
except where a closed form was as cheap (expm1, log1p); the terms of order (d u)^2 cond(L) left out are below 1e-9 of the bound
at every case of tests/kde_cases.py.  tests/test_kde_reference_host.py shows how slack the bound is per case, and
tests/test_gpu_kde_truth.py adds a statistical criterion for that reason.
"""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
EXTENDED = np.finfo(LD).nmant >= 63          # x87 80-bit (or wider); otherwise the mpmath route
U = 2.0 ** -53
TINY = 2.0 ** -1074
MP_DIGITS = 50
QUERY_STRIDE = 1 if EXTENDED else 16         # the mpmath route keeps every 16th query
CHUNK_BYTES = 100e6
E_EXP2S_TAB256 = 2 * 3 + 4                   # ceil(2.2) = 3; kernel_sum_reference.E_EXP2S_TAB256
KDE_TAIL = -650.0                            # kde.hip: largest exponent below this -> the shifted pass


def c_exponent(d, log_out):
    """Roundings of the augmented product charged u A each (module docstring)."""
    return d + 3 + (1 if log_out else 0)


def _live(logw):
    lw = np.asarray(logw, dtype=np.float64)
    return np.isfinite(lw)                   # -inf, NaN: weight zero (+inf is not a weight)


def forward_substitution(L, B, dtype=LD):
    """L^-1 B for lower-triangular L, row by row, vectorised over the trailing axes of B[d, ...]."""
    L = np.asarray(L, dtype=dtype); B = np.asarray(B, dtype=dtype)
    V = np.empty_like(B)
    for i in range(L.shape[0]):
        acc = B[i].copy()
        for j in range(i):
            acc -= L[i, j] * V[j]
        V[i] = acc / L[i, i]
    return V


def log_norm_ld(L):
    """-sum_k log(L_kk sqrt(2 pi)) in extended precision from the fp64 diagonal."""
    if not EXTENDED:
        import mpmath as mp
        with mp.workdps(MP_DIGITS):
            return LD(float(-mp.fsum(mp.log(mp.mpf(float(v)) * mp.sqrt(2 * mp.pi)) for v in np.diag(L))))
    two_pi = LD(8) * np.arctan(LD(1))
    return -np.sum(np.log(np.diag(np.asarray(L, dtype=np.float64)).astype(LD) * np.sqrt(two_pi)))


class Truth:
    """logpdf[M] (np.longdouble), mx[M] the largest exponent, arg[M] its sample, p[M, N] the softmax weights (float64),
    keep[M'] the query indices evaluated (all of them where long double is extended)."""

    def __init__(self, logpdf, mx, arg, p, keep):
        self.logpdf, self.mx, self.arg, self.p, self.keep = logpdf, mx, arg, p, keep

    @property
    def pdf(self):
        with np.errstate(under="ignore"):
            v = np.exp(self.logpdf)
        return np.where(v < LD(TINY), LD(0), v)


def truth(X, logw, L, Q, direct=False):
    """The Truth of every query (every QUERY_STRIDE-th one on the mpmath route)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64)); Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
    keep = np.arange(0, Q.shape[0], QUERY_STRIDE)
    if not EXTENDED:
        return truth_mp(X, logw, L, Q, keep)
    N, d = X.shape
    M = Q.shape[0]
    live = _live(logw)
    lw = np.where(live, np.asarray(logw, dtype=np.float64), 0.0).astype(LD)
    ln = log_norm_ld(L)
    out = np.empty(M, dtype=LD); mx = np.empty(M, dtype=LD); arg = np.empty(M, dtype=np.int64); p = np.empty((M, N))
    if not direct:
        a = X[0].astype(LD)
        zx = forward_substitution(L, (X.astype(LD) - a[None, :]).T)          # [d, N]
        zq = forward_substitution(L, (Q.astype(LD) - a[None, :]).T)          # [d, M]
    step = max(1, int(CHUNK_BYTES / (16 * 4 * N * (d if direct else 1))))
    for m0 in range(0, M, step):
        m1 = min(M, m0 + step)
        if direct:
            D = Q[m0:m1].astype(LD).T[:, :, None] - X.astype(LD).T[:, None, :]   # [d, m, N]: the differences themselves
            Y = forward_substitution(L, D)
            r2 = np.sum(Y * Y, axis=0)
        else:
            r2 = np.zeros((m1 - m0, N), dtype=LD)
            for k in range(d):
                df = zq[k, m0:m1][:, None] - zx[k][None, :]
                r2 += df * df
        ex = np.where(live[None, :], lw[None, :] - r2 / LD(2), -np.inf)
        top = ex.max(axis=1)
        with np.errstate(under="ignore"):
            t = np.exp(ex - top[:, None])
        s = t.sum(axis=1)
        out[m0:m1] = top + np.log(s) + ln
        mx[m0:m1] = top
        arg[m0:m1] = ex.argmax(axis=1)
        p[m0:m1] = (t / s[:, None]).astype(np.float64)
    return Truth(out, mx, arg, p, keep)


def truth_mp(X, logw, L, Q, keep=None, digits=MP_DIGITS):
    """The same quantities with mpmath at ``digits`` decimal digits, rounded once to np.longdouble at the end (the cross-check of
    the long-double routes, and the whole truth where long double is only a double)."""
    import mpmath as mp
    X = np.atleast_2d(np.asarray(X, dtype=np.float64)); Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
    N, d = X.shape
    keep = np.arange(Q.shape[0]) if keep is None else np.asarray(keep)
    live = _live(logw)
    out = np.empty(len(keep), dtype=LD); mx = np.empty(len(keep), dtype=LD); arg = np.empty(len(keep), dtype=np.int64)
    p = np.zeros((len(keep), N))
    with mp.workdps(digits):
        Lm = [[mp.mpf(float(L[i][j])) for j in range(i + 1)] for i in range(d)]
        ln = -mp.fsum(mp.log(Lm[k][k] * mp.sqrt(2 * mp.pi)) for k in range(d))

        def white(row):
            y = []
            for k in range(d):
                y.append((mp.mpf(float(row[k])) - mp.fdot(Lm[k][:k], y)) / Lm[k][k])
            return y

        # at 50 digits L^-1 q - L^-1 x IS L^-1 (q - x): a common offset of 1e4 costs 5 of the 50 digits
        zx = [white(row) if ok else None for row, ok in zip(X, live)]
        lwm = [mp.mpf(float(v)) if ok else None for v, ok in zip(np.asarray(logw, dtype=np.float64), live)]
        for i, m in enumerate(keep):
            zq = white(Q[m])
            ex = []
            for n in range(N):
                if lwm[n] is None:
                    ex.append(None)
                    continue
                ex.append(lwm[n] - mp.fsum((a - b) ** 2 for a, b in zip(zq, zx[n])) / 2)
            top = max(e for e in ex if e is not None)
            t = [mp.exp(e - top) if e is not None else mp.mpf(0) for e in ex]
            s = mp.fsum(t)
            out[i] = _mp_to_ld(top + mp.log(s) + ln)
            mx[i] = _mp_to_ld(top)
            arg[i] = max(range(N), key=lambda n: t[n])
            p[i] = [float(v / s) for v in t]
    return Truth(out, mx, arg, p, keep)


def _mp_to_ld(v):
    """Nearest long double of an mpf: the leading double plus the double nearest to the remainder."""
    hi = float(v)
    if hi == 0.0 or not math.isfinite(hi):
        return LD(hi)
    return LD(hi) + LD(float(v - hi))


def truth_logpdf(X, logw, L, Q):
    return truth(X, logw, L, Q).logpdf


def truth_pdf(X, logw, L, Q):
    return truth(X, logw, L, Q).pdf


# ------------------------------------------------------------------------------------------------------------- the bound
def _rho(X, logw, L, Q, tr, log_out):
    """rho[M'] of the module docstring for the queries tr.keep, and the pieces the callers add to it."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64)); Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))[tr.keep]
    L = np.asarray(L, dtype=np.float64)
    N, d = X.shape
    live = _live(logw)
    alw = np.where(live, np.abs(np.where(live, np.asarray(logw, dtype=np.float64), 0.0)), 0.0)
    Linv = np.abs(forward_substitution(L, np.eye(d)).astype(np.float64))
    La = np.abs(L)
    c = X.mean(axis=0)
    dc = U * ((N - 1) * np.abs(X).mean(axis=0) + np.abs(c))
    grow = Linv @ dc                                                          # |L^-1| dc: enlarges every magnitude
    xc, qc = X - c, Q - c
    z = forward_substitution(L, xc.T, np.float64).T                           # [N, d]
    u = forward_substitution(L, qc.T, np.float64).T                           # [M, d]
    za, ua = np.abs(z) + grow, np.abs(u) + grow
    dz = (d * U * (za @ La.T) + U * (np.abs(xc) + dc)) @ Linv.T               # [N, d]
    du = (d * U * (ua @ La.T) + U * (np.abs(qc) + dc)) @ Linv.T               # [M, d]
    hz = 0.5 * np.sum(za * za, axis=1) + alw
    hu = 0.5 * np.sum(ua * ua, axis=1)
    H = hu[:, None] + hz[None, :]
    A = ua @ za.T + H
    W = np.zeros_like(A)
    for k in range(d):
        W += np.abs(u[:, k][:, None] - z[:, k][None, :]) * (du[:, k][:, None] + dz[:, k][None, :])
    W += 0.5 * (np.linalg.norm(du, axis=1)[:, None] + np.linalg.norm(dz, axis=1)[None, :]) ** 2
    e = U * (c_exponent(d, log_out) * A + (d + 2) * H) + W
    rho = np.sum(tr.p * np.expm1(e + E_EXP2S_TAB256 * U), axis=1) + (N - 1) * U
    return rho


def tolerance_logpdf(X, logw, L, Q, tr=None):
    """tol[M'] (float64) for |logpdf - truth| at the queries tr.keep."""
    tr = truth(X, logw, L, Q) if tr is None else tr
    X = np.atleast_2d(X)
    N, d = X.shape
    rho = _rho(X, logw, L, Q, tr, True)
    g = np.abs(np.log(np.diag(np.asarray(L, dtype=np.float64)) * math.sqrt(2.0 * math.pi)))
    G = U * np.sum(2.0 + 2.0 * g) + (d - 1) * U * np.sum(g)
    ln = float(log_norm_ld(L))
    lp = tr.logpdf.astype(np.float64)
    mx = tr.mx.astype(np.float64)
    first = 2.0 * U * np.abs(lp - ln) + U * np.abs(lp)
    tail = 2.0 * U * (math.log(N) + 1.0) + U * np.abs(mx) + U * np.abs(mx + ln) + U * np.abs(lp)
    T = np.where(mx >= KDE_TAIL + 1.0, first, np.where(mx < KDE_TAIL - 1.0, tail, np.maximum(first, tail)))
    return -np.log1p(-rho) + T + G


def tolerance_pdf(X, logw, L, Q, tr=None):
    """tol[M'] (np.longdouble: not rounded to the 2^-1074 grid of the doubles) for |pdf - truth| at the queries tr.keep."""
    tr = truth(X, logw, L, Q) if tr is None else tr
    X = np.atleast_2d(X)
    N, d = X.shape
    rho = _rho(X, logw, L, Q, tr, False)
    norm = np.exp(log_norm_ld(L))
    return tr.pdf * LD(1) * (rho + (2 * d + 4) * U).astype(LD) + LD(TINY) * (LD(1) + LD(N) * norm)
