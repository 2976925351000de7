"""Extended-precision truth for the library's kernel sums  amp sum_n alpha_n k(q, x_n)  and for the predictive variance, with the
forward-error bound every evaluation path is held to (tests/test_kernel_sum_reference_host.py, tests/test_gpu_kernel_sums.py,
tests/test_gpu_variance_truth.py).  Plain NumPy (mpmath where ``np.longdouble`` is only a double); no GPU, nothing imported
from alabi_amd.

Inputs are the library's own fp64 numbers: the inverse length scales ``exp(-log_M / 2)``, the amplitude ``exp(log_amp)``, the
nugget ``exp(log_white_noise)`` (one libm ``exp`` each, as alabi_gp_set_hyper forms them), the scaled coordinates
``fl(x * inv_len)`` (ONE fp64 multiply, as every kernel forms them) and the device's alpha.  From there on everything is
evaluated in extended precision (64-bit significand, ~1e-19), so the reference is ~2000 times more precise than the fp64 code
under test and does not share its rounding.

The bound (``tolerance``), u = 2^-53, for query m:

    tol_m = u sum_n |term_mn| (E + (N - 1) + c A_mn)  +  2^-1074 (1 + amp sum_n |alpha_n|)

  E      relative roundings of one term outside the exponential's argument: twice the documented ulp figure of the path's
         exponential (gp_device.hpp: exp_neg_half / exp_direct 1.23 ulp, exp2s_tab256 2.2 ulp; exp_tab32 has the reduction of
         exp_neg_half with a shorter polynomial and one more multiply and is held to the same figure) rounded up, plus 4: the
         multiply by alpha, the multiply by amp, the combine of partial sums and the final fma.  8 for exp_neg_half, exp_direct
         and exp_tab32, 10 for exp2s_tab256.
  N - 1  the additions of the sum, worst case for ANY order (each addition loses at most u of a partial sum that is at most
         sum_n |term|).
  c A    the exponential's argument carries c roundings, each at most u A_mn in absolute value, and exp turns an absolute
         error of its argument into the same relative error of the term.
           difference form (gp_kernel_dot_block, the tile kernels, assemble_tile, alabi_kernel_matrix, the batched fit):
             df = x - q (relative u on df, 2u on df^2, together 2u r^2), then d fmas into r2 (u r^2 each at most); -r2/2 is
             exact.  c = d + 2, A = r^2 / 2.
           augmented dot product about the training mean (predict_mean_mfma_kernel, ens_group_kernel): c = d + 3, the count the
             issue states: the d + 2 accumulations of the matrix core (q_k x_k, 1 * (-|x|^2/2), (-|q|^2/2) * 1) and the scaling
             of the operand by 256/ln2, each charged u A,
             A = sum_k |q_k x_k| + |q|^2/2 + |x|^2/2 in coordinates relative to the training mean.  A strict worst-case count
             also charges the centring (x - c, q - c: one rounding per coordinate, 2 u A in all) and the d fmas of each half
             norm (d u of their own part of A), 2 d + 5 in all; d + 3 is the tighter of the two and is what the tests assert.
             Should a path ever miss it, the strict count is the re-count.
           se_pair_terms (half-step, stream, pair and nested kernels): nhq - h, then d fmas: d + 1 roundings, the half norm
             of q and h's own rounding: d + 3 as well; overwriting bit 0 of h with the sign of alpha moves h by one ulp, i.e.
             by at most 2 u |h|: A gains 2 |h_n|.
           Matern / rational quadratic (library exp / log1p, <= 1 ulp each in the HIP math tables): the argument is
             s = sqrt(3 r2) or sqrt(5 r2): half the relative error (d + 2) u of r2, the multiply and the square root,
             c = ceil((d + 2) / 2) + 2, A = s; or alpha log1p(r2 / (2 alpha)): r2 (d + 2), the divide, log1p's ulp and its
             rounding, the multiply, c = d + 6, A = alpha log1p(r2 / (2 alpha)).  E = 2 * 1 + 4 plus the roundings of the
             polynomial in front of the exponential: 2 (Matern-3/2), 5 (Matern-5/2), 0 (rational quadratic).
  2^-1074 (1 + amp sum |alpha|)   terms in the denormal range are rounded to a multiple of 2^-1074 before alpha and amp scale
         them.

No constant here is fitted to device output.  The counts are worst cases of honest fp64 arithmetic; the host test shows that
plain NumPy restatements of both forms come within a factor two of the bound, i.e. that it is attainable and not slack.
"""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
EXTENDED = np.finfo(LD).nmant >= 63          # x87 80-bit (or wider); otherwise the mpmath route below
U = 2.0 ** -53
TINY = 2.0 ** -1074
MP_DIGITS = 50
QUERY_STRIDE = 1 if EXTENDED else 16         # the mpmath route keeps every 16th query
CHUNK_BYTES = 200e6

FAMILIES = ("ExpSquaredKernel", "Matern32Kernel", "Matern52Kernel", "RationalQuadraticKernel")
# (E, c(d)) per path; see the module docstring
E_EXP_NEG_HALF = E_EXP_DIRECT = E_EXP_TAB32 = 2 * 2 + 4          # ceil(1.23) = 2
E_EXP2S_TAB256 = 2 * 3 + 4                                       # ceil(2.2) = 3
E_FAMILY = {"ExpSquaredKernel": E_EXP_NEG_HALF, "Matern32Kernel": 2 * 1 + 4 + 2, "Matern52Kernel": 2 * 1 + 4 + 5,
            "RationalQuadraticKernel": 2 * 1 + 4}


# roundings of the argument after r2 is formed (the multiply and the square root; the divide, log1p twice and the multiply)
C_FAMILY_OWN = {"ExpSquaredKernel": 0, "Matern32Kernel": 2, "Matern52Kernel": 2, "RationalQuadraticKernel": 4}


def c_difference(d, family="ExpSquaredKernel"):
    if family in ("Matern32Kernel", "Matern52Kernel"):
        return (d + 3) // 2 + 2                     # the square root halves the relative error of r2
    return d + 2 + C_FAMILY_OWN[family]


def c_dot(d):
    return d + 3


def hyper_fp64(log_amp, log_white_noise, log_M):
    """(amp, wn, inv_len) as the library forms them: one libm exp each (alabi_gp_set_hyper, launch_predict_mean)."""
    return (math.exp(log_amp), math.exp(log_white_noise),
            np.array([math.exp(-0.5 * float(v)) for v in np.ravel(log_M)], dtype=np.float64))


def scaled(X, inv_len):
    """fl(x * inv_len): the one fp64 multiply every kernel applies to its inputs."""
    return np.atleast_2d(np.asarray(X, dtype=np.float64)) * np.asarray(inv_len, dtype=np.float64)[None, :]


def _rows_per_chunk(N, itemsize=16, live=4):
    return max(1, int(CHUNK_BYTES / (itemsize * live * max(N, 1))))


def _r2(qs, xs, dtype):
    """[m, n] squared distances of already scaled rows, accumulated coordinate by coordinate in ``dtype``."""
    q = qs.astype(dtype); x = xs.astype(dtype)
    r2 = np.zeros((q.shape[0], x.shape[0]), dtype=dtype)
    for k in range(q.shape[1]):
        df = q[:, k][:, None] - x[:, k][None, :]
        r2 += df * df
    return r2


def _radial_ld(r2, family, log_alpha):
    if family == "ExpSquaredKernel":
        return np.exp(-r2 / LD(2))
    if family == "Matern32Kernel":
        s = np.sqrt(LD(3) * r2)
        return (LD(1) + s) * np.exp(-s)
    if family == "Matern52Kernel":
        s = np.sqrt(LD(5) * r2)
        return (LD(1) + s + s * s / LD(3)) * np.exp(-s)
    if family == "RationalQuadraticKernel":
        a = LD(math.exp(log_alpha))
        return np.exp(-a * np.log1p(r2 / (LD(2) * a)))
    raise ValueError(family)


def kernel_sum(X, alpha, amp, inv_len, Q, family="ExpSquaredKernel", log_alpha=1.0):
    """(ref[M], terms[M, N]) in np.longdouble: terms[m, n] = alpha_n amp k(q_m, x_n), ref = terms.sum(1).  X, Q: raw inputs;
    inv_len, amp: hyper_fp64's.  Queries go through in chunks so that no temporary exceeds ~200 MB."""
    if not EXTENDED:
        return kernel_sum_mp(X, alpha, amp, inv_len, Q, family, log_alpha, MP_DIGITS)
    xs, qs = scaled(X, inv_len), scaled(Q, inv_len)
    w = np.asarray(alpha, dtype=np.float64).astype(LD) * LD(amp)
    M, N = qs.shape[0], xs.shape[0]
    terms = np.empty((M, N), dtype=LD)
    step = _rows_per_chunk(N)
    for m0 in range(0, M, step):
        terms[m0:m0 + step] = _radial_ld(_r2(qs[m0:m0 + step], xs, LD), family, log_alpha) * w[None, :]
    return terms.sum(axis=1), terms


def kernel_sum_mp(X, alpha, amp, inv_len, Q, family="ExpSquaredKernel", log_alpha=1.0, digits=MP_DIGITS):
    """The same sum with mpmath at ``digits`` decimal digits, rounded once to np.longdouble at the end (element by element:
    for the cross-check of the long-double route, and the whole reference where long double is only a double)."""
    import mpmath as mp
    xs, qs = scaled(X, inv_len), scaled(Q, inv_len)
    M, N = qs.shape[0], xs.shape[0]
    terms = np.empty((M, N), dtype=LD)
    ref = np.empty(M, dtype=LD)
    with mp.workdps(digits):
        w = [mp.mpf(float(a)) * mp.mpf(float(amp)) for a in np.asarray(alpha, dtype=np.float64)]
        xm = [[mp.mpf(float(v)) for v in row] for row in xs]
        a = mp.mpf(math.exp(log_alpha))                       # the library's fp64 alpha, not the exact exponential
        for m in range(M):
            q = [mp.mpf(float(v)) for v in qs[m]]
            tot = mp.mpf(0)
            for n in range(N):
                r2 = mp.fsum((qk - xk) ** 2 for qk, xk in zip(q, xm[n]))
                if family == "ExpSquaredKernel":
                    f = mp.exp(-r2 / 2)
                elif family == "Matern32Kernel":
                    s = mp.sqrt(3 * r2); f = (1 + s) * mp.exp(-s)
                elif family == "Matern52Kernel":
                    s = mp.sqrt(5 * r2); f = (1 + s + s * s / 3) * mp.exp(-s)
                elif family == "RationalQuadraticKernel":
                    f = mp.exp(-a * mp.log1p(r2 / (2 * a)))
                else:
                    raise ValueError(family)
                t = w[n] * f
                tot += t
                terms[m, n] = _mp_to_ld(t)
            ref[m] = _mp_to_ld(tot)
    return ref, terms


def _mp_to_ld(v):
    """Nearest long double of an mpf: the leading double plus the double nearest to the remainder."""
    hi = float(v)
    if hi == 0.0 or not math.isfinite(hi):
        return LD(hi)
    return LD(hi) + LD(float(v - hi))


# ------------------------------------------------------------------------------------------------- argument magnitudes
def arg_difference(X, inv_len, Q, family="ExpSquaredKernel", log_alpha=1.0):
    """A[m, n] of the difference form (fp64 is ample for a magnitude): r^2/2; the exponential's argument for the other families."""
    r2 = _r2(scaled(Q, inv_len), scaled(X, inv_len), np.float64)
    if family == "ExpSquaredKernel":
        return 0.5 * r2
    if family == "Matern32Kernel":
        return np.sqrt(3.0 * r2)
    if family == "Matern52Kernel":
        return np.sqrt(5.0 * r2)
    a = math.exp(log_alpha)
    return a * np.log1p(0.5 * r2 / a)


def arg_dot(X, inv_len, Q, alpha=None):
    """A[m, n] of the two dot-product forms: sum_k |q_k x_nk| + |q|^2/2 + |x_n|^2/2 in coordinates relative to the mean of the
    scaled training inputs (xa_centre_kernel, ens_se_prepare_kernel).  With ``alpha`` (se_pair_terms): + 2 |h_n|,
    h_n = |x_n|^2/2 - ln|alpha_n|."""
    xs, qs = scaled(X, inv_len), scaled(Q, inv_len)
    c = xs.mean(axis=0)
    xc, qc = xs - c, qs - c
    hx = 0.5 * np.sum(xc * xc, axis=1)
    A = np.abs(qc) @ np.abs(xc).T + 0.5 * np.sum(qc * qc, axis=1)[:, None] + hx[None, :]
    if alpha is not None:
        al = np.abs(np.asarray(alpha, dtype=np.float64))
        with np.errstate(divide="ignore"):
            h = np.where(al > 0, hx - np.log(al), 0.0)
        A = A + 2.0 * np.abs(h)[None, :]
    return A


def tolerance(terms, A, E, c, alpha, amp, dtype=np.float64):
    """tol[M] of the module docstring in ``dtype`` (np.longdouble where the bound itself must not be rounded to the 2^-1074 grid
    of the doubles).  terms[M, N] from kernel_sum, A[M, N] (or None for c = 0)."""
    if dtype is not np.float64:
        t = np.abs(np.asarray(terms, dtype=dtype))
        w = dtype(E + (t.shape[1] - 1)) + (dtype(0) if A is None else dtype(c) * np.asarray(A, dtype=dtype))
        return dtype(U) * np.sum(t * w, axis=1) + dtype(TINY) * (dtype(1) + dtype(amp) * dtype(np.sum(np.abs(np.asarray(alpha, dtype=np.float64)))))
    t = np.abs(np.asarray(terms)).astype(np.float64)
    N = t.shape[1]
    w = float(E + (N - 1)) + (0.0 if A is None else float(c) * np.asarray(A, dtype=np.float64))
    return U * np.sum(t * w, axis=1) + TINY * (1.0 + float(amp) * float(np.sum(np.abs(np.asarray(alpha, dtype=np.float64)))))


# ------------------------------------------------------------------------------------------ Cholesky and the variance
def kernel_matrix(X, amp, wn, inv_len, family="ExpSquaredKernel", log_alpha=1.0):
    """K = amp f(r2) + wn I in extended precision from the library's fp64 inputs."""
    if not EXTENDED:
        return _kernel_matrix_mp(X, None, amp, wn, inv_len, family, log_alpha)
    xs = scaled(X, inv_len)
    K = LD(amp) * _radial_ld(_r2(xs, xs, LD), family, log_alpha)
    K[np.diag_indices_from(K)] += LD(wn)
    return K


def cross_matrix(X, amp, inv_len, Q, family="ExpSquaredKernel", log_alpha=1.0):
    """K*[N, M] = amp f(r2(x_n, q_m)) in extended precision."""
    if not EXTENDED:
        return _kernel_matrix_mp(X, Q, amp, 0.0, inv_len, family, log_alpha)
    return LD(amp) * _radial_ld(_r2(scaled(X, inv_len), scaled(Q, inv_len), LD), family, log_alpha)


def cholesky(K):
    """Lower Cholesky factor in the precision of K: the column loop, each column's update vectorised over its rows."""
    if K.dtype == object:
        return _cholesky_obj(K)
    K = np.asarray(K, dtype=LD)
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        row = L[j, :j]
        piv = K[j, j] - np.sum(row * row)
        if not piv > 0:
            raise np.linalg.LinAlgError(f"{j + 1}-th leading minor of the array is not positive definite")
        L[j, j] = np.sqrt(piv)
        if j + 1 < n:
            L[j + 1:, j] = (K[j + 1:, j] - (L[j + 1:, :j] * row[None, :]).sum(axis=1)) / L[j, j]
    return L


def variance(L, kstar, amp):
    """sigma^2[M] = amp - |L^-1 k*|^2: forward substitution down the rows of L, vectorised over the M columns of kstar[N, M].
    Returned as float64 (the nearest double of the extended-precision value)."""
    if L.dtype == object:
        return _variance_obj(L, kstar, amp)
    V = forward_substitution(L, kstar)
    return (LD(amp) - (V * V).sum(axis=0)).astype(np.float64)


def forward_substitution(L, B):
    """L^-1 B for lower-triangular L, row by row, vectorised over the columns of B[N, M] (long double route only)."""
    L = np.asarray(L, dtype=LD); B = np.asarray(B, dtype=LD)
    V = np.empty_like(B)
    for i in range(L.shape[0]):
        V[i] = (B[i] - (L[i, :i][:, None] * V[:i]).sum(axis=0)) / L[i, i]
    return V


# mpmath route (object arrays of mpf): the same algorithms, for platforms whose long double is a double
def _kernel_matrix_mp(X, Q, amp, wn, inv_len, family, log_alpha):
    import mpmath as mp
    xs = scaled(X, inv_len)
    qs = xs if Q is None else scaled(Q, inv_len)
    out = np.empty((xs.shape[0], qs.shape[0]), dtype=object)
    with mp.workdps(MP_DIGITS):
        a = mp.mpf(math.exp(log_alpha))
        for i in range(xs.shape[0]):
            xi = [mp.mpf(float(v)) for v in xs[i]]
            for j in range(qs.shape[0]):
                r2 = mp.fsum((u - mp.mpf(float(v))) ** 2 for u, v in zip(xi, qs[j]))
                if family == "ExpSquaredKernel":
                    f = mp.exp(-r2 / 2)
                elif family == "Matern32Kernel":
                    s = mp.sqrt(3 * r2); f = (1 + s) * mp.exp(-s)
                elif family == "Matern52Kernel":
                    s = mp.sqrt(5 * r2); f = (1 + s + s * s / 3) * mp.exp(-s)
                else:
                    f = mp.exp(-a * mp.log1p(r2 / (2 * a)))
                out[i, j] = mp.mpf(float(amp)) * f + (mp.mpf(float(wn)) if (Q is None and i == j) else 0)
    return out


def _cholesky_obj(K):
    import mpmath as mp
    n = K.shape[0]
    L = np.empty((n, n), dtype=object); L[:] = mp.mpf(0)
    with mp.workdps(MP_DIGITS):
        for j in range(n):
            piv = K[j, j] - sum((v * v for v in L[j, :j]), mp.mpf(0))
            if not piv > 0:
                raise np.linalg.LinAlgError(f"{j + 1}-th leading minor of the array is not positive definite")
            L[j, j] = mp.sqrt(piv)
            for i in range(j + 1, n):
                L[i, j] = (K[i, j] - sum((a * b for a, b in zip(L[i, :j], L[j, :j])), mp.mpf(0))) / L[j, j]
    return L


def _variance_obj(L, kstar, amp):
    import mpmath as mp
    n, M = kstar.shape
    out = np.empty(M, dtype=np.float64)
    with mp.workdps(MP_DIGITS):
        for m in range(M):
            v = []
            for i in range(n):
                v.append((kstar[i, m] - sum((a * b for a, b in zip(L[i, :i], v)), mp.mpf(0))) / L[i, i])
            out[m] = float(mp.mpf(float(amp)) - sum((x * x for x in v), mp.mpf(0)))
    return out


# ---------------------------------------------------------------------------------------- fp64 restatements of the two forms
def difference_form_fp64(X, alpha, amp, inv_len, Q):
    """The difference form in plain fp64 NumPy, in the kernels' operation order: r2 += (x - q)^2 per coordinate, exp(-r2/2),
    times alpha, summed over n, times amp."""
    xs, qs = scaled(X, inv_len), scaled(Q, inv_len)
    r2 = np.zeros((qs.shape[0], xs.shape[0]))
    for k in range(xs.shape[1]):
        df = xs[:, k][None, :] - qs[:, k][:, None]
        r2 = df * df + r2
    f = np.exp(-0.5 * r2) * np.asarray(alpha, dtype=np.float64)[None, :]
    return amp * np.sum(f, axis=1)


def centred_dot_form_fp64(X, alpha, amp, inv_len, Q):
    """The augmented dot product about the training mean in plain fp64 NumPy: exp(q.x - |q|^2/2 - |x|^2/2), centred coordinates."""
    xs, qs = scaled(X, inv_len), scaled(Q, inv_len)
    c = xs.mean(axis=0)
    xc, qc = xs - c, qs - c
    hx = -0.5 * np.sum(xc * xc, axis=1)
    hq = -0.5 * np.sum(qc * qc, axis=1)
    arg = np.zeros((qs.shape[0], xs.shape[0]))
    for k in range(xs.shape[1]):
        arg = qc[:, k][:, None] * xc[:, k][None, :] + arg
    arg = (arg + hx[None, :]) + hq[:, None]
    f = np.exp(arg) * np.asarray(alpha, dtype=np.float64)[None, :]
    return amp * np.sum(f, axis=1)


# ------------------------------------------------------------------------------------------------ the shared case grid
def rays(X, inv_len, M, seed, rmax=56.0):
    """M queries on rays from randomly chosen training points in random directions, scaled radius linspace(0, 1, M)^1.5 rmax
    (r^2 from 0 through the denormal range of exp(-r^2/2) to exact underflow), plus three at 1e3, 1e6 and 1e9 length scales."""
    rng = np.random.RandomState(seed)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    N, d = X.shape
    base = X[rng.randint(0, N, M)]
    u = rng.randn(M, d)
    u /= np.linalg.norm(u, axis=1)[:, None]
    rad = np.linspace(0.0, 1.0, M) ** 1.5 * rmax
    Q = base + (rad[:, None] * u) / np.asarray(inv_len)[None, :]
    far = np.array([[s / inv_len[k] for k in range(d)] for s in (1e3, 1e6, 1e9)]) / np.sqrt(d) + X.mean(axis=0)[None, :]
    return np.vstack([Q, far])


def lattice(n=130, d=3, spacing=9.0, inv_len=None):
    """n points of a cubic lattice in d dimensions, ``spacing`` length scales apart (K is diagonal to rounding), positive targets."""
    side = int(np.ceil(n ** (1.0 / d)))
    idx = np.stack(np.meshgrid(*([np.arange(side)] * d), indexing="ij"), axis=-1).reshape(-1, d)[:n]
    inv_len = np.ones(d) if inv_len is None else np.asarray(inv_len)
    X = (idx - 0.5 * (side - 1)) * spacing / inv_len[None, :]
    y = 1.0 + 0.5 * np.cos(0.7 * np.arange(n))
    return X, y
