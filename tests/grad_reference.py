"""Extended-precision truth for the library's gradients with respect to the query point -- d mu / d x, d var / d x and the
gradient of the ensemble's fused log-probability -- with the bounds every evaluation path is held to
(tests/test_grad_reference_host.py, tests/test_gpu_grad_truth.py).  Plain NumPy (mpmath where ``np.longdouble`` is only a
double); no GPU, nothing imported from alabi_amd.  It extends tests/kernel_sum_reference.py (``ksr``) and keeps its input
convention: the hyper-parameters of ``ksr.hyper_fp64``, the scaled coordinates ``fl(x * inv_len)`` and the device's own fp64
alpha are the inputs; everything after that runs in ``ksr.LD`` (64-bit significand), or in mpmath at ``ksr.MP_DIGITS`` digits on
every ``ksr.QUERY_STRIDE``-th query where ``ksr.EXTENDED`` is false.  Because alpha is an input, the mean gradient's truth isolates
the SUM and does not share the solve's conditioning.

With s = scaled coordinates, r2 = |s_q - s_n|^2 and f the radial profile (k = amp f(r2)):

    dk_n / dx_c  = 2 amp f'(r2_n) (s_qc - s_nc) inv_len_c
    dmu / dx_c   = sum_n alpha_n dk_n/dx_c                           (``mean_gradient``)
    dvar / dx_c  = -2 sum_n z_n dk_n/dx_c,  z = K^-1 k* = L^-T L^-1 k*   (``variance_gradient``)
    f'(r2): -f/2 (squared exponential), -(3/2) e^-s with s = sqrt(3 r2) (Matern-3/2), -(5/6)(1 + s) e^-s with s = sqrt(5 r2)
            (Matern-5/2), -(1/2) (1 + u)^(-a - 1) with u = r2 / (2 a) (rational quadratic)         (``radial_slope``)


The mean gradient's bound (``mean_gradient_tolerance``), u = 2^-53, per query m and coordinate c
--------------------------------------------------------------------------------------------------

    tol_mc = u sum_n |term_mnc| (E_g + (N - 1) + c A_mn + c2 A2_mn)  +  2^-1074 * 2 sum_n P_mnc

  N - 1, c, A   as in ksr: the additions of the sum in ANY order (adding the zeros of idle lanes is exact), and the c roundings
                of the exponential's argument, each at most u A (difference form: ``ksr.c_difference``, ``ksr.arg_difference``).
                For the Matern slopes the sensitivity to s of the polynomial in front works AGAINST that of e^-s
                (d ln|f'| / d ln s = s / (1 + s) - s for Matern-5/2, -s for Matern-3/2), so c A covers the slope as it covers the
                value.
  c2 A2         rational quadratic only.  f' = -(1/2) (1 + u)^(-a - 1): an error of relative size delta in u moves ln|f'| by
                (a + 1) u / (1 + u) delta.  a u / (1 + u) <= a log1p(u) = A is inside c A; the remaining u / (1 + u) = A2 is
                charged the roundings of u: the d + 2 of r2 and the divide by a (0.5 * r2 is exact), c2 = d + 3.  Zero otherwise.
  E_g           relative roundings of one term outside the exponential's argument, counted in pgrad_final_kernel
                (gp_predict_grad.hip), rounding by rounding:
                  the exponential          2 ceil(ulp) as in ksr: 4 for exp_neg_half (1.23 ulp), 2 for the library exp
                  the slope's polynomial   squared exponential 0 (-0.5 * f is exact); Matern-3/2 1 (-1.5 * e); Matern-5/2 4 (the
                                           constant 5/6, 1 + r, and two multiplies); rational quadratic 2 (1 + u and the divide;
                                           -0.5 * f is exact)
                  df = q_c - x_c           1
                  g = 2 amp f'             1 (2.0 * amp is exact)
                  ga = alpha g             1
                  fma(ga, df, sum)         1 (the product inside the fma is exact; its addition is charged here once more, on
                                           top of N - 1, as ksr charges "the final fma")
                  combine of wave partials 1 (as ksr charges it: the four wave totals are added in a fixed order)
                  t * inv_len_c            1
                E_g = exponential + polynomial + 6:  10, 9, 12, 10 for the four families.
                lp_grad_eval (ens_grad_device.hpp) has the same count by other steps: x - q (1), w = -2 alpha f' (1; -2 alpha is
                exact), fma (1), amp * inv_len (1), times the sum (1), and the fold fl(lp_scale amp) of lp_grad_args (1) in place
                of the combine (one wave sums a coordinate).  ``E_LP`` = ``E_G``.
  2^-1074 ...   a value in the denormal range is rounded to a multiple of 2^-1074 instead of relatively.  That can happen to f', g,
                ga and the partial sums (four places, at most 2^-1075 each, hence the 2); what follows multiplies it by at most
                P_mnc = max(1, 2 amp) max(1, |alpha_n|) max(1, |df_mnc|) max(1, inv_len_c).

The log-probability's gradient (``log_prob_gradient_tolerance``), with a = lp_scale, b = lp_shift, M = a mu + b:

    identity   g = a dmu:            tol = mean_gradient_tolerance of the terms scaled by |a|  (the fold's rounding is in E_LP)
    y map      L = -+10^M, g = ln10 L a dmu:
                 tol = ln10 |L| tol_dmu  +  ln10 |a dmu| dL  +  3 u |g|
               3: the constant ln10, times L, times the gradient.  dL = ln10 |L| dM + 2 u |L| (pow: 2 ulp charged), and
               dM = ksr.tolerance of the value's terms scaled by |a| with E = ksr.E_FAMILY + 1 (the fold of amp)
                    + u (|M| + |fma(a, mean, b)|): the fma that adds the folded mean, and that mean's own rounding.
    prior      g_k -= (q_k - m_k) / s_k^2, evaluated as (q - m) * is * is with is = fl(1 / s):
                 tol += u (5 |p_k| + |g_k|),  p_k the prior's term
               5: the subtraction, the two multiplies (the three roundings of the expression) and the rounding of the reciprocal,
               which enters twice; u |g_k| is the subtraction from the gradient.

The variance gradient's bound (``variance_gradient_bound``): see its docstring.  No constant anywhere here is fitted to device
output; tests/test_grad_reference_host.py shows that honest fp64 restatements lie inside every bound and that planted defects
lie outside.
"""
from __future__ import annotations

import math

import numpy as np

import kernel_sum_reference as ksr
import solve_reference as sr

LD = ksr.LD
U, TINY = ksr.U, ksr.TINY
LN10_STR = "2.302585092994045684017991454684364207601"

E_EXP = {"ExpSquaredKernel": 4, "Matern32Kernel": 2, "Matern52Kernel": 2, "RationalQuadraticKernel": 2}
E_SLOPE_POLY = {"ExpSquaredKernel": 0, "Matern32Kernel": 1, "Matern52Kernel": 4, "RationalQuadraticKernel": 2}
E_G = {f: E_EXP[f] + E_SLOPE_POLY[f] + 6 for f in ksr.FAMILIES}
E_LP = dict(E_G)


# --------------------------------------------------------------------------------------------------------------- the slopes
def radial_slope(r2, family, log_alpha=1.0):
    """f'(r2) in the precision of r2: np.longdouble arrays, or object arrays of mpf (inside an mp.workdps block)."""
    r2 = np.asarray(r2)
    if r2.dtype == object:
        import mpmath as mp
        a = mp.mpf(math.exp(log_alpha))

        def one(v):
            if family == "ExpSquaredKernel":
                return -mp.exp(-v / 2) / 2
            if family == "Matern32Kernel":
                return -mp.mpf(3) / 2 * mp.exp(-mp.sqrt(3 * v))
            if family == "Matern52Kernel":
                s = mp.sqrt(5 * v)
                return -mp.mpf(5) / 6 * (1 + s) * mp.exp(-s)
            if family == "RationalQuadraticKernel":
                u = v / (2 * a)
                return -mp.exp(-(a + 1) * mp.log1p(u)) / 2
            raise ValueError(family)
        return np.array([one(v) for v in r2.ravel()], dtype=object).reshape(r2.shape)
    r2 = r2.astype(LD)
    if family == "ExpSquaredKernel":
        return -np.exp(-r2 / LD(2)) / LD(2)
    if family == "Matern32Kernel":
        return -LD(3) / LD(2) * np.exp(-np.sqrt(LD(3) * r2))
    if family == "Matern52Kernel":
        s = np.sqrt(LD(5) * r2)
        return -LD(5) / LD(6) * (LD(1) + s) * np.exp(-s)
    if family == "RationalQuadraticKernel":
        a = LD(math.exp(log_alpha))
        return -np.exp(-(a + LD(1)) * np.log1p(r2 / (LD(2) * a))) / LD(2)
    raise ValueError(family)


def _mp_array(a):
    import mpmath as mp
    a = np.asarray(a, dtype=np.float64)
    return np.array([mp.mpf(float(v)) for v in a.ravel()], dtype=object).reshape(a.shape)


def _to_ld(a):
    """Object arrays of mpf rounded to the nearest long doubles; anything else as long double."""
    a = np.asarray(a)
    if a.dtype != object:
        return a.astype(LD)
    return np.array([_mp_to_ld(v) for v in a.ravel()], dtype=LD).reshape(a.shape)


def _mp_to_ld(v):
    """Nearest long double of an mpf through its mantissa and exponent (ksr._mp_to_ld goes through a double, whose range ends
    where the far queries' terms begin)."""
    import mpmath as mp
    if v == 0:
        return LD(0)
    m, e = mp.frexp(v)
    hi = float(m)
    return np.ldexp(LD(hi) + LD(float(m - hi)), int(e))


def kernel_gradient(X, amp, inv_len, Q, family="ExpSquaredKernel", log_alpha=1.0, mp_digits=None):
    """dks[M, N, d] = dk_n / dx_c at query m in extended precision (``mp_digits``: by mpmath at that many digits, rounded once to
    long double at the end)."""
    xs, qs = ksr.scaled(X, inv_len), ksr.scaled(Q, inv_len)
    if mp_digits is None and ksr.EXTENDED:
        df = qs.astype(LD)[:, None, :] - xs.astype(LD)[None, :, :]
        slope = LD(2) * LD(amp) * radial_slope((df * df).sum(axis=2), family, log_alpha)
        return slope[:, :, None] * df * np.asarray(inv_len, dtype=np.float64).astype(LD)[None, None, :]
    import mpmath as mp
    with mp.workdps(mp_digits or ksr.MP_DIGITS):
        df = _mp_array(qs)[:, None, :] - _mp_array(xs)[None, :, :]
        slope = 2 * mp.mpf(float(amp)) * radial_slope((df * df).sum(axis=2), family, log_alpha)
        return _to_ld(slope[:, :, None] * df * _mp_array(inv_len)[None, None, :])


def mean_gradient(X, alpha, amp, inv_len, Q, family="ExpSquaredKernel", log_alpha=1.0, mp_digits=None, dks=None):
    """(ref[M, d], terms[M, N, d]) in np.longdouble: term_mnc = alpha_n 2 amp f'(r2_mn) (s_mc - s_nc) inv_len_c.  ``dks``: a
    cached ``kernel_gradient`` of the same inputs (the truth is linear in alpha)."""
    if dks is None:
        dks = kernel_gradient(X, amp, inv_len, Q, family, log_alpha, mp_digits)
    terms = dks * np.asarray(alpha, dtype=np.float64).astype(LD)[None, :, None]
    return terms.sum(axis=1), terms


def backward_substitution(L, B):
    """L^-T B for lower-triangular L, row by row from the last, vectorised over the columns of B[N, M] (the counterpart of
    ``ksr.forward_substitution``; long double, or object arrays of mpf)."""
    dt = object if L.dtype == object else LD
    L = np.asarray(L, dtype=dt); B = np.asarray(B, dtype=dt)
    V = np.empty_like(B)
    n = L.shape[0]
    for i in range(n - 1, -1, -1):
        V[i] = (B[i] - (L[i + 1:, i][:, None] * V[i + 1:]).sum(axis=0)) / L[i, i]
    return V


def _forward(L, B):
    if L.dtype != object:
        return ksr.forward_substitution(L, B)
    V = np.empty_like(B)
    for i in range(L.shape[0]):
        V[i] = (B[i] - (L[i, :i][:, None] * V[:i]).sum(axis=0)) / L[i, i]
    return V


def solve_z(L, ks):
    """z[N, M] = L^-T L^-1 k* in the precision of L."""
    return backward_substitution(L, _forward(L, np.asarray(ks, dtype=L.dtype if L.dtype == object else LD)))


def variance_gradient(L, X, amp, inv_len, Q, family="ExpSquaredKernel", log_alpha=1.0, mp_digits=None, dks=None, z=None):
    """(ref[M, d], terms[M, N, d]) in np.longdouble: term_mnc = -2 z_nm dk_n/dx_c, z = L^-T L^-1 k* with the extended-precision
    factor ``L`` of ``ksr.cholesky(ksr.kernel_matrix(...))``.  ``mp_digits``: L is an object array of mpf and everything runs in
    mpmath at that many digits."""
    if L.dtype == object:
        import mpmath as mp
        with mp.workdps(mp_digits or ksr.MP_DIGITS):
            ks = ksr._kernel_matrix_mp(X, Q, amp, 0.0, inv_len, family, log_alpha)
            z = _to_ld(solve_z(L, ks))
    elif z is None:
        z = solve_z(L, ksr.cross_matrix(X, amp, inv_len, Q, family, log_alpha))
    if dks is None:
        dks = kernel_gradient(X, amp, inv_len, Q, family, log_alpha, mp_digits)
    terms = LD(-2) * np.asarray(z, dtype=LD).T[:, :, None] * dks
    return terms.sum(axis=1), terms


# ----------------------------------------------------------------------------------------------------- the log-probability
def log_prob_gradient(X, alpha, amp, inv_len, Q, mean, family="ExpSquaredKernel", log_alpha=1.0, affine=(1.0, 0.0), ymap=None,
                      prior=None, dks=None):
    """The chain rule of lp_grad_eval in extended precision, never rounded to fp64 on the way: a dict with
      grad[M, d]   a dmu  (times ln10 L under a y map)  minus (q - m) / s^2 on the coordinates with a normal prior
      lp[M]        a mu + b, mapped (-+10^.), plus the normal priors' log-densities            (no box gate)
      gterms, vterms   the mean gradient's and the value's terms scaled by a;  M_aff = a mu + b;  L;  dmu_a = a dmu;  prior_grad
    which is what ``log_prob_gradient_tolerance`` reads.  ``mean``: the GP's constant mean; ``affine`` = (lp_scale, lp_shift);
    ``ymap`` None / "nlog" / "log"; ``prior`` = (mean[d], std[d]) with NaN where there is none."""
    a, b = LD(float(affine[0])), LD(float(affine[1]))
    dmu, gterms = mean_gradient(X, alpha, amp, inv_len, Q, family, log_alpha, dks=dks)
    val, vterms = ksr.kernel_sum(X, alpha, amp, inv_len, Q, family, log_alpha)
    M_aff = a * (LD(float(mean)) + val) + b
    dmu_a, gterms, vterms = a * dmu, a * gterms, a * vterms
    L, grad = M_aff, dmu_a
    if ymap is not None:
        ln10 = LD(LN10_STR)
        L = (LD(-1) if ymap == "nlog" else LD(1)) * np.exp(ln10 * M_aff)
        grad = ln10 * L[:, None] * dmu_a
    lp = L
    pg = np.zeros_like(grad)
    if prior is not None:
        pm, ps = (np.asarray(v, dtype=np.float64) for v in prior)
        q = np.atleast_2d(np.asarray(Q, dtype=np.float64)).astype(LD)
        for k in np.nonzero(np.isfinite(pm) & np.isfinite(ps) & (ps > 0))[0]:
            t = (q[:, k] - LD(pm[k])) / LD(ps[k])
            lp = lp + (-t * t / LD(2) - np.log(LD(ps[k])) - LD("0.91893853320467274178032973640561763986"))
            pg[:, k] = -(q[:, k] - LD(pm[k])) / (LD(ps[k]) * LD(ps[k]))
        grad = grad + pg
    return dict(grad=grad, lp=lp, gterms=gterms, vterms=vterms, M_aff=M_aff, L=L, dmu_a=dmu_a, prior_grad=pg)


# --------------------------------------------------------------------------------------------------------------- the bounds
def slope_arg(X, inv_len, Q, family="ExpSquaredKernel", log_alpha=1.0):
    """(c2, A2[M, N]) of the module docstring: the rational quadratic's u / (1 + u) with d + 3 roundings; (0, None) otherwise."""
    if family != "RationalQuadraticKernel":
        return 0, None
    u = 0.5 * ksr._r2(ksr.scaled(Q, inv_len), ksr.scaled(X, inv_len), np.float64) / math.exp(log_alpha)
    return np.atleast_2d(X).shape[1] + 3, u / (1.0 + u)


def _weights(terms, A, family, d, E, A2=None):
    N = terms.shape[1]
    w = float(E + (N - 1)) + float(ksr.c_difference(d, family)) * np.asarray(A, dtype=np.float64)
    if A2 is not None:
        w = w + float(d + 3) * np.asarray(A2, dtype=np.float64)
    return w


def tiny_floor(X, alpha, amp, inv_len, Q):
    """2^-1074 * 2 sum_n P_mnc  [M, d] (module docstring)."""
    xs, qs = ksr.scaled(X, inv_len), ksr.scaled(Q, inv_len)
    df = np.maximum(1.0, np.abs(qs[:, None, :] - xs[None, :, :]))
    al = np.maximum(1.0, np.abs(np.asarray(alpha, dtype=np.float64)))
    P = max(1.0, 2.0 * float(amp)) * np.einsum("mnc,n->mc", df, al) * np.maximum(1.0, np.asarray(inv_len))[None, :]
    return TINY * 2.0 * P


def mean_gradient_tolerance(terms, A, family, d, A2=None, floor=0.0, E=None):
    """tol[M, d] of the module docstring.  terms[M, N, d] from ``mean_gradient``; A[M, N] = ``ksr.arg_difference``; A2 from
    ``slope_arg`` (rational quadratic); floor[M, d] = ``tiny_floor``; E: E_G[family] unless given."""
    t = np.abs(np.asarray(terms)).astype(np.float64)
    w = _weights(t, A, family, d, E_G[family] if E is None else E, A2)
    return U * np.einsum("mnc,mn->mc", t, w) + floor


def log_prob_gradient_tolerance(lpg, A, family, d, alpha, amp, folded_mean, A2=None, floor=0.0, ymap=None, affine=(1.0, 0.0)):
    """tol[M, d] of the module docstring.  ``lpg``: what ``log_prob_gradient`` returned; ``folded_mean`` = fma(a, mean, b)."""
    tol = mean_gradient_tolerance(lpg["gterms"], A, family, d, A2, abs(float(affine[0])) * floor, E=E_LP[family])
    if ymap is not None:
        ln10 = math.log(10.0)
        Lf = np.abs(np.asarray(lpg["L"]).astype(np.float64))
        Mf = np.abs(np.asarray(lpg["M_aff"]).astype(np.float64))
        dM = ksr.tolerance(lpg["vterms"], A, ksr.E_FAMILY[family] + 1, ksr.c_difference(d, family), alpha,
                           abs(float(affine[0])) * amp) + U * (Mf + abs(float(folded_mean)))
        dL = ln10 * Lf * dM + 2.0 * U * Lf
        dmu_a = np.abs(np.asarray(lpg["dmu_a"]).astype(np.float64))
        g = ln10 * Lf[:, None] * dmu_a
        tol = ln10 * Lf[:, None] * tol + ln10 * dmu_a * dL[:, None] + 3.0 * U * g
    pg = np.abs(np.asarray(lpg["prior_grad"]).astype(np.float64))
    if np.any(pg != 0.0):
        tol = tol + np.where(pg != 0.0, U * (5.0 * pg + np.abs(np.asarray(lpg["grad"]).astype(np.float64))), 0.0)
    return tol


def variance_gradient_bound(X, Q, amp, inv_len, L, ks, dks, family="ExpSquaredKernel", log_alpha=1.0, n0_append=None):
    """First-order bound B[M, d] of what the FORMULATION  v^ = W k*,  z^ = W^T v^,  dvar_c = -2 sum_n z^_n dk_nc  (W = L^-1 formed
    explicitly) may lose, from the true factor alone (no device output; magnitudes in fp64): the bilinear counterpart of
    ``derived_bound`` in tests/test_gpu_variance_truth.py.  With g_c = dk*/dx_c, a_c = K^-1 g_c, v = K^-1 k*, w = L^-1 k*:

      dvar_c = -2 g_c^T K^-1 k*.

      factor      the computed factor satisfies L^ L^T = K + dK with |dK| <= u G,
                  G_ij = (min(i, j) + 5) (|L||L^T|)_ij + |K_ij| (E + c A_ij)  (the count of ``derived_bound`` and of
                  solve_reference.factor_allowed: the right-looking Cholesky and the assembly of K).  To first order
                  d(g^T K^-1 k*) = -a_c^T dK v:                                  2 u |a_c|^T G |v|.
      K*          k*^_n = k*_n (1 + e_n), |e_n| <= u (E + c A_n):               2 u sum_n |a_cn| |k*_n| (E + c A_n).
      W = L^-1    the explicit inverse carries |dW| <= (N + 2) u |W||L||W| and enters twice, z^ = (W + dW)^T (W + dW) k*:
                    through W     2 (N + 2) u |W g_c|^T (|W||L||W|) |k*|
                    through W^T   2 (N + 2) u |g_c|^T (|W||L||W|)^T |w|
                  and each of the two products is a sum of up to N terms on the matrix cores (plus the combine of z's row parts):
                    2 N u ( |W g_c|^T |W| |k*|  +  |g_c|^T |W|^T |w| ).
      dk          dk^_nc = dk_nc (1 + e), |e| <= u (E_g + c A_n + c2 A2_n)  (module docstring; z takes alpha's place in the
                  count):                                                       2 u sum_n |v_n| |dk_nc| (E_g + c A_n + c2 A2_n).
      final sum   N - 1 additions in any order:                                 2 (N - 1) u sum_n |v_n| |dk_nc|.
    E, c: ksr.E_FAMILY and ksr.c_difference of the family.  ``n0_append``: the rows from n0 on were appended one at a time
    (gp_append.hip); u G is then solve_reference.append_bound (device counts, generic inverse), whose leading block is the above."""
    from scipy.linalg import solve_triangular
    N, d = np.atleast_2d(X).shape
    Lf = np.asarray(L, dtype=np.float64)
    ksf = np.abs(np.asarray(ks, dtype=np.float64))                           # [N, M]
    g = np.asarray(dks, dtype=np.float64)                                    # [M, N, d]
    M = g.shape[0]
    La = np.abs(Lf)
    Wm = solve_triangular(Lf, np.eye(N), lower=True)
    Wa = np.abs(Wm)
    w = np.abs(solve_triangular(Lf, np.asarray(ks, dtype=np.float64), lower=True))                   # [N, M]
    v = np.abs(solve_triangular(Lf.T, solve_triangular(Lf, np.asarray(ks, dtype=np.float64), lower=True), lower=False))
    E, c = ksr.E_FAMILY[family], ksr.c_difference(d, family)
    c2, A2 = slope_arg(X, inv_len, Q, family, log_alpha)
    AQ = ksr.arg_difference(X, inv_len, Q, family, log_alpha)                # [M, N]
    idx = np.minimum(np.arange(N)[:, None], np.arange(N)[None, :]) + 5.0
    G = idx * (La @ La.T) + np.abs(Lf @ Lf.T) * (E + c * ksr.arg_difference(X, inv_len, X, family, log_alpha))
    if n0_append is not None:
        G = sr.append_bound(X, inv_len, np.abs(Lf @ Lf.T), Lf, d, n0_append, "device", "generic", family, log_alpha) / U
    WLW = Wa @ La @ Wa
    B = np.zeros((M, d))
    for m in range(M):
        gm = g[m]                                                            # [N, d]
        Wg = np.abs(Wm @ gm)                                                 # |W g_c|  [N, d]
        a = np.abs(solve_triangular(Lf.T, Wm @ gm, lower=False))             # |K^-1 g_c|  [N, d]
        ga = np.abs(gm)
        vm, km, wm = v[:, m], ksf[:, m], w[:, m]
        b = 2.0 * a.T @ (G @ vm)
        b += 2.0 * a.T @ (km * (E + c * AQ[m]))
        b += 2.0 * (N + 2) * (Wg.T @ (WLW @ km) + ga.T @ (WLW.T @ wm))
        b += 2.0 * N * (Wg.T @ (Wa @ km) + ga.T @ (Wa.T @ wm))
        wt = E_G[family] + c * AQ[m] + (c2 * A2[m] if A2 is not None else 0.0) + (N - 1)
        b += 2.0 * ga.T @ (vm * wt)
        B[m] = b
    return U * B


def component_scale(z, dks):
    """S[M, d] = 2 sum_n |z_n dk_nc| with the true z[N, M]: the scale of a variance-gradient component before it cancels."""
    return 2.0 * np.einsum("nm,mnc->mc", np.abs(np.asarray(z).astype(np.float64)), np.abs(np.asarray(dks).astype(np.float64)))


# ----------------------------------------------------------------------------------- fp64 restatement of the device's formulation
def _sum_kernel_order(T):
    """Sum over axis 0 (the training points) in the order of pgrad_final_kernel: thread t adds the points t, t + 256, ... in turn,
    each wave of 64 lanes is reduced by a binary tree and the four wave totals are combined as (0 + 1) + (2 + 3)."""
    T = np.asarray(T, dtype=np.float64)
    n = T.shape[0]
    pad = (-n) % 256
    if pad:
        T = np.concatenate([T, np.zeros((pad,) + T.shape[1:])], axis=0)
    T = T.reshape((-1, 256) + T.shape[1:])
    acc = np.zeros(T.shape[1:])
    for r in range(T.shape[0]):
        acc = acc + T[r]
    wv = acc.reshape((4, 64) + acc.shape[1:])
    width = 64
    while width > 1:
        width //= 2
        wv = wv[:, :width] + wv[:, width:2 * width]
    wv = wv[:, 0]
    return (wv[0] + wv[1]) + (wv[2] + wv[3])


def slope_fp64(r2, family, log_alpha=1.0):
    """f'(r2) in fp64 as radial_and_slope writes it."""
    if family == "ExpSquaredKernel":
        return -0.5 * np.exp(-0.5 * r2)
    if family == "Matern32Kernel":
        return -1.5 * np.exp(-np.sqrt(3.0 * r2))
    if family == "Matern52Kernel":
        r = np.sqrt(5.0 * r2)
        return -(5.0 / 6.0) * (1.0 + r) * np.exp(-r)
    a = math.exp(log_alpha)
    u = 0.5 * r2 / a
    return -0.5 * np.exp(-a * np.log1p(u)) / (1.0 + u)


def value_fp64(r2, family, log_alpha=1.0):
    if family == "ExpSquaredKernel":
        return np.exp(-0.5 * r2)
    if family == "Matern32Kernel":
        r = np.sqrt(3.0 * r2)
        return (1.0 + r) * np.exp(-r)
    if family == "Matern52Kernel":
        r = np.sqrt(5.0 * r2)
        return (1.0 + r + r * r / 3.0) * np.exp(-r)
    a = math.exp(log_alpha)
    return np.exp(-a * np.log1p(0.5 * r2 / a))


def device_form_fp64(X, alpha, amp, inv_len, Q, W, family="ExpSquaredKernel", log_alpha=1.0, mutate=None):
    """(dmu[M, d], dvar[M, d]) by the device's formulation in plain fp64 NumPy: K* in the difference form, v = W k*, z = W^T v with
    the explicit inverse ``W`` of an fp64 factor, then one pass over the training points in pgrad_final_kernel's order of
    operations and of sums.  ``mutate`` plants a defect (tests/test_grad_reference_host.py):
      ("drop", m, n, c)   training point n's term left out of component c of query m (both gradients)
      ("slope", eps, sign[M, N])   f'(r2_mn) times (1 + eps sign_mn)
      ("inv_len", c)      coordinate c's final multiply takes its neighbour's inv_len
      ("stale_z",)        query m reads the z of query m - 1"""
    xs, qs = ksr.scaled(X, inv_len), ksr.scaled(Q, inv_len)
    M, N, d = qs.shape[0], xs.shape[0], xs.shape[1]
    kind = mutate[0] if mutate else None
    il = np.asarray(inv_len, dtype=np.float64).copy()
    if kind == "inv_len":
        c = mutate[1]
        il[c] = inv_len[c + 1] if c + 1 < d else inv_len[c - 1]
    dmu, dvar = np.empty((M, d)), np.empty((M, d))
    r2 = np.zeros((M, N))
    for k in range(d):
        df = qs[:, k][:, None] - xs[:, k][None, :]
        r2 = df * df + r2
    ks = amp * value_fp64(r2, family, log_alpha)                             # [M, N]
    z = (W.T @ (W @ ks.T)).T                                                 # [M, N]
    if kind == "stale_z":
        z = np.roll(z, 1, axis=0)
    fp = slope_fp64(r2, family, log_alpha)
    if kind == "slope":
        fp = fp * (1.0 + mutate[1] * mutate[2])
    gslope = (2.0 * amp) * fp
    ga = np.asarray(alpha, dtype=np.float64)[None, :] * gslope
    gz = z * gslope
    for m in range(M):
        df = qs[m][None, :] - xs                                             # [N, d]
        tm, tv = ga[m][:, None] * df, gz[m][:, None] * df
        if kind == "drop" and mutate[1] == m:
            tm[mutate[2], mutate[3]] = 0.0
            tv[mutate[2], mutate[3]] = 0.0
        dmu[m] = _sum_kernel_order(tm) * il
        dvar[m] = -2.0 * _sum_kernel_order(tv) * il
    return dmu, dvar


# ------------------------------------------------------------------------------------------------------- the shared case grid
M_QUERIES = 37
KINDS = ("box", "near", "outside", "on", "far")
# (N, d, log white noise, squared length scale of make_problem or None for its default, shift in length scales)
CASES = {"n1d1": (1, 1, -8.0, None, 0.0), "n64d2": (64, 2, -8.0, None, 0.0), "n65d3": (65, 3, -12.0, None, 0.0),
         "n130d10": (130, 10, -8.0, None, 0.0), "n200d17": (200, 17, -8.0, 4.0 * 17, 0.0), "n130d64": (130, 64, -8.0, 4.0 * 64, 0.0),
         "n130d10far": (130, 10, -8.0, None, 1000.0)}
LOG_ALPHA = {"ExpSquaredKernel": 1.0, "Matern32Kernel": 1.0, "Matern52Kernel": 1.0, "RationalQuadraticKernel": 0.4}
LP_CASES = ("n65d3", "n130d10", "n130d64")
# make_problem's seed is 700 + N + d unless listed here.  n65d3: with the default seed the weakest coordinate of dmu is 1.1e-3 to
# 2.1e-3 of the strongest over the four families; of the seeds 1 to 8 only 3 keeps all four below the 1e-3 the host test asserts
# (7.3e-4 to 9.3e-4).  NOTES.md ("Gradient truth") records the search.
SEEDS = {"n65d3": 3}
N_APPEND = 10


def case(name, make_problem):
    """The problem of a case: X, y, the hyper-parameters h (from d = 3 up with ln(squared length scale) ramped by
    linspace(0, ln 1e4, d): ARD), the M_QUERIES queries, their kinds, and the ten points the append path adds.
    ``shift`` moves training inputs, queries and appended points by that many length scales in every coordinate."""
    N, d, log_wn, ell2, shift = CASES[name]
    seed = SEEDS.get(name, 700 + N + d)
    with np.errstate(divide="ignore"):                   # one target has no variance: make_problem takes its logarithm
        X, y, h = make_problem(N, d, seed, log_wn=log_wn, **({} if ell2 is None else dict(ell2=ell2)))
    if N == 1:                                           # as solve_reference.case: the one target IS the median
        h = dict(h, mean=h["mean"] + 0.37, log_amp=0.0)
    if d >= 3:
        # ARD.  The targets are make_problem's function at the inputs scaled by the same ramp: a surrogate that interpolates
        # targets varying alike in every coordinate has gradients alike in every coordinate, whatever its length scales (with
        # make_problem's own y the weakest coordinate of dmu is 1.2e-2, 1.6e-2, 6.9e-3 and 6.0e-4 of the strongest at d = 3, 10,
        # 17 and 64: no weak coordinate at all up to d = 17).
        ramp = np.linspace(0.0, math.log(1e4), d)
        y = sr._target(X * np.exp(-ramp)[None, :], seed)
        h = dict(h, log_M=h["log_M"] + ramp, mean=float(np.median(y)), log_amp=float(np.log(np.var(y))))
    amp, wn, inv_len = ksr.hyper_fp64(h["log_amp"], h["log_white_noise"], h["log_M"])
    rng = np.random.RandomState(N + 7 * d)
    Mq = M_QUERIES
    kind = np.arange(Mq) % 5                                               # groups of 16, 16 and 5: every group holds each kind
    Q = rng.uniform(-3.0, 3.0, (Mq, d))
    j = rng.randint(0, N, Mq)
    near = X[j] + 1e-3 * rng.uniform(-1.0, 1.0, (Mq, d)) / inv_len[None, :] / np.sqrt(d)
    out = rng.uniform(3.0, 4.5, (Mq, d)) * rng.choice([-1.0, 1.0], (Mq, d))
    far = X[j].copy()
    far[:, 0] = X[:, 0].max() + 40.0 / inv_len[0]                           # r >= 40 from every training point
    Q[kind == 1] = near[kind == 1]
    Q[kind == 2] = out[kind == 2]
    Q[kind == 3] = X[j][kind == 3]
    Q[kind == 4] = far[kind == 4]
    Xadd = np.random.RandomState(N).uniform(-3.0, 3.0, (N_APPEND, d))
    off = shift / inv_len
    return dict(name=name, N=N, d=d, X=X + off, y=y, h=h, Q=Q + off, kind=kind, Xadd=Xadd + off, off=off,
                amp=amp, wn=wn, inv_len=inv_len)


def append_sets(c):
    """(X0, Xa, ya) of the append path: the factor of X0 is extended point by point to Xa.  A chain may not start on a multiple
    of 64 rows (the first step would refactorise), so the N = 64 case is REACHED by ten appends from 54 points; every other case
    grows from N to N + 10."""
    if c["N"] % 64 == 0:
        return c["X"][:c["N"] - N_APPEND], c["X"], c["y"]
    return c["X"], np.vstack([c["X"], c["Xadd"]]), np.concatenate([c["y"], np.zeros(N_APPEND)])


def oracle_gradients(X, y, Q, h, family):
    """(dmu, dvar) of oracle.utility_oracle.analytic_predict_grad in the input convention of the truth: the oracle GP is built on
    the scaled coordinates fl(x * inv_len) with unit length scales and its gradients, taken with respect to the scaled query, are
    multiplied by inv_len (the one rounding the bound charges for that step).  On raw coordinates the oracle forms q - x before
    it scales, which differs from fl(q inv_len) - fl(x inv_len) by up to u (|s_q| + |s_x|): a difference of INPUTS of some
    1000 u relative where a query sits 1e-3 length scales from a training point, or 1000 length scales from the origin."""
    from oracle.gp_oracle import OracleGP
    from oracle.utility_oracle import analytic_predict_grad
    inv_len = ksr.hyper_fp64(h["log_amp"], h["log_white_noise"], h["log_M"])[2]
    d = np.atleast_2d(X).shape[1]
    o = OracleGP(d, h["mean"], h["log_white_noise"], h["log_amp"], np.zeros(d), kernel=family, log_alpha=LOG_ALPHA[family])
    o.compute(ksr.scaled(X, inv_len))
    _, _, dmu, dvar = analytic_predict_grad(o, y, ksr.scaled(Q, inv_len))
    return dmu * inv_len[None, :], dvar * inv_len[None, :], np.asarray(o._compute_alpha(y), dtype=np.float64)


def truth(X, Q, h, family, with_bound=True, n0_append=None):
    """Everything that does not depend on alpha, once: dks[M, N, d], the true factor, z, the variance gradient with its terms,
    the bound B (``n0_append``: for a factor whose rows from n0 on were appended) and the scale S, the argument magnitudes.  Queries beyond ksr.QUERY_STRIDE are left out (``keep``)."""
    la = LOG_ALPHA[family]
    amp, wn, inv_len = ksr.hyper_fp64(h["log_amp"], h["log_white_noise"], h["log_M"])
    keep = np.arange(0, len(Q), ksr.QUERY_STRIDE)
    Qk = Q[keep]
    dks = kernel_gradient(X, amp, inv_len, Qk, family, la)
    K = ksr.kernel_matrix(X, amp, wn, inv_len, family, la)
    L = ksr.cholesky(K)
    ks = ksr.cross_matrix(X, amp, inv_len, Qk, family, la)
    if L.dtype == object:
        import mpmath as mp
        with mp.workdps(ksr.MP_DIGITS):
            z = _to_ld(solve_z(L, ks))
        L, K, ks = _to_ld(L), _to_ld(K), _to_ld(ks)
    else:
        z = solve_z(L, ks)
    dvar, vterms = variance_gradient(L, X, amp, inv_len, Qk, family, la, dks=dks, z=z)
    c2, A2 = slope_arg(X, inv_len, Qk, family, la)
    out = dict(keep=keep, dks=dks, K=K, L=L, ks=ks, z=z, dvar=dvar, S=component_scale(z, dks), A=ksr.arg_difference(X, inv_len, Qk, family, la),
               A2=A2, amp=amp, wn=wn, inv_len=inv_len, log_alpha=la)
    if with_bound:
        out["B"] = variance_gradient_bound(X, Qk, amp, inv_len, L, ks, dks, family, la, n0_append)
    return out


def mean_truth(t, X, Q, alpha, family):
    """(dmu truth [M, d] in long double, tolerance [M, d]) for one alpha from a cached ``truth``."""
    ref, terms = mean_gradient(X, alpha, t["amp"], t["inv_len"], Q[t["keep"]], family, t["log_alpha"], dks=t["dks"])
    floor = tiny_floor(X, alpha, t["amp"], t["inv_len"], Q[t["keep"]])
    return ref, mean_gradient_tolerance(terms, t["A"], family, X.shape[1], t["A2"], floor)


def yardstick(dvar, dvar_oracle, t, rows=None, centre=None):
    """The rule every variance gradient is held to, in one place: (e_ref[d], e[d], allowed[d], err / B [rows, d]).
    ``dvar`` and ``dvar_oracle`` are [len(rows), d], aligned with the rows ``rows`` of the truth ``t`` (default: all of them).
    e_ref: per coordinate the oracle's largest distance from the truth over those queries; e: that of ``dvar`` from ``centre``
    (default the truth; the attribution passes the gradient a given factor yields); allowed = 10 e_ref + 64 u S_c with S_c the
    largest scale 2 sum_n |z_n dk_nc| over those queries; err / B: the distance from ``centre`` over the derived bound, per
    component."""
    rows = np.arange(len(t["dvar"])) if rows is None else np.asarray(rows)
    ref = t["dvar"][rows]
    mid = ref if centre is None else np.asarray(centre, dtype=LD)
    err = np.abs((np.asarray(dvar).astype(LD) - mid).astype(np.float64))
    e_ref = np.max(np.abs((np.asarray(dvar_oracle).astype(LD) - ref).astype(np.float64)), axis=0)
    allowed = 10.0 * e_ref + 64.0 * U * np.max(t["S"][rows], axis=0)
    B = t["B"][rows]
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(B > 0, err / B, np.where(err > 0, np.inf, 0.0))
    return e_ref, np.max(err, axis=0), allowed, frac


# ----------------------------------------------------------------------------------------- the log-probability's settings
AFFINE = (2.5, -3.0)
LP_SETTINGS = ("identity", "affine", "nlog", "log", "prior")


def lp_settings(c, setting):
    """(EnsembleSampler keywords, log_prob_gradient keywords) of a named setting on a case."""
    d = c["d"]
    if setting == "affine":
        return dict(logp_affine=AFFINE), dict(affine=AFFINE)
    if setting in ("nlog", "log"):
        return dict(logp_map=setting), dict(ymap=setting)
    if setting == "prior":
        pm, ps = np.full(d, np.nan), np.full(d, np.nan)
        for i, k in enumerate(sorted({0, min(2, d - 1), d - 1})):           # the first lanes and the last one
            pm[k], ps[k] = c["off"][k] + (0.4, -0.8, 0.3)[i], (0.7, 1.3, 0.9)[i]
        return dict(normal_prior=(pm, ps)), dict(prior=(pm, ps))
    return {}, {}


def lp_truth(t, X, Q, alpha, mean, family, ex):
    """(log_prob_gradient's dict, tolerance[M, d]) of a setting ``ex`` (lp_settings' second dict) from a cached ``truth``."""
    affine = ex.get("affine", (1.0, 0.0))
    Qk = Q[t["keep"]]
    lpg = log_prob_gradient(X, alpha, t["amp"], t["inv_len"], Qk, mean, family, t["log_alpha"], affine=affine, ymap=ex.get("ymap"),
                            prior=ex.get("prior"), dks=t["dks"])
    floor = tiny_floor(X, alpha, t["amp"], t["inv_len"], Qk)
    tol = log_prob_gradient_tolerance(lpg, t["A"], family, X.shape[1], alpha, t["amp"], affine[0] * mean + affine[1], t["A2"], floor,
                                      ymap=ex.get("ymap"), affine=affine)
    return lpg, tol


def log_prob_grad_fp64(X, alpha, amp, inv_len, Q, mean, family="ExpSquaredKernel", log_alpha=1.0, affine=(1.0, 0.0), ymap=None,
                       prior=None, mutate=None):
    """(lp[M], grad[M, d]) by lp_grad_eval's formulation in plain fp64 NumPy, no box gate: the weights w_n = -2 alpha_n f'(r2_n),
    s_k = sum_n w_n (x_nk - q_k) with the difference formed per point, g_k = fl(a amp) inv_len_k s_k, the value through
    fma(a amp, sum, a mean + b), the y map, the normal priors with is = fl(1 / s).  ``mutate`` plants a defect:
      ("slope", eps, sign[M, N])   f'(r2_mn) times (1 + eps sign_mn)
      ("no_fold",)                 the gradient multiplied by amp where the value takes a amp
      ("stale_L",)                 the y map's factor L of query m - 1 in the gradient of query m
      ("prior_swap",)              a prior coordinate's term formed with the prior mean of the next prior coordinate"""
    xs, qs = ksr.scaled(X, inv_len), ksr.scaled(Q, inv_len)
    kind = mutate[0] if mutate else None
    a, b = float(affine[0]), float(affine[1])
    ampf, meanf = a * amp, a * mean + b
    r2 = np.zeros((qs.shape[0], xs.shape[0]))
    for k in range(xs.shape[1]):
        df = xs[:, k][None, :] - qs[:, k][:, None]
        r2 = df * df + r2
    al = np.asarray(alpha, dtype=np.float64)
    fp = slope_fp64(r2, family, log_alpha)
    if kind == "slope":
        fp = fp * (1.0 + mutate[1] * mutate[2])
    w = (-2.0 * al)[None, :] * fp
    mu = ampf * np.sum(value_fp64(r2, family, log_alpha) * al[None, :], axis=1) + meanf
    s = np.stack([np.sum(w * (xs[:, k][None, :] - qs[:, k][:, None]), axis=1) for k in range(xs.shape[1])], axis=1)
    g = ((amp if kind == "no_fold" else ampf) * np.asarray(inv_len, dtype=np.float64))[None, :] * s
    lp = mu
    if ymap is not None:
        lp = (-1.0 if ymap == "nlog" else 1.0) * 10.0 ** mu
        g = 2.302585092994046 * (np.roll(lp, 1) if kind == "stale_L" else lp)[:, None] * g
    if prior is not None:
        pm, ps = (np.asarray(v, dtype=np.float64) for v in prior)
        ks = np.nonzero(np.isfinite(pm) & np.isfinite(ps) & (ps > 0))[0]
        q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
        for i, k in enumerate(ks):
            is_ = 1.0 / ps[k]
            m_k = pm[ks[(i + 1) % len(ks)]] if kind == "prior_swap" else pm[k]
            tt = (q[:, k] - pm[k]) * is_
            lp = lp + (-0.5 * tt * tt - np.log(ps[k]) - 0.9189385332046727)
            g[:, k] = g[:, k] - (q[:, k] - m_k) * is_ * is_
    return lp, g
