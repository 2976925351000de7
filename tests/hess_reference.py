"""Extended-precision truth for the Hessian of the ensemble's fused log-probability with respect to the query point
(``EnsembleSampler.log_prob_hessian``: ens_lp_hess_kernel / lp_hess_eval, alabi_amd/csrc/ens_map.hip and ens_hess_device.hpp), with
the bound the kernel is held to (tests/test_hess_reference_host.py, tests/test_gpu_hess_truth.py).  Plain NumPy in ``ksr.LD``
(mpmath where ``np.longdouble`` is only a double); no GPU, nothing imported from alabi_amd.  It extends tests/grad_reference.py
(``gr``), which it imports and does not edit, and keeps its input convention: the hyper-parameters of ``ksr.hyper_fp64``, the scaled
coordinates ``fl(x * inv_len)`` and the device's own fp64 alpha are the inputs; everything after that runs in extended precision.

With s = scaled coordinates, dl = s_q - s_n, r2 = |dl|^2 and f the radial profile (k = amp f(r2)):

    d2 mu / dx_a dx_b = amp inv_a inv_b sum_n alpha_n [4 f''(r2_n) dl_na dl_nb + 2 f'(r2_n) 1(a = b)]       (``mean_hessian``)
    f''(r2): f / 4 (squared exponential), (9/4) e^-s / s with s = sqrt(3 r2) (Matern-3/2; the whole dl dl term is 0 at r2 = 0, to
             which it tends), (25/12) e^-s with s = sqrt(5 r2) (Matern-5/2), (a + 1) / (4 a) (1 + u)^(-a - 2) with u = r2 / (2 a)
             (rational quadratic)                                                                          (``radial_curvature``)

Through the maps (``log_prob_hessian``), with Mu = a mu + b:  identity H = a d2mu;  y map L = -+10^Mu: H = ln10 L a d2mu +
ln10^2 L (a dmu)(a dmu)^T;  a normal prior on coordinate k subtracts 1 / s_k^2 on the diagonal.


The mean Hessian's bound (``mean_hessian_tolerance``), u = 2^-53, per query m and entry (a, b)
------------------------------------------------------------------------------------------------

    tol_mab = u sum_n |T2_mnab| (E_h2 + (N - 1) + c A_mn + 2 c2 A2_mn)
            + 1(a = b) u sum_n |T1_mna| (E_h1 + (N - 1) + c A_mn + c2 A2_mn)  +  2^-1074 * 4 sum_n P_mnab

  T2, T1        the two parts of a term: T2 = alpha amp inv_a inv_b 4 f'' dl_a dl_b, T1 = alpha amp inv_a^2 2 f'.  On the diagonal the
                kernel adds them per point before it sums; |T2| and |T1| are charged separately, which bounds the same roundings.
  N - 1, c, A   as in ksr and gr: the additions of the sum in any order and the c roundings of the exponential's argument.
  c2 A2         rational quadratic only, as in gr: f'' carries (1 + u)^(-a - 2), so beyond c A the sensitivity to u is
                2 u / (1 + u) = 2 A2 (f': A2), each charged the c2 = d + 3 roundings of u.
  E_h2          relative roundings of a T2 term outside the exponential's argument, counted in lp_hess_eval and
                ens_lp_hess_kernel rounding by rounding:
                  the exponential          gr.E_EXP: 4 for exp_neg_half, 2 for the library exp
                  f'' from it              squared exponential 0 (0.25 * f is exact); Matern-3/2 2 + c (2.25 * e, the divide by r,
                                           and r's own relative error, at most c u, which 1 / r passes on once more on top of what
                                           c A charges for e^-r); Matern-5/2 2 (the constant 25/12 and the multiply); rational
                                           quadratic 7 (1 + u, which enters squared: 2; its square; a + 1; the divide by 4 a, 4 a
                                           being exact; times f; the divide)
                  u2 = 4 alpha f''         1 (4 alpha is exact)
                  dl_a, dl_b               2
                  (u2 dl_a) dl_b           2
                  t += u1 (diagonal)       1 (charged to every entry)
                  s += t                   1 (on top of N - 1, as ksr charges the final addition; one wave sums an item, so there
                                           is no combine of partials)
                  inv_a inv_b, amp * that, times the sum    3
                  the fold fl(lp_scale amp) of the launcher  1
                E_h2 = exponential + f'' + 11.
  E_h1          of a T1 term: the exponential, gr.E_SLOPE_POLY, u1 = 2 alpha f' (1), t += u1 (1), s += t (1), the same 4 at the
                end: exponential + slope + 7.
  2^-1074 ...   as in gr: a value in the denormal range is rounded absolutely; f'', u2, the two products and the sums (at most
                2^-1075 each, eight places, hence the 4), multiplied afterwards by at most P = max(1, 4 amp) max(1, |alpha|)
                max(1, |dl_a|) max(1, |dl_b|) max(1, inv_a inv_b).

The log-probability's Hessian (the tolerance ``log_prob_hessian`` returns with the truth):

    identity   tol = mean_hessian_tolerance of the terms scaled by |a|
    y map      H = ln10 L Hm + ln10^2 L ga gb  (Hm = a d2mu, g = a dmu):
                 tol = ln10 |L| tol_Hm + ln10 |Hm| dL + 3 u |ln10 L Hm|
                     + ln10^2 [|L| (|ga| dg_b + |gb| dg_a) + |ga gb| dL] + 6 u |ln10^2 L ga gb|  +  u |H|
               dL and dg as gr.log_prob_gradient_tolerance has them (dg with E = gr.E_LP: lp_hess_eval's gradient sum has
               lp_grad_eval's count: dl (1), u1 (1), fma (1), amp * inv (1), times the sum (1), the fold (1)); 3: the constant,
               times L, times Hm; 6: the constant ln10's own rounding, which enters twice, ln10 * ln10, times L, ga * gb, the last
               multiply; u |H|: the final addition.
    prior      H_aa -= is * is with is = fl(1 / s):  tol += u (3 / s^2 + |H_aa|): the reciprocal's rounding, which enters twice,
               the multiply, and the subtraction.

No constant here is fitted to device output; tests/test_hess_reference_host.py shows that an honest fp64 restatement lies inside
the bound and that planted defects lie outside.
"""
from __future__ import annotations

import math

import numpy as np

import grad_reference as gr
import kernel_sum_reference as ksr

LD = ksr.LD
U, TINY = ksr.U, ksr.TINY

E_CURV_POLY = {"ExpSquaredKernel": 0, "Matern32Kernel": 2, "Matern52Kernel": 2, "RationalQuadraticKernel": 7}


def e_h2(family, d):
    own = ksr.c_difference(d, family) if family == "Matern32Kernel" else 0
    return gr.E_EXP[family] + E_CURV_POLY[family] + own + 11


def e_h1(family):
    return gr.E_EXP[family] + gr.E_SLOPE_POLY[family] + 7


# ------------------------------------------------------------------------------------------------------------ the curvature
def radial_curvature(r2, family, log_alpha=1.0):
    """f''(r2) in the precision of r2 (np.longdouble arrays, or object arrays of mpf inside an mp.workdps block); Matern-3/2
    returns 0 at r2 = 0, where the term it multiplies is defined as 0."""
    r2 = np.asarray(r2)
    if r2.dtype == object:
        import mpmath as mp
        a = mp.mpf(math.exp(log_alpha))

        def one(v):
            if family == "ExpSquaredKernel":
                return mp.exp(-v / 2) / 4
            if family == "Matern32Kernel":
                s = mp.sqrt(3 * v)
                return mp.mpf(9) / 4 * mp.exp(-s) / s if v > 0 else mp.mpf(0)
            if family == "Matern52Kernel":
                return mp.mpf(25) / 12 * mp.exp(-mp.sqrt(5 * v))
            if family == "RationalQuadraticKernel":
                return (a + 1) / (4 * a) * mp.exp(-(a + 2) * mp.log1p(v / (2 * a)))
            raise ValueError(family)
        return np.array([one(v) for v in r2.ravel()], dtype=object).reshape(r2.shape)
    r2 = r2.astype(LD)
    if family == "ExpSquaredKernel":
        return np.exp(-r2 / LD(2)) / LD(4)
    if family == "Matern32Kernel":
        s = np.sqrt(LD(3) * r2)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(r2 > 0, LD(9) / LD(4) * np.exp(-s) / np.where(r2 > 0, s, LD(1)), LD(0))
    if family == "Matern52Kernel":
        return LD(25) / LD(12) * np.exp(-np.sqrt(LD(5) * r2))
    if family == "RationalQuadraticKernel":
        a = LD(math.exp(log_alpha))
        return (a + LD(1)) / (LD(4) * a) * np.exp(-(a + LD(2)) * np.log1p(r2 / (LD(2) * a)))
    raise ValueError(family)


def _differences(X, inv_len, q):
    """dl[N, d] = s_q - s_n of ONE query in extended precision, and whether it is an object array of mpf."""
    xs, qs = ksr.scaled(X, inv_len), ksr.scaled(q, inv_len)[0]
    if ksr.EXTENDED:
        return qs.astype(LD)[None, :] - xs.astype(LD), False
    return gr._mp_array(qs)[None, :] - gr._mp_array(xs), True


def mean_hessian(X, alpha, amp, inv_len, Q, family="ExpSquaredKernel", log_alpha=1.0):
    """A list with one dict per query:
      H [d, d]          d2 mu / dx_a dx_b in np.longdouble
      T2 [N, d, d]      |alpha_n amp inv_a inv_b 4 f''(r2_n) dl_na dl_nb|   (fp64 magnitudes: what the bound reads)
      T1 [N, d]         |alpha_n amp inv_a^2 2 f'(r2_n)|
    Query by query: a [N, d, d] array of long doubles at d = 64 is 8.5 MB."""
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
    inv = np.asarray(inv_len, dtype=np.float64)
    al = np.asarray(alpha, dtype=np.float64)
    out = []
    for q in Q:
        dl, is_mp = _differences(X, inv_len, q[None, :])
        if is_mp:
            import mpmath as mp
            with mp.workdps(ksr.MP_DIGITS):
                r2 = (dl * dl).sum(axis=1)
                c2 = 4 * mp.mpf(float(amp)) * gr._mp_array(al) * radial_curvature(r2, family, log_alpha)
                c1 = 2 * mp.mpf(float(amp)) * gr._mp_array(al) * gr.radial_slope(r2, family, log_alpha)
                iv = gr._mp_array(inv)
                T2 = gr._to_ld(c2[:, None, None] * dl[:, :, None] * dl[:, None, :] * iv[None, :, None] * iv[None, None, :])
                T1 = gr._to_ld(c1[:, None] * (iv * iv)[None, :])
        else:
            r2 = (dl * dl).sum(axis=1)
            c2 = LD(4) * LD(amp) * al.astype(LD) * radial_curvature(r2, family, log_alpha)
            c1 = LD(2) * LD(amp) * al.astype(LD) * gr.radial_slope(r2, family, log_alpha)
            iv = inv.astype(LD)
            T2 = c2[:, None, None] * dl[:, :, None] * dl[:, None, :] * iv[None, :, None] * iv[None, None, :]
            T1 = c1[:, None] * (iv * iv)[None, :]
        H = T2.sum(axis=0)
        H[np.diag_indices(len(inv))] += T1.sum(axis=0)
        out.append(dict(H=H, T2=np.abs(T2).astype(np.float64), T1=np.abs(T1).astype(np.float64)))
    return out


def hessian_floor(X, alpha, amp, inv_len, q):
    """2^-1074 * 4 sum_n P_nab  [d, d] of one query (module docstring)."""
    xs, qs = ksr.scaled(X, inv_len), ksr.scaled(q, inv_len)[0]
    df = np.maximum(1.0, np.abs(qs[None, :] - xs))
    al = np.maximum(1.0, np.abs(np.asarray(alpha, dtype=np.float64)))
    inv = np.asarray(inv_len, dtype=np.float64)
    P = max(1.0, 4.0 * float(amp)) * np.einsum("n,na,nb->ab", al, df, df) * np.maximum(1.0, inv[:, None] * inv[None, :])
    return TINY * 4.0 * P


def mean_hessian_tolerance(mh, A, family, d, A2=None, floor=0.0):
    """tol[d, d] of ONE query: ``mh`` an entry of ``mean_hessian``'s list, A[N] and A2[N] the query's rows of
    ``ksr.arg_difference`` and ``gr.slope_arg``."""
    N = mh["T2"].shape[0]
    c = float(ksr.c_difference(d, family))
    A = np.asarray(A, dtype=np.float64)
    w2 = float(e_h2(family, d) + N - 1) + c * A
    w1 = float(e_h1(family) + N - 1) + c * A
    if A2 is not None:
        w2 = w2 + 2.0 * float(d + 3) * np.asarray(A2, dtype=np.float64)
        w1 = w1 + float(d + 3) * np.asarray(A2, dtype=np.float64)
    tol = U * np.einsum("nab,n->ab", mh["T2"], w2)
    tol[np.diag_indices(d)] += U * np.einsum("na,n->a", mh["T1"], w1)
    return tol + floor


# ----------------------------------------------------------------------------------------------------- the log-probability
def log_prob_hessian(X, alpha, amp, inv_len, Q, mean, family="ExpSquaredKernel", log_alpha=1.0, affine=(1.0, 0.0), ymap=None,
                     prior=None, with_tolerance=True):
    """(H[M, d, d] in np.longdouble, tol[M, d, d] or None) of the fused log-probability WITHOUT the box gate, by the chain rule
    in extended precision.  ``mean``: the GP's constant mean; ``affine`` = (lp_scale, lp_shift); ``ymap`` None / "nlog" / "log";
    ``prior`` = (mean[d], std[d]) with NaN where there is none."""
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
    M, d = Q.shape
    a = LD(float(affine[0]))
    aa = abs(float(affine[0]))
    mhs = mean_hessian(X, alpha, amp, inv_len, Q, family, log_alpha)
    lpg = gr.log_prob_gradient(X, alpha, amp, inv_len, Q, mean, family, log_alpha, affine=affine, ymap=ymap, prior=None)
    H = np.empty((M, d, d), dtype=LD)
    tol = np.empty((M, d, d)) if with_tolerance else None
    if with_tolerance:
        A = ksr.arg_difference(X, inv_len, Q, family, log_alpha)
        _, A2 = gr.slope_arg(X, inv_len, Q, family, log_alpha)
        folded_mean = float(affine[0]) * float(mean) + float(affine[1])
        if ymap is not None:
            dg = gr.mean_gradient_tolerance(lpg["gterms"], A, family, d, A2, aa * gr.tiny_floor(X, alpha, amp, inv_len, Q),
                                            E=gr.E_LP[family])
            Lf = np.abs(np.asarray(lpg["L"]).astype(np.float64))
            Mf = np.abs(np.asarray(lpg["M_aff"]).astype(np.float64))
            dM = ksr.tolerance(lpg["vterms"], A, ksr.E_FAMILY[family] + 1, ksr.c_difference(d, family), alpha, aa * amp) + \
                U * (Mf + abs(folded_mean))
            dL = math.log(10.0) * Lf * dM + 2.0 * U * Lf
    ln10 = LD(gr.LN10_STR)
    l10 = math.log(10.0)
    for m in range(M):
        Hm = a * mhs[m]["H"]
        Hq = Hm
        if ymap is not None:
            g = lpg["dmu_a"][m]
            Lm = lpg["L"][m]
            Hq = ln10 * Lm * Hm + ln10 * ln10 * Lm * g[:, None] * g[None, :]
        if with_tolerance:
            t = aa * mean_hessian_tolerance(mhs[m], A[m], family, d, None if A2 is None else A2[m],
                                            hessian_floor(X, alpha, amp, inv_len, Q[m:m + 1]))
            if ymap is not None:
                Hmf, gf = np.abs(Hm.astype(np.float64)), np.abs(g.astype(np.float64))
                first = l10 * Lf[m] * Hmf
                second = l10 * l10 * Lf[m] * gf[:, None] * gf[None, :]
                t = (l10 * Lf[m] * t + l10 * Hmf * dL[m] + 3.0 * U * first +
                     l10 * l10 * (Lf[m] * (gf[:, None] * dg[m][None, :] + gf[None, :] * dg[m][:, None]) + gf[:, None] * gf[None, :] * dL[m]) +
                     6.0 * U * second + U * np.abs(Hq.astype(np.float64)))
        if prior is not None:
            pm, ps = (np.asarray(v, dtype=np.float64) for v in prior)
            Hq = Hq.copy()
            for k in np.nonzero(np.isfinite(pm) & np.isfinite(ps) & (ps > 0))[0]:
                p = LD(1) / (LD(ps[k]) * LD(ps[k]))
                Hq[k, k] = Hq[k, k] - p
                if with_tolerance:
                    t[k, k] += U * (3.0 * float(p) + abs(float(Hq[k, k])))
        H[m] = Hq
        if with_tolerance:
            tol[m] = t
    return H, tol


# ------------------------------------------------------------------------------------- fp64 restatement (the host test)
def curvature_fp64(r2, family, log_alpha=1.0):
    """f''(r2) in fp64 as radial_value_slope_curv writes it."""
    if family == "ExpSquaredKernel":
        return 0.25 * np.exp(-0.5 * r2)
    if family == "Matern32Kernel":
        r = np.sqrt(3.0 * r2)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(r2 > 0.0, 2.25 * np.exp(-r) / np.where(r2 > 0.0, r, 1.0), 0.0)
    if family == "Matern52Kernel":
        return (25.0 / 12.0) * np.exp(-np.sqrt(5.0 * r2))
    a = math.exp(log_alpha)
    opu = 1.0 + 0.5 * r2 / a
    return (a + 1.0) / (4.0 * a) * np.exp(-a * np.log1p(0.5 * r2 / a)) / (opu * opu)


def log_prob_hessian_fp64(X, alpha, amp, inv_len, Q, mean, family="ExpSquaredKernel", log_alpha=1.0, affine=(1.0, 0.0), ymap=None,
                          prior=None, mutate=None):
    """H[M, d, d] by ens_lp_hess_kernel's formulation in plain fp64 NumPy, no box gate.  ``mutate`` plants a defect:
    "no_diag" drops the 2 f' 1(a = b) term, "wrong_family" takes the squared exponential's f'' = f / 4 whatever the family (for the
    squared exponential: Matern-5/2's), "no_outer" drops the dMu dMu^T term of a y map."""
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
    M, d = Q.shape
    inv = np.asarray(inv_len, dtype=np.float64)
    xs, qs = ksr.scaled(X, inv_len), ksr.scaled(Q, inv_len)
    al = np.asarray(alpha, dtype=np.float64)
    a_fold = float(affine[0]) * float(amp)
    m_fold = float(affine[0]) * float(mean) + float(affine[1])
    H = np.empty((M, d, d))
    cf = family
    if mutate == "wrong_family":
        cf = "Matern52Kernel" if family == "ExpSquaredKernel" else "ExpSquaredKernel"
    for m in range(M):
        dl = qs[m][None, :] - xs
        r2 = np.sum(dl * dl, axis=1)
        f = gr.value_fp64(r2, family, log_alpha)
        fp = gr.slope_fp64(r2, family, log_alpha)
        fpp = curvature_fp64(r2, cf, log_alpha)
        u1, u2 = 2.0 * al * fp, 4.0 * al * fpp
        S = np.einsum("n,na,nb->ab", u2, dl, dl)
        if mutate != "no_diag":
            S[np.diag_indices(d)] += np.sum(u1)
        G = dl.T @ u1
        h = a_fold * (inv[:, None] * inv[None, :]) * S
        if ymap is not None:
            Mu = a_fold * float(np.sum(al * f)) + m_fold
            L = (-1.0 if ymap == "nlog" else 1.0) * 10.0 ** Mu
            g = a_fold * inv * G
            h = math.log(10.0) * L * h
            if mutate != "no_outer":
                h = h + math.log(10.0) ** 2 * L * g[:, None] * g[None, :]
        if prior is not None:
            pm, ps = (np.asarray(v, dtype=np.float64) for v in prior)
            for k in np.nonzero(np.isfinite(pm) & np.isfinite(ps) & (ps > 0))[0]:
                h[k, k] -= (1.0 / ps[k]) ** 2
        H[m] = h
    return H


# ------------------------------------------------------------------------------------------ problems of moves_shapes_common
def problem_inputs(prob, alpha=None):
    """(X, alpha, amp, inv_len, mean, family, log_alpha) of a problem of tests/moves_shapes_common.py; ``alpha``: the device's own,
    else the oracle's."""
    h = prob.h
    amp, _, inv_len = ksr.hyper_fp64(h["log_amp"], h["log_white_noise"], h["log_M"])
    if alpha is None:
        alpha = np.asarray(prob.oracle._compute_alpha(prob.y), dtype=np.float64)
    return prob.X, np.asarray(alpha, dtype=np.float64), amp, inv_len, h["mean"], prob.kernel_name, prob.log_alpha


def problem_hessian(prob, ex, Q, alpha=None, with_tolerance=False):
    """The truth Hessian [M, d, d] (fp64 values of the long doubles) of a problem under the extras of hmc_cases (affine, ymap,
    prior); with ``with_tolerance`` the pair (H in long double, tol)."""
    X, al, amp, inv_len, mean, family, la = problem_inputs(prob, alpha)
    H, tol = log_prob_hessian(X, al, amp, inv_len, Q, mean, family, la, affine=ex.get("affine", (1.0, 0.0)), ymap=ex.get("ymap"),
                              prior=ex.get("prior"), with_tolerance=with_tolerance)
    return (H, tol) if with_tolerance else H.astype(np.float64)
