"""Extended-precision truth and yardsticks for the hyper-parameter gradient of the log marginal likelihood,
alabi_gp_grad_log_likelihood (csrc/gp_grad.hip: grad_contract_kernel, grad_final_kernel, radial_with_derivative), used by
tests/test_hyper_grad_reference_host.py and tests/test_gpu_hyper_grad_truth.py.  Plain NumPy plus kernel_sum_reference (ksr)
and solve_reference (sr); no GPU, nothing imported from alabi_amd.

With A = alpha alpha^T - K^-1 the gradient is  g_p = 0.5 sum_ij A_ij T^p_ij,  T^p = dK/dp, in the C ABI's order
(``entry_names``): mean, log_wn, log_amp, log_alpha, log_M_0 ...

    mean        sum_i alpha_i
    log_wn      T = wn I
    log_amp     T = amp f(r2)                                  (= K - wn I, the diagonal included)
    log_alpha   T = amp a f (q - l),  q = v / (1 + v), l = log1p(v), v = r2 / (2 a)      (rational quadratic only, else 0)
    log_M_k     T = -amp f'(r2) D_k^2,  D_k the difference of the scaled coordinates

It is a difference of two large, nearly equal parts, so no error of it is measured against |g|.  The scale of entry p is
    S_p = 0.5 sum_ij (|alpha_i alpha_j| + |K^-1_ij|) |T^p_ij|          (mean: sum_i |alpha_i|),
which ``truth`` returns beside g.  u = 2^-53.  Every bound below is a count of roundings of honest fp64 arithmetic or a distance
from the truth; no constant is fitted to device output.  All counts are to first order in u.

Truth (``truth``)
    From the library's own fp64 inputs (ksr.hyper_fp64, ksr.scaled) in the precision of ksr.kernel_matrix (long double; mpmath
    at ksr.MP_DIGITS where long double is a double, or on request): K, its factor L, alpha = L^-T L^-1 (y - mean), W = L^-1 by
    substitution, K^-1 = W^T W, then the contraction above.

Contraction given its inputs (``contract_given`` with ``given_bound``)
    The same contraction in extended precision from ANY fp64 alpha and K^-1 (the device's own: solver.get_inverse() runs the
    kinv_block that grad_contract_kernel consumes), so what is left is gp_grad.hip's own arithmetic.  Per element, with
    a_ij = |alpha_i alpha_j| + |K^-1_ij| >= |A_ij|:
      A        the product and the subtraction (or one fused operation): 2 u a_ij.
      r2       D_k = x_ik - x_jk (u), its square (3 u together), d - 1 additions: (d + 2) u r2, ksr's count c for the difference
               form; ksr.c_difference turns it into the count c of the family's exponential argument Arg (ksr.arg_difference),
               and every one of f, f', the log_alpha factor moves by at most c Arg u of itself when its argument does (|d ln f /
               d ln arg| <= arg for all four families; for q - l see below).
      f, f'    E_f, E_f' roundings outside the argument, ksr's convention (twice the exponential's ulp figure rounded up, one
               per further operation):
                 squared exponential    f = exp_neg_half (1.23 ulp: 4),  f' = -f / 2 exact:                     4, 4
                 Matern-3/2             exp 2; f = (1 + r) e: 2 more; f' = -1.5 e: 1 more:                      4, 3
                 Matern-5/2             exp 2; f = (1 + r + r r / 3) e: 5; f' = -(5/6)(1 + r) e: 4 (5/6 itself): 7, 6
                 rational quadratic     f = exp(-a l): 2; f' = -f / (2 (1 + v)): the addition, the division and the
                                        (d + 3) u of v (r2 and the division by a), v / (1 + v) <= 1:           2, 4 + d + 3
      terms    amp f: 1 more (E_f + 1).   -A amp f' then times D_k^2 (3 u): E_f' + 5.
               log_alpha: q - l cancels for small v, so its error is counted absolutely.  Its argument: d (q - l) / dv =
               -v / (1 + v)^2, so (d + 3) u q^2; q: addition and division 2 u q; l: log1p 2 u l; the subtraction, a f, times
               (q - l), times amp: with f's own, (E_f + 4 + c Arg) u |q - l|.  Together
                   u amp a f ((d + 3) q^2 + 2 q + 2 l + (E_f + 4 + c Arg) |q - l|).
      sums     n_acc roundings of partial sums, each at most sum |A T| (``acc_count``):
                 "device"  16 fused multiply-adds per thread (the products are not rounded), block_sum 6 + 3,
                           grad_final_kernel ceil(blocks / 256) additions per thread and block_sum 6 + 3; the weight 2 and
                           the halving are exact; the log_wn entry one more for the multiplication by wn;
                           mean: ceil(N / 256) + 9.
                 "numpy"   ``contract_numpy``: the product rounded (1), sr.sum8 along the rows and sum8 of the row sums,
                           2 (ceil(N / 8) + 3); log_wn one more; mean: ceil(N / 8) + 3.
    bound_p = 0.5 u sum_ij (2 a_ij |T_ij| + |A_ij| R_ij + n_acc |A_ij T_ij|),  R_ij = |T_ij| (E + c Arg_ij) or the log_alpha
    expression.  Entries of T in the denormal range add at most 2^-1074 a_ij each, below the resolution of every case here.

First-order end-to-end bound (``first_order_bound``), from the truth alone, the limit of what the formulation may lose:
    dA = d_alpha alpha^T + alpha d_alpha^T - dKinv,   |d_alpha| <= B_alpha of sr.first_order_bounds (G = sr.factor_allowed),
    |dKinv| <= |K^-1| G |K^-1|  +  Wd^T |W| + |W|^T Wd  +  (N + 2) u |W|^T |W|,      Wd = (N + 2) u |W||L||W|
    (the factor's own residual; any inverse with the count of sr's "generic" form; the N products and additions of W^T W),
    bound_p = B_alpha^T |T^p| |alpha| + 0.5 sum_ij |dKinv|_ij |T^p_ij| + given_bound at the truth (device counts);
    mean: sum B_alpha + its sum's bound.

fp64 restatements on the same inputs (``restatements``): LAPACK's factor of the fp64 K and cho_solve for alpha, then
    "wtw"     W = sr.lower_inverse_fp64(L), K^-1 = W^T W     (the library's route)
    "lapack"  K^-1 = cho_solve(L, I)
each contracted by ``contract_numpy``.
"""
from __future__ import annotations

import contextlib
import math

import numpy as np

import kernel_sum_reference as ksr
import solve_reference as sr

LD, U = ksr.LD, ksr.U
BLK = 64
E_F = {"ExpSquaredKernel": 4, "Matern32Kernel": 4, "Matern52Kernel": 7, "RationalQuadraticKernel": 2}
E_FP = {"ExpSquaredKernel": 4, "Matern32Kernel": 3, "Matern52Kernel": 6, "RationalQuadraticKernel": 4}   # + d + 3 for the last


def entry_names(d):
    return ["mean", "log_wn", "log_amp", "log_alpha"] + ["log_M_%d" % k for k in range(d)]


def family_entries(d, family):
    """The entries the family has: log_alpha only for the rational quadratic."""
    return [n for n in entry_names(d) if n != "log_alpha" or family == "RationalQuadraticKernel"]


# ------------------------------------------------------------------------------------------------- extended arithmetic
def _mp_context(obj):
    if not obj:
        return contextlib.nullcontext()
    import mpmath as mp
    return mp.workdps(ksr.MP_DIGITS)


_LIKE = {False: np.empty(0, dtype=LD), True: np.empty(0, dtype=object)}


def _lift(a, obj):
    """fp64 numbers in the working precision (exact): sr._lift, to long double or to mpmath objects."""
    a = np.asarray(a)
    return a if a.dtype == object else sr._lift(a, _LIKE[bool(obj)])


def _fn(name):
    def apply(x):
        x = np.asarray(x)
        if x.dtype == object:
            import mpmath as mp
            return np.frompyfunc(getattr(mp, name), 1, 1)(x)
        return getattr(np, name)(x)
    return apply


_exp, _sqrt, _log1p = _fn("exp"), _fn("sqrt"), _fn("log1p")


def radial_all(r2, family, a):
    """(f, f', a f (q - l)) of radial_with_derivative in the precision of r2; ``a`` the rational quadratic's alpha."""
    if family == "ExpSquaredKernel":
        f = _exp(-r2 / 2)
        return f, -f / 2, 0 * f
    if family == "Matern32Kernel":
        s = _sqrt(3 * r2); e = _exp(-s)
        return (1 + s) * e, -3 * e / 2, 0 * e
    if family == "Matern52Kernel":
        s = _sqrt(5 * r2); e = _exp(-s)
        return (1 + s + s * s / 3) * e, -5 * (1 + s) * e / 6, 0 * e
    if family == "RationalQuadraticKernel":
        v = r2 / (2 * a)
        l = _log1p(v)
        f = _exp(-a * l)
        return f, -f / (2 * (1 + v)), a * f * (v / (1 + v) - l)
    raise ValueError(family)


def _differences(xs, pairs=None):
    """(r2[N, N], [D_k^2[N, N]]) of scaled rows in their own precision; with ``pairs`` = (I, J) only those pairs, as vectors."""
    dk2 = []
    for k in range(xs.shape[1]):
        df = xs[:, k][:, None] - xs[:, k][None, :] if pairs is None else xs[pairs[0], k] - xs[pairs[1], k]
        dk2.append(df * df)
    r2 = dk2[0] * 1
    for t in dk2[1:]:
        r2 = r2 + t
    return r2, dk2


def _inputs(c):
    h = c["h"]
    amp, wn, inv_len = ksr.hyper_fp64(h["log_amp"], h["log_white_noise"], h["log_M"])
    return amp, wn, inv_len, math.exp(c["log_alpha"]), np.asarray(c["y"], dtype=np.float64) - h["mean"]


def _terms(c, obj, scale=None, pairs=None):
    """[T_amp, T_alpha, T_M_0 ...] in the working precision.  ``scale`` (extended numbers: amp, wn, a, per-coordinate factors of
    the scaled rows) replaces the lifted fp64 inputs for the central differences; ``pairs``: see _differences."""
    amp, wn, inv_len, a, _ = _inputs(c)
    xs = _lift(ksr.scaled(c["X"], inv_len), obj)
    amp, a = _lift(amp, obj)[()], _lift(a, obj)[()]
    if scale is not None:
        amp, a, xs = scale["amp"], scale["a"], xs * scale["x"][None, :]
    r2, dk2 = _differences(xs, pairs)
    f, fp, fa = radial_all(r2, c["family"], a)
    return [amp * f, amp * fa] + [-(amp * fp) * t for t in dk2]


def _contract(alpha, Kinv, c, obj, want_S=True):
    """(g, S) of the module docstring from extended alpha and K^-1.  The terms are symmetric, so the sum runs over the pairs
    i <= j with weight 2 off the diagonal and the mean of K^-1_ij and K^-1_ji (LAPACK's inverse is symmetric only to rounding):
    the same number as the sum over both triangles, at half the work.  ``want_S`` = False leaves S out (None)."""
    N = len(alpha)
    I, J = np.triu_indices(N)
    pairs, diag = (I, J), I == J
    wn = _lift(_inputs(c)[1], obj)[()]
    T = _terms(c, obj, pairs=pairs)
    aa, Kij = alpha[I] * alpha[J], (Kinv[I, J] + Kinv[J, I]) / 2
    w = np.where(diag, 1, 2).astype(alpha.dtype)
    A = w * (aa - Kij)
    g = [alpha.sum(), wn * A[diag].sum() / 2] + [(A * t).sum() / 2 for t in T]
    if not want_S:
        return np.array(g, dtype=alpha.dtype), None
    a = w * (np.abs(aa) + (np.abs(Kinv[I, J]) + np.abs(Kinv[J, I])) / 2)
    S = [np.abs(alpha).sum(), wn * a[diag].sum() / 2] + [(a * np.abs(t)).sum() / 2 for t in T]
    return np.array(g, dtype=alpha.dtype), sr._f64(np.array(S, dtype=alpha.dtype))


def truth(c, mp_route=False):
    """dict(g[4 + d] extended, S[4 + d] fp64, alpha, Kinv, K, L, W) of a case; ``mp_route`` forces mpmath at ksr.MP_DIGITS (the
    cross-check of the long-double route: S is then left out)."""
    obj = mp_route or not ksr.EXTENDED
    amp, wn, inv_len, _, r = _inputs(c)
    with _mp_context(obj):
        if obj:
            K = ksr._kernel_matrix_mp(c["X"], None, amp, wn, inv_len, c["family"], c["log_alpha"])
        else:
            K = ksr.kernel_matrix(c["X"], amp, wn, inv_len, c["family"], c["log_alpha"])
        L = ksr.cholesky(K)
        rl = _lift(r, obj)
        alpha = sr.backward_substitution(L, sr.forward_substitution(L, rl))
        W = sr.forward_substitution(L, _lift(np.eye(len(r)), obj))
        Kinv = W.T @ W
        g, S = _contract(alpha, Kinv, c, obj, want_S=not mp_route)
        logdet = 2 * sr._log(np.diagonal(L)).sum()
        nll = (rl @ alpha) / 2 + logdet / 2 + sr.log_2pi(L) * len(r) / 2
    return dict(g=g, S=S, alpha=alpha, Kinv=Kinv, K=K, L=L, W=W, nll=nll)


def nll_shifted(c, shift):
    """The truth's negative log-likelihood (long double) with entry ``name`` moved by ``h``: shift = (name, h).  The fp64 inputs
    stay what they are; amp, wn and alpha are multiplied by exp(h) and coordinate k by exp(-h / 2) in extended precision, the mean
    is moved by h."""
    name, h = shift
    amp, wn, inv_len, a, r = _inputs(c)
    d = c["X"].shape[1]
    h = LD(h)
    sc = dict(amp=LD(amp), a=LD(a), x=np.ones(d, dtype=LD))
    wn, rl = LD(wn), r.astype(LD)
    if name == "mean":
        rl = rl - h
    elif name == "log_wn":
        wn = wn * np.exp(h)
    elif name == "log_amp":
        sc["amp"] = sc["amp"] * np.exp(h)
    elif name == "log_alpha":
        sc["a"] = sc["a"] * np.exp(h)
    else:
        sc["x"][int(name.rsplit("_", 1)[1])] = np.exp(-h / 2)
    K = _terms(c, False, sc)[0]
    K[np.diag_indices_from(K)] += wn
    L = ksr.cholesky(K)
    alpha = sr.backward_substitution(L, sr.forward_substitution(L, rl))
    return (rl @ alpha) / 2 + np.log(np.diagonal(L)).sum() + sr.log_2pi() * len(rl) / 2


# ------------------------------------------------------------------------------------------ the contraction given its inputs
def contract_given(alpha_hat, Kinv_hat, c):
    """g[4 + d] in extended precision from fp64 alpha and K^-1 (module docstring)."""
    obj = not ksr.EXTENDED
    with _mp_context(obj):
        g, _ = _contract(_lift(alpha_hat, obj), _lift(Kinv_hat, obj), c, obj, want_S=False)
    return g


def acc_count(N, who):
    """(n_acc of the matrix entries, the count of the mean's sum)."""
    if who == "numpy":
        c = (N + 7) // 8 + 3
        return 2 * c + 1, c
    nb = (N + BLK - 1) // BLK
    blocks = nb * (nb + 1) // 2
    return 16 + 9 + (blocks + 255) // 256 + 9, (N + 255) // 256 + 9


def given_bound(alpha_hat, Kinv_hat, c, who="device"):
    """bound[4 + d] of the module docstring (fp64 magnitudes)."""
    family, d, N = c["family"], c["X"].shape[1], len(c["y"])
    amp, wn, inv_len, a_rq, _ = _inputs(c)
    al = np.asarray(alpha_hat, dtype=np.float64)
    Ki = np.asarray(Kinv_hat, dtype=np.float64)
    aa = np.abs(np.outer(al, al))
    Aabs, a = np.abs(np.outer(al, al) - Ki), aa + np.abs(Ki)
    xs = ksr.scaled(c["X"], inv_len)
    r2, dk2 = _differences(xs)
    f, fp, fa = radial_all(r2, family, a_rq)
    cArg = ksr.c_difference(d, family) * ksr.arg_difference(c["X"], inv_len, c["X"], family, c["log_alpha"])
    n_acc, n_mean = acc_count(N, who)
    e_fp = E_FP[family] + (d + 3 if family == "RationalQuadraticKernel" else 0)

    def entry(T, R, n):
        T = np.abs(T)
        return 0.5 * U * float(np.sum(2.0 * a * T + Aabs * R + n * Aabs * T))

    out = [n_mean * U * float(np.sum(np.abs(al))), wn * entry(np.eye(N), 0.0, n_acc + 1)]
    T = amp * f
    out.append(entry(T, np.abs(T) * (E_F[family] + 1 + cArg), n_acc))
    if family == "RationalQuadraticKernel":
        v = r2 / (2.0 * a_rq)
        q, l = v / (1.0 + v), np.log1p(v)
        R = amp * a_rq * f * ((d + 3) * q * q + 2.0 * q + 2.0 * l + (E_F[family] + 4 + cArg) * np.abs(q - l))
        out.append(entry(amp * fa, R, n_acc))
    else:
        out.append(0.0)
    for t in dk2:
        T = amp * fp * t
        out.append(entry(T, np.abs(T) * (e_fp + 5 + cArg), n_acc))
    return np.array(out)


# ------------------------------------------------------------------------------------------------- the fp64 restatements
def terms_fp64(c, plant=None):
    """[T_amp, T_alpha, T_M_0 ...] in plain fp64 NumPy in radial_with_derivative's operation order.  ``plant`` names a defect
    for the host test: "five_sixths", "log_for_log1p", "fprime_bias"."""
    amp, wn, inv_len, a, _ = _inputs(c)
    family = c["family"]
    xs = ksr.scaled(c["X"], inv_len)
    r2, dk2 = _differences(xs)
    fa = np.zeros_like(r2)
    if family == "ExpSquaredKernel":
        f = np.exp(-0.5 * r2); fp = -0.5 * f
    elif family == "Matern32Kernel":
        r = np.sqrt(3.0 * r2); e = np.exp(-r)
        f = (1.0 + r) * e; fp = -1.5 * e
    elif family == "Matern52Kernel":
        r = np.sqrt(5.0 * r2); e = np.exp(-r)
        f = (1.0 + r + r * r / 3.0) * e
        fp = -(0.8333333333 if plant == "five_sixths" else 5.0 / 6.0) * (1.0 + r) * e
    else:
        v = 0.5 * r2 / a
        l = np.log(1.0 + v) if plant == "log_for_log1p" else np.log1p(v)
        lf = np.log1p(v)
        f = np.exp(-a * lf)
        fp = -0.5 * f / (1.0 + v)
        fa = a * f * (v / (1.0 + v) - l)
    if plant == "fprime_bias":
        fp = fp * (1.0 + 2.0 ** -30)
    return [amp * f, amp * fa] + [(-(amp * fp)) * t for t in dk2]


def contract_numpy(alpha, Kinv, c, plant=None):
    """The contraction in plain fp64 NumPy: every sum by sr.sum8 (rows, then the row sums).  ``plant``: the three of terms_fp64,
    or ("block_once", ta, tb) the mirror image of one off-diagonal 64 x 64 block left out, "padded_row" one padding row of the
    device's layout admitted (alpha = 0 and K^-1 = I there: A = -1 on its diagonal, f(0) = 1), "no_wn" the trace part not
    multiplied by wn, ("swap", k, l) two log_M slots exchanged."""
    amp, wn, _, _, _ = _inputs(c)
    al = np.asarray(alpha, dtype=np.float64)
    A = al[:, None] * al[None, :] - np.asarray(Kinv, dtype=np.float64)
    T = terms_fp64(c, plant if isinstance(plant, str) else None)

    def total(P):
        if isinstance(plant, tuple) and plant[0] == "block_once":
            P = P.copy()
            ta, tb = plant[1:]
            P[tb * BLK:(tb + 1) * BLK, ta * BLK:(ta + 1) * BLK] = 0.0
        return sr.sum8(sr.sum8(P))

    tr = sr.sum8(np.diagonal(A).copy())
    s = [total(A * t) for t in T]
    if plant == "padded_row":
        tr, s[0] = tr - 1.0, s[0] - amp
    g = [sr.sum8(al), 0.5 * (tr if plant == "no_wn" else tr * wn)] + [0.5 * v for v in s]
    if isinstance(plant, tuple) and plant[0] == "swap":
        k, l = plant[1:]
        g[4 + k], g[4 + l] = g[4 + l], g[4 + k]
    return np.array(g, dtype=np.float64)


def restatements(c, K64, L_lapack, a_lapack):
    """{"wtw": (alpha, Kinv, g), "lapack": (alpha, Kinv, g)} in fp64 (module docstring)."""
    from scipy.linalg import cho_solve
    W = sr.lower_inverse_fp64(L_lapack)
    out = {}
    for tag, Kinv in (("wtw", W.T @ W), ("lapack", cho_solve((L_lapack, True), np.eye(len(L_lapack))))):
        out[tag] = (a_lapack, Kinv, contract_numpy(a_lapack, Kinv, c))
    return out


# ------------------------------------------------------------------------------------------ the first-order end-to-end bound
def first_order_bound(c, t, b_alpha, G):
    """bound[4 + d] of the module docstring from the truth ``t``, sr's B_alpha and the factor's allowance G."""
    amp, wn, _, _, _ = _inputs(c)
    N = len(c["y"])
    al, Ki = sr._f64(t["alpha"]), sr._f64(t["Kinv"])
    Wa, La = np.abs(sr._f64(t["W"])), np.abs(sr._f64(t["L"]))
    Wd = (N + 2) * U * (Wa @ (La @ Wa))
    dK = np.abs(Ki) @ G @ np.abs(Ki) + Wd.T @ Wa + Wa.T @ Wd + (N + 2) * U * (Wa.T @ Wa)
    T = [np.abs(x) for x in terms_fp64(c)]               # magnitudes: fp64 is ample
    gb = given_bound(al, Ki, c, "device")
    out = [float(np.sum(b_alpha)) + gb[0], 0.5 * wn * float(np.trace(dK)) + wn * float(b_alpha @ np.abs(al)) + gb[1]]
    for i, x in enumerate(T):
        out.append(float(b_alpha @ (x @ np.abs(al))) + 0.5 * float(np.sum(dK * x)) + gb[2 + i])
    return np.array(out)


# -------------------------------------------------------------------------------------------------- one case's reference
def reference(c):
    """Everything the tests need of a case, computed once: sr.reference's (K, L, LAPACK's factor and alpha, the allowance, the
    first-order bounds of alpha), the truth gradient with S, both restatements with their errors, and the first-order bound."""
    ref = sr.reference(c)
    t = truth(c)
    ref.update(g=t["g"], g64=sr._f64(t["g"]), S=t["S"], Kinv=t["Kinv"], W=t["W"], nll_hg=t["nll"])
    ref["fo_grad"] = first_order_bound(c, t, ref["fo"][0], ref["allowed"])
    ref["restate"] = restatements(c, ref["K64"], ref["L_lapack"], ref["a_lapack"])
    ref["e_ref"] = error(ref["restate"]["wtw"][2], t["g"])
    ref["e_lapack"] = error(ref["restate"]["lapack"][2], t["g"])
    return ref


def error(g_hat, g_true):
    """|g^ - g| entry by entry, the difference in the precision of the truth.  g^ in fp64 or long double (then lifted as the
    sum of its nearest double and the remainder, which is exact)."""
    obj = np.asarray(g_true).dtype == object
    g_hat = np.asarray(g_hat)
    with _mp_context(obj):
        hi = g_hat.astype(np.float64)
        lifted = _lift(hi, obj) + _lift((g_hat - hi.astype(g_hat.dtype)).astype(np.float64), obj)
        return np.abs(sr._f64(lifted - g_true))
