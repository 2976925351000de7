"""Extended-precision truth and yardsticks for what PRODUCES the library's factor and alpha: every factorisation path, both
triangular-solve kernels, the append of one row, the two scalar reductions and K^-1 (tests/test_solve_reference_host.py,
tests/test_gpu_solve_truth.py).  Plain NumPy plus kernel_sum_reference (K and its Cholesky factor in 64-bit-significand
arithmetic from the library's own fp64 inputs); no GPU, nothing imported from alabi_amd.

u = 2^-53 throughout.  Every yardstick is either a count of roundings of honest fp64 arithmetic or a distance measured from the
truth; no constant is fitted to device output.

Factor (``factor_allowed``, ``factor_excess``)
    |L^ L^T - K|_ij <= u ((min(i, j) + 5) (|L||L^T|)_ij + |K_ij| (E + c A_ij))       (i, j counted from 0)
    min(i, j) fused updates of the entry, the scaling by the reciprocal square root and that root's own 1.3 u (a right-looking
    Cholesky, any blocking); K itself is assembled to u |K_ij| (E + c A_ij) (kernel_sum_reference: E roundings of a term, c
    of the exponential's argument A).  The product L^ L^T is formed in extended precision: formed in fp64 it would carry
    N u |L||L^T| of its own, the size of what is measured.

Solve (``omega``)
    omega = max_i |r - K a^|_i / (|L||L^T||a^|)_i, residual in extended precision: the component-wise backward error of a^ as
    the solution of a system whose matrix is perturbed relative to |L||L^T| (Higham, Accuracy and Stability, thm 7.3 with
    E = |L||L^T|).  Two substitutions give (L + dL1)(L^T + dL2) a^ = r with |dL| <= (N + 3) u |L| each (N - 1 fused updates of
    a row's right-hand side in any order, the multiplication by the stored reciprocal and that reciprocal's own rounding), and
    the factor's own |L L^T - K|: omega <= (3 N + 11) u to first order (``omega_first_order``).  LAPACK sits 100 times below
    that, so the working yardstick is LAPACK's own omega on the same case (tests: 10 omega_ref + 16 u).

Reductions given their inputs (``logdet_given`` / ``quad_given`` / ``nll_given`` and their ``*_bound``)
    log-determinant  2 sum log L_ii: the logarithm's ulp (counted 2 u), at most N - 1 additions of partial sums that are at most
                     sum |log L_ii|, the doubling exact: (N + 2) u 2 sum |log L_ii|.
    quadratic form   sum r_i a_i by fused multiply-adds (the product is not rounded), N additions: (N + 2) u sum |r_i a_i|.
    likelihood       0.5 q + 0.5 ld + 0.5 N log(2 pi) as api.hip forms it: the halvings and 0.5 N are exact; log(2 pi) in fp64
                     carries the rounding of 2 pi, the logarithm's 2 u and the multiplication: 4 u of the third term; two
                     additions, each u of a partial sum that is at most |t1| + |t2| + |t3|.
    These are tight: they separate the reduction kernels from the factor and the solve.

Inverse (``inverse_omega``): omega column by column, K^-1[:, j] as the solution of K x = e_j.

Append (``append_numpy``, ``append_bound``)
    gp_append.hip extends L and the cached W = L^-1 by one row:  l = W k,  l_nn = sqrt(kss - |l|^2),  W' row = -(l^T W) / l_nn.
    With R = L^ W^ - I the right residual of the stored inverse, row n of the extended factor satisfies, for j < n,
        (L^ l^)_j - K_nj = dk_j + (R k)_j + (L^ e)_j,       |e| <= c_l u |W||k|  the roundings of the product W k,
    i.e.  |.| <= u |K_nj| (E + c A_nj) + (|R||k|)_j + c_l u (|L||W||k|)_j.  The rows of R:
      * an appended row m: l_m^T W + l_mm w_m vanishes in exact arithmetic WHATEVER the error of the W it was formed from, so
        it holds only the roundings of that product and of the division, (c_w + 1) u (|L||W|)_m., and u on the diagonal:
        the right residual does not accumulate over the rows appended since the last factorisation;
      * a row of the last factorisation: form "substitution" -- W solved column by column, (L + dL_j) w_j = e_j,
        |R| <= c_0 u |L||W|; form "generic" -- any inverse with |dW| <= (n0 + 2) u |W||L||W| (the count of derived_bound
        in test_gpu_variance_truth.py; it covers the block-recursive inverse of gp_inverse.hip), |R| <= (n0 + 2) u |L||W||L||W|.
    The diagonal entry: |l|^2 + l_nn^2 - K_nn is the rounding of the sum of squares, the subtraction and the root,
    u (c_p |l|^2 + 4 K_nn).
    Counts (``append_counts``), tiles = ceil(n / 64):
      "device"  c_l = 8 tiles + 3 (append_lrow_kernel: two accumulators of 8 fused multiply-adds per 64-column tile, their sum,
                two shuffles), c_w = tiles + 63 (append_wrow_kernel: one fused multiply-add per 64 rows, then the 64-way LDS
                sum in a fixed order), c_p = ceil(n / 256) + 10 (append_pivot_kernel: one fused multiply-add per 256 rows, the
                wave and block sums), c_0 = n0 + 2;
      "numpy"   every sum of append_numpy goes through sum8, the same eight-accumulator layout in NumPy: ceil(n / 8) + 3 and the
                product's own rounding (NumPy has no fused multiply-add), c_l = c_w = c_p = ceil(n / 8) + 4, and
                c_0 = ceil(n0 / 8) + 5 with the division.  (With BLAS products the order, hence the count, would be unknown;
                the any-order count n made the bound 40 times slack on the ill-conditioned chain.)
    Multiplying by an explicit inverse is not backward stable to the Cholesky count: |L||W| grows with the conditioning.  The
    host test shows how far the NumPy statement is from the fresh allowance, and that the "substitution" bound is within a
    factor 20 of what that statement actually loses.

First-order end-to-end bounds (``first_order_bounds``), from the truth alone, with G the element-wise bound of L^ L^T - K
(factor_allowed, or append_bound on the appended rows) and S = 2 (N + 3) u |L||L^T||alpha| the two substitutions:
    alpha    |K^-1| (G |alpha| + S)                              logdet   sum_ij |K^-1|_ij G_ij  +  logdet_bound
    quad     |alpha|^T G |alpha| + 2 |alpha|^T S + quad_bound
They exceed LAPACK's actual error 100 to 1000 times and would alone catch nothing subtle; they are asserted unconditionally
as the limit of what the formulation may lose.

Restatement (``blocked_solve_numpy``): the device's operation order in fp64 -- 64-row blocks, multiplication by a stored
1 / L_ii, "stream" (trsv_stream_kernel: the off-diagonal products of a block row accumulated, subtracted once) or "steps"
(trsv_fwd_step_kernel / trsv_bwd_step_kernel: subtracted after every block step).
"""
from __future__ import annotations

import math

import numpy as np

import kernel_sum_reference as ksr

LD, U = ksr.LD, ksr.U
BLK = 64
GRID_N = (1, 63, 64, 65, 128, 129, 200)
GRID_D = ((3, -12.0), (10, -8.0))
SEED = 7


# ------------------------------------------------------------------------------------------------------------ the cases
def _target(X, seed):
    """make_problem's targets at other inputs (the same random stream: X, then the precision matrix)."""
    N, d = X.shape
    rng = np.random.RandomState(seed)
    rng.uniform(-3.0, 3.0, (N, d))
    A = rng.randn(d, d)
    prec = A @ A.T / d + 0.5 * np.eye(d)
    return -0.5 * np.einsum("ni,ij,nj->n", X, prec, X) / d


def case(name, make_problem):
    """dict(X, y, h, family, log_alpha) of a named case.  ``make_problem`` is conftest's.
      nNdD            make_problem(N, D, 7), nugget e^-12 at d = 3 and e^-8 at d = 10 (N = 1: the one target IS the median and has
                      no variance, so the mean is moved by 0.37 to keep the right-hand side from vanishing and the amplitude is 1)
      n129d3-FAMILY   the other three kernel families
      ill             ell2 = 8, N = 192, d = 3: length scales twice as long, cond(K) at the limit of fp64
      clustered       N = 128, d = 3, the last half of the rows replaced by random earlier rows displaced by 1e-2 length scales
                      per coordinate (normal, RandomState(8)): the points an active learner adds
      big             N = 705, d = 6: 11 block rows"""
    family, log_alpha = "ExpSquaredKernel", 1.0
    if name == "ill":
        X, y, h = make_problem(192, 3, SEED, log_wn=-12.0, ell2=8.0)
    elif name == "big":
        X, y, h = make_problem(705, 6, SEED, log_wn=-12.0)
    elif name == "clustered":
        X, y, h = make_problem(128, 3, SEED, log_wn=-12.0)
        inv_len = ksr.hyper_fp64(h["log_amp"], h["log_white_noise"], h["log_M"])[2]
        rng = np.random.RandomState(SEED + 1)
        X = X.copy()
        X[64:] = X[rng.randint(0, 64, 64)] + 1e-2 * rng.randn(64, 3) / inv_len[None, :]
        y = _target(X, SEED)
    else:
        head, _, fam = name.partition("-")
        N, d = (int(v) for v in head[1:].split("d"))
        with np.errstate(divide="ignore"):               # one target has no variance: make_problem takes its logarithm
            X, y, h = make_problem(N, d, SEED, log_wn=dict(GRID_D)[d])
        if fam:
            family = fam
        if N == 1:
            h = dict(h, mean=h["mean"] + 0.37, log_amp=0.0)
    return dict(name=name, X=X, y=y, h=h, family=family, log_alpha=log_alpha)


GRID = ["n%dd%d" % (N, d) for d, _ in GRID_D for N in GRID_N]
FAMILY_CASES = ["n129d3-" + f for f in ksr.FAMILIES[1:]]
# (case, n0): 63 consecutive appends from n0 rows to n0 + 63
APPEND_CHAINS = [("n128d3", 65), ("n128d10", 65), ("n64d3", 1), ("ill", 129), ("clustered", 65)]


def kernel_fp64(X1, X2, amp, inv_len, family="ExpSquaredKernel", log_alpha=1.0):
    """amp f(r2) in plain fp64 NumPy (the honest fp64 statement of the assembly; r2 coordinate by coordinate)."""
    r2 = ksr._r2(ksr.scaled(X1, inv_len), ksr.scaled(X2, inv_len), np.float64)
    if family == "ExpSquaredKernel":
        f = np.exp(-0.5 * r2)
    elif family == "Matern32Kernel":
        s = np.sqrt(3.0 * r2); f = (1.0 + s) * np.exp(-s)
    elif family == "Matern52Kernel":
        s = np.sqrt(5.0 * r2); f = (1.0 + s + s * s / 3.0) * np.exp(-s)
    else:
        a = math.exp(log_alpha); f = np.exp(-a * np.log1p(r2 / (2.0 * a)))
    return amp * f


def matrix_fp64(X, amp, wn, inv_len, family="ExpSquaredKernel", log_alpha=1.0):
    K = kernel_fp64(X, X, amp, inv_len, family, log_alpha)
    K[np.diag_indices_from(K)] = amp + wn
    return K


# ---------------------------------------------------------------------------------------------------------- the truths
def _prec():
    """The working precision of the mpmath route (where np.longdouble is only a double); nothing to set for long double."""
    if ksr.EXTENDED:
        import contextlib
        return contextlib.nullcontext()
    import mpmath as mp
    return mp.workdps(ksr.MP_DIGITS)


def _ext(a):
    """fp64 numbers in the precision of the truth (exact): long double, or mpmath objects where that is only a double."""
    a = np.asarray(a)
    if a.dtype == object or (ksr.EXTENDED and a.dtype == LD):
        return a
    if ksr.EXTENDED:
        return a.astype(LD)
    import mpmath as mp
    return np.array([mp.mpf(float(v)) for v in a.ravel()], dtype=object).reshape(a.shape)


def _f64(a):
    """The nearest doubles of extended-precision numbers."""
    return np.asarray(a).astype(np.float64)


def _log(v):
    if v.dtype == object:
        import mpmath as mp
        return np.array([mp.log(x) for x in v], dtype=object)
    return np.log(v)


def forward_substitution(L, B):
    """L^-1 B row by row in the precision of L (long double or mpmath objects), B[N] or B[N, M]."""
    B = np.asarray(B, dtype=L.dtype)
    V = np.empty_like(B)
    for i in range(L.shape[0]):
        V[i] = (B[i] - (L[i, :i] @ V[:i] if i else 0)) / L[i, i]
    return V


def backward_substitution(L, B):
    """L^-T B row by row from the last, in the precision of L."""
    B = np.asarray(B, dtype=L.dtype)
    V = np.empty_like(B)
    n = L.shape[0]
    for i in range(n - 1, -1, -1):
        V[i] = (B[i] - (L[i + 1:, i] @ V[i + 1:] if i + 1 < n else 0)) / L[i, i]
    return V


def _lift(a, like):
    """fp64 numbers in the precision of ``like`` (exact)."""
    a = np.asarray(a, dtype=np.float64)
    if like.dtype == object:
        import mpmath as mp
        return np.array([mp.mpf(float(v)) for v in a.ravel()], dtype=object).reshape(a.shape)
    return a.astype(LD)


def log_2pi(like=None):
    """log(2 pi) in extended precision (the constant's 21 digits; mpmath's where the truth is mpmath's)."""
    if like is not None and like.dtype == object:
        import mpmath as mp
        return mp.log(2 * mp.pi)
    return LD("1.8378770664093454835606594728112353")


def truths(L, r):
    """alpha_true = L^-T L^-1 r, logdet_true = 2 sum log L_ii, quad_true = r^T alpha_true, nll_true, from the truth's factor."""
    with _prec():
        rl = _lift(r, L)
        alpha = backward_substitution(L, forward_substitution(L, rl))
        logdet = 2 * _log(np.diagonal(L)).sum()
        quad = rl @ alpha
        nll = quad / 2 + logdet / 2 + log_2pi(L) * len(rl) / 2
    return dict(alpha=alpha, logdet=logdet, quad=quad, nll=nll)


# ----------------------------------------------------------------------------------------------------------- the factor
def factor_allowed(X, inv_len, K, L, d, family="ExpSquaredKernel", log_alpha=1.0):
    """The element-wise allowance of |L^ L^T - K| (module docstring).  K, L: the truth's (magnitudes taken in fp64)."""
    N = len(X)
    Lf = np.abs(np.asarray(L, dtype=np.float64))
    idx = np.minimum(np.arange(N)[:, None], np.arange(N)[None, :]) + 5.0
    return U * (idx * (Lf @ Lf.T) + np.abs(np.asarray(K, dtype=np.float64)) *
                (ksr.E_FAMILY[family] + ksr.c_difference(d, family) * ksr.arg_difference(X, inv_len, X, family, log_alpha)))


def factor_residual(L_hat, K_ld):
    """L^ L^T - K with the product formed in extended precision, rounded once to fp64."""
    with _prec():
        Lh = _ext(np.asarray(L_hat, dtype=np.float64))
        return _f64(Lh @ Lh.T - _ext(K_ld))


def factor_excess(L_hat, K_ld, allowed):
    """|L^ L^T - K|_ij / allowed_ij, element by element."""
    return np.abs(factor_residual(L_hat, K_ld)) / allowed


# ------------------------------------------------------------------------------------------------------------ the solve
def _ratio(num, den):
    """num / den with 0 / 0 = 0 (a vanishing right-hand side has a vanishing solution and no backward error)."""
    num = np.asarray(num, dtype=np.float64); den = np.asarray(den, dtype=np.float64)
    out = np.zeros_like(num)
    nz = den > 0
    out[nz] = num[nz] / den[nz]
    out[~nz & (num > 0)] = np.inf
    return out


def omega(K_ld, L, alpha_hat, r):
    """max_i |r - K a^|_i / (|L||L^T||a^|)_i, residual in long double (module docstring)."""
    a = np.asarray(alpha_hat, dtype=np.float64)
    with _prec():
        res = np.abs(_f64(_ext(np.asarray(r, dtype=np.float64)) - _ext(K_ld) @ _ext(a)))
    Lf = np.abs(np.asarray(L, dtype=np.float64))
    return float(np.max(_ratio(res, Lf @ (Lf.T @ np.abs(a)))))


def omega_first_order(N):
    """(3 N + 11) u: two substitutions of (N + 3) u each and the factor's (N + 5) u, all relative to |L||L^T|."""
    return (3 * N + 11) * U


def inverse_omega(K_ld, L, Kinv_hat):
    """omega column by column: max_ij |I - K Kinv^|_ij / (|L||L^T||Kinv^|)_ij."""
    Ki = np.asarray(Kinv_hat, dtype=np.float64)
    with _prec():
        res = _ext(K_ld) @ _ext(Ki)
        res[np.diag_indices_from(res)] -= 1
        res = np.abs(_f64(res))
    Lf = np.abs(np.asarray(L, dtype=np.float64))
    return float(np.max(_ratio(res, Lf @ (Lf.T @ np.abs(Ki)))))


def sum8(T):
    """Sum along the last axis in a STATED order: eight interleaved accumulators (entry j goes to accumulator j mod 8), then a
    three-level tree -- ceil(n / 8) + 3 roundings at most per result, the layout of append_lrow_kernel's row sums (four lanes
    of two accumulators, their sum and two shuffles).  A BLAS product would leave the order, and so the count, unknown."""
    T = np.asarray(T, dtype=np.float64)
    n = T.shape[-1]
    if n % 8:
        T = np.concatenate([T, np.zeros(T.shape[:-1] + (8 - n % 8,))], axis=-1)      # adding zeros is exact
    T = T.reshape(T.shape[:-1] + (-1, 8))
    acc = np.zeros(T.shape[:-2] + (8,))
    for c in range(T.shape[-2]):
        acc = acc + T[..., c, :]
    a = acc[..., :4] + acc[..., 4:]
    a = a[..., :2] + a[..., 2:]
    return a[..., 0] + a[..., 1]


def lower_inverse_fp64(L, ordered=False):
    """W = L^-1 in fp64, column by column by forward substitution (vectorised over the columns).  ``ordered``: the row sums by
    sum8 (the append statement, whose count must be known); otherwise a BLAS product (magnitudes for the bounds)."""
    n = L.shape[0]
    W = np.zeros((n, n))
    for i in range(n):
        if i:
            W[i, :i] = -(sum8(W[:i, :i].T * L[i, :i][None, :]) if ordered else L[i, :i] @ W[:i, :i]) / L[i, i]
        W[i, i] = 1.0 / L[i, i]
    return W


# -------------------------------------------------------------------------------------- reductions given their inputs
def logdet_given(L_hat):
    with _prec():
        return 2 * _log(_ext(np.diagonal(np.asarray(L_hat, dtype=np.float64)).copy())).sum()


def logdet_bound(L_hat):
    N = len(L_hat)
    return (N + 2) * U * 2.0 * float(np.sum(np.abs(np.log(np.diagonal(np.asarray(L_hat, dtype=np.float64))))))


def quad_given(r, alpha_hat):
    with _prec():
        return _ext(np.asarray(r, dtype=np.float64)) @ _ext(np.asarray(alpha_hat, dtype=np.float64))


def quad_bound(r, alpha_hat):
    return (len(r) + 2) * U * float(np.sum(np.abs(np.asarray(r, dtype=np.float64) * np.asarray(alpha_hat, dtype=np.float64))))


def nll_given(L_hat, r, alpha_hat):
    with _prec():
        return quad_given(r, alpha_hat) / 2 + logdet_given(L_hat) / 2 + log_2pi(_ext(np.zeros(1))) * len(r) / 2


def nll_bound(L_hat, r, alpha_hat):
    t1, t2 = abs(float(quad_given(r, alpha_hat))) / 2, abs(float(logdet_given(L_hat))) / 2
    t3 = 0.5 * len(r) * math.log(2.0 * math.pi)
    return 0.5 * quad_bound(r, alpha_hat) + 0.5 * logdet_bound(L_hat) + U * (4.0 * t3 + 2.0 * (t1 + t2 + t3))


# ------------------------------------------------------------------------------------------------------------ the append
def append_numpy(K64, n0, plant=None):
    """gp_append.hip's algebra in plain fp64 NumPy: the leading n0 x n0 block factorised (LAPACK) and inverted (substitution),
    then every further row by  l = W k,  l_nn = sqrt(kss - |l|^2),  W' row = -(l^T W) / l_nn, every sum by sum8.  Returns (L, W).
    ``plant`` = (n, i, j, eps) plants a defect for the host test: row n forms its l from a W whose entry (i, j) is off by eps."""
    N = K64.shape[0]
    L, W = np.zeros((N, N)), np.zeros((N, N))
    L[:n0, :n0] = np.linalg.cholesky(K64[:n0, :n0])
    W[:n0, :n0] = lower_inverse_fp64(L[:n0, :n0], ordered=True)
    for n in range(n0, N):
        Wn = W[:n, :n]
        if plant is not None and plant[0] == n:
            Wn = Wn.copy(); Wn[plant[1], plant[2]] *= 1.0 + plant[3]
        l = sum8(Wn * K64[:n, n][None, :])
        piv = K64[n, n] - sum8(l * l)
        if not piv > 0:
            raise np.linalg.LinAlgError(f"{n + 1}-th leading minor of the array is not positive definite")
        lnn = math.sqrt(piv)
        L[n, :n], L[n, n] = l, lnn
        W[n, :n], W[n, n] = -sum8(W[:n, :n].T * l[None, :]) / lnn, 1.0 / lnn
    return L, W


def append_counts(n, who):
    """(c_l, c_w, c_p) of a row appended to n existing rows: the roundings of one entry of W k, of l^T W and of |l|^2 (module
    docstring)."""
    if who == "numpy":
        c = float((n + 7) // 8 + 4)
        return c, c, c
    tiles = (n - 1) // BLK + 1
    return 8.0 * tiles + 3.0, tiles + 63.0, (n + 255) // 256 + 10.0


def append_bound(X, inv_len, K, L, d, n0, who, form, family="ExpSquaredKernel", log_alpha=1.0):
    """Element-wise bound G[N, N] of |L^ L^T - K| for a factor whose rows n0.. were appended one at a time (module docstring);
    the leading n0 x n0 block is factor_allowed.  K, L: the truth's; magnitudes in fp64, W = L^-1 by substitution."""
    N = len(X)
    Kf = np.abs(np.asarray(K, dtype=np.float64))
    Lt = np.asarray(L, dtype=np.float64)
    La, Wa = np.abs(Lt), np.abs(lower_inverse_fp64(Lt))
    G = factor_allowed(X, inv_len, K, L, d, family, log_alpha)
    assembly = U * Kf * (ksr.E_FAMILY[family] + ksr.c_difference(d, family) * ksr.arg_difference(X, inv_len, X, family, log_alpha))
    P = La @ Wa                                          # lower triangular; its leading blocks are those of the leading factors
    R = np.zeros((N, N))
    P0 = P[:n0, :n0]
    c_fresh = (n0 + 7) // 8 + 5 if (who, form) == ("numpy", "substitution") else n0 + 2
    R[:n0, :n0] = c_fresh * U * (P0 if form == "substitution" else P0 @ P0)
    cl, cp = np.zeros(N), np.zeros(N)
    for n in range(n0, N):
        cl[n], cw, cp[n] = append_counts(n, who)
        R[n, :n] = (cw + 1.0) * U * P[n, :n]
        R[n, n] = U
    Koff = np.triu(Kf, 1)                                # column n holds |k| of row n: the rows above the diagonal
    T = (R @ Koff).T + (cl * U)[:, None] * (P @ Koff).T  # [n, j], j < n
    rows = np.arange(N)[:, None] >= n0
    low = np.tril(np.ones((N, N), dtype=bool), -1)
    B = np.where(low & rows, assembly + T, 0.0)
    B = B + B.T
    l2 = np.sum(Lt * Lt, axis=1) - np.diagonal(Lt) ** 2
    diag = U * (cp * l2 + 4.0 * np.diagonal(Kf))
    out = G.copy()
    sel = (np.arange(N)[:, None] >= n0) | (np.arange(N)[None, :] >= n0)
    out[sel] = B[sel]
    app = np.arange(N) >= n0
    out[app, app] = diag[app]
    return out


# ------------------------------------------------------------------------------------------- first-order end-to-end bounds
def first_order_bounds(K, L, r, G):
    """(B_alpha[N], B_logdet, B_quad, B_nll) of the module docstring from the truth's K, L (magnitudes in fp64)."""
    Lt = np.asarray(L, dtype=np.float64)
    N = len(Lt)
    W = lower_inverse_fp64(Lt)
    Kinv = np.abs(W.T @ W)
    rf = np.asarray(r, dtype=np.float64)
    a = np.abs(W.T @ (W @ rf))
    La = np.abs(Lt)
    S = 2.0 * (N + 3) * U * (La @ (La.T @ a))
    b_alpha = Kinv @ (G @ a + S)
    b_logdet = float(np.sum(Kinv * G)) + logdet_bound(Lt)
    b_quad = float(a @ (G @ a) + 2.0 * (a @ S)) + (N + 2) * U * float(np.sum(np.abs(rf) * a))
    t3 = 0.5 * N * math.log(2.0 * math.pi)
    b_nll = 0.5 * b_quad + 0.5 * b_logdet + U * (4.0 * t3 + 2.0 * (0.5 * float(np.abs(rf) @ a) + float(np.sum(np.abs(np.log(np.diagonal(Lt))))) + t3))
    return b_alpha, b_logdet, b_quad, b_nll


# ------------------------------------------------------------------------------------------------------- the restatement
def blocked_solve_numpy(L, r, reciprocal=True, mode="stream", lose=None):
    """alpha = L^-T L^-1 r in fp64 in the device's operation order (module docstring).  ``lose`` = (i, k, eps) plants a defect
    for the host test: the forward sweep sees (1 - eps) L[i, k] of that 64 x 64 off-diagonal block."""
    L = np.asarray(L, dtype=np.float64)
    N = len(L)
    nb = (N + BLK - 1) // BLK
    Np = nb * BLK
    Lp = np.eye(Np); Lp[:N, :N] = L                     # the padding rows are the identity, as in the device's layout
    rp = np.zeros(Np); rp[:N] = r
    dg = np.diagonal(Lp).copy()
    dinv = 1.0 / dg
    blk = lambda i, k: Lp[i * BLK:(i + 1) * BLK, k * BLK:(k + 1) * BLK]  # noqa: E731

    def scale(v, j, b):
        return v * dinv[b * BLK + j] if reciprocal else v / dg[b * BLK + j]

    z = np.zeros(Np)
    for i in range(nb):
        acc, v = np.zeros(BLK), rp[i * BLK:(i + 1) * BLK].copy()
        for k in range(i):
            Lik = blk(i, k) * (1.0 - lose[2]) if lose is not None and (i, k) == tuple(lose[:2]) else blk(i, k)
            p = Lik @ z[k * BLK:(k + 1) * BLK]
            if mode == "stream":
                acc += p
            else:
                v -= p
        if mode == "stream":
            v -= acc
        D = blk(i, i)
        for j in range(BLK):
            v[j] = scale(v[j], j, i)
            v[j + 1:] -= D[j + 1:, j] * v[j]
        z[i * BLK:(i + 1) * BLK] = v
    a = np.zeros(Np)
    for i in range(nb - 1, -1, -1):
        acc, v = np.zeros(BLK), z[i * BLK:(i + 1) * BLK].copy()
        for k in range(nb - 1, i, -1):
            p = blk(k, i).T @ a[k * BLK:(k + 1) * BLK]
            if mode == "stream":
                acc += p
            else:
                v -= p
        if mode == "stream":
            v -= acc
        D = blk(i, i)
        for j in range(BLK - 1, -1, -1):
            v[j] = scale(v[j], j, i)
            v[:j] -= D[j, :j] * v[j]
        a[i * BLK:(i + 1) * BLK] = v
    return a[:N]


# -------------------------------------------------------------------------------------------------- one case's reference
def reference(c, n0=None):
    """Everything the tests need of a case, computed once: the truth (K, L, alpha, logdet, quad, nll), the fp64 K, LAPACK's
    factor and cho_solve with their excess and omega, the allowance and the first-order bounds; with ``n0`` also the append
    statement (L_app, W_app), its excess and both append bounds."""
    X, y, h, family, log_alpha = c["X"], c["y"], c["h"], c["family"], c["log_alpha"]
    N, d = X.shape
    amp, wn, inv_len = ksr.hyper_fp64(h["log_amp"], h["log_white_noise"], h["log_M"])
    r = y - h["mean"]
    K = ksr.kernel_matrix(X, amp, wn, inv_len, family, log_alpha)
    L = ksr.cholesky(K)
    t = truths(L, r)
    K64 = matrix_fp64(X, amp, wn, inv_len, family, log_alpha)
    allowed = factor_allowed(X, inv_len, K, L, d, family, log_alpha)
    L_lapack = np.linalg.cholesky(K64)
    a_lapack = _cho_solve(L_lapack, r)
    out = dict(c, N=N, d=d, amp=amp, wn=wn, inv_len=inv_len, r=r, K=K, L=L, K64=K64, allowed=allowed, L_lapack=L_lapack,
               a_lapack=a_lapack, omega_ref=omega(K, L, a_lapack, r), **t)
    out["alpha64"] = _f64(t["alpha"])
    out["fo"] = first_order_bounds(K, L, r, allowed)
    if n0 is not None:
        out["n0"] = n0
        out["L_app"], out["W_app"] = append_numpy(K64, n0)
        for who in ("numpy", "device"):
            for form in ("substitution", "generic"):
                out["G_%s_%s" % (who, form)] = append_bound(X, inv_len, K, L, d, n0, who, form, family, log_alpha)
        out["fo_app"] = first_order_bounds(K, L, r, out["G_device_generic"])
    return out


def _cho_solve(L, r):
    """LAPACK's two triangular solves where SciPy is there, otherwise the general solver on the triangles."""
    try:
        from scipy.linalg import cho_solve
        return cho_solve((L, True), r)
    except ImportError:                                  # pragma: no cover
        return np.linalg.solve(L.T, np.linalg.solve(L, r))
