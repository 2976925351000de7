"""Training sets whose Cholesky factorisation fails at a KNOWN pivot, and the rule that says which: netlib's dpotf2.  Shared by
test_not_pd_host.py (the constructions against the rule and against LAPACK, on the oracle's matrix) and test_gpu_not_pd.py (every
factorisation path of csrc/gp_cholesky.hip (its kernels: csrc/chol_steps.hpp, csrc/chol_queue.hpp) and csrc/gp_append.hip
against ``p + 1``).  Not a test module.

The only way into the library is K = amp f(r) + wn I, so the failing pivot is placed through the training points:

(a) ``nonfinite_row``: one coordinate of row p is NaN / +inf / -inf.  Row and column p of K (at least K[p, p]: inf - inf) are
    NaN and nothing before column p is touched, so pivot p is the first that is not > 0: info = p + 1.
(b) ``ones_block``: log_amp = 0 and log_white_noise = -80 (1 + e^-80 rounds to 1) and rows q < p at the SAME point, 1000 away
    from the cloud in every coordinate.  For the squared-exponential and Matern kernels their covariance with every other point
    underflows to an exact 0, so rows q and p of K are zero except for K[q,q] = K[q,p] = K[p,p] = 1: L[q,q] = 1, L[p,q] = 1 and
    pivot p = 1 - 1 is an exact 0 in any order of summation: info = p + 1, the finite way to fail (rsq(0) instead of rsq(NaN)).
    The rational quadratic kernel never underflows; it gets (a) only.

``potf2_info`` is the reference for both.  scipy's dpotrf (OpenBLAS) agrees on (b) but returns info = 0 on a NaN pivot and leaves
the NaN on the diagonal, so it cannot referee (a).  For a large N the expectation needs no O(N^3) Python loop: the healthy K factors
(one dpotrf: ``healthy_factors``), hence every leading minor does, and pivot p is NaN or an exact zero."""
import numpy as np

FAR = 1000.0                                 # distance of the duplicated point of (b) from the cloud, per coordinate
ONES_HYPER = dict(log_amp=0.0, log_white_noise=-80.0)


def potf2_info(K):
    """LAPACK's ``info`` of the unblocked lower Cholesky factorisation of K, by netlib dpotf2's rule: column by column,
    ajj = K[j,j] - L[j,:j] . L[j,:j]; ``ajj <= 0 or isnan(ajj)`` ends it with info = j + 1; 0 when every pivot passes."""
    A = np.array(K, dtype=np.float64)
    n = A.shape[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(n):
            ajj = A[j, j] - np.dot(A[j, :j], A[j, :j])
            if ajj <= 0.0 or np.isnan(ajj):
                return j + 1
            ajj = np.sqrt(ajj)
            A[j, j] = ajj
            if j + 1 < n:
                A[j + 1:, j] = (A[j + 1:, j] - A[j + 1:, :j] @ A[j, :j]) / ajj
    return 0


def dpotrf_info(K):
    """info of scipy's LAPACK dpotrf (lower) on a copy of K."""
    from scipy.linalg import lapack
    return int(lapack.dpotrf(np.array(K, dtype=np.float64, order="F"), lower=1, overwrite_a=1)[1])


def healthy_factors(K):
    """The premise of ``p + 1`` at large N: the healthy matrix factors, with finite pivots."""
    from scipy.linalg import lapack
    c, info = lapack.dpotrf(np.array(K, dtype=np.float64, order="F"), lower=1, overwrite_a=1)
    return info == 0 and bool(np.all(np.isfinite(np.diag(c))) and np.all(np.diag(c) > 0.0))


def nonfinite_row(X, p, value=np.nan, coord=0):
    """(a): a copy of X with one coordinate of row p set to ``value`` (NaN, +inf or -inf)."""
    Xb = np.array(X, dtype=np.float64)
    Xb[p, coord] = value
    return Xb


def far_point(X):
    """A point FAR beyond the cloud in every coordinate."""
    return np.max(np.asarray(X, dtype=np.float64), axis=0) + FAR


def ones_block(X, q, p):
    """(b): a copy of X with rows q < p both at ``far_point(X)``; to be used with ONES_HYPER."""
    assert 0 <= q < p < len(X)
    Xb = np.array(X, dtype=np.float64)
    Xb[q] = Xb[p] = far_point(X)
    return Xb


def ones_hyper(h):
    """The hyper-parameters of (b): the problem's own mean and metric with unit amplitude and no nugget to speak of."""
    return dict(h, **ONES_HYPER)


def positions(N):
    """The pivot positions worth a case at size N: slab boundaries inside the first tile (16-column slabs), tile boundaries, panel
    boundaries of the 2/4/8-column panels (128/256/512) -- 512 is also the first grouped update of the task queue (8 block
    columns) --, a middle row of a middle block column, the first row of the last (ragged) tile, and the last two rows."""
    nb = (N + 63) // 64
    fixed = [0, 15, 16, 17, 47, 48, 63, 64, 65, 127, 128, 255, 256, 511, 512, 513]
    extra = [64 * (nb // 2) + 29, 64 * (nb - 1), N - 2, N - 1]
    return sorted({p for p in fixed + extra if 0 <= p < N})


def ones_pairs(N):
    """(q, p) of construction (b): q in an earlier block column than p (the 1 arrives through a panel solve and a trailing update),
    in the same tile but an earlier slab, and in the same slab; in the first tile, in a middle tile and in the last one."""
    nb = (N + 63) // 64
    out = [(3, 9), (5, 40)]                                    # first tile: same slab, earlier slab
    if nb >= 2:
        t = 64 * (nb // 2)
        hi = min(t + 63, N - 1)
        out += [(7, min(t + 33, N - 1)), (t, hi), (max(hi - 2, t), hi)]
        last = 64 * (nb - 1)
        if N - 1 > last:
            out += [(last, N - 1)]
        out += [(20, N - 1), (N - 2, N - 1)]
    return sorted({(q, p) for q, p in out if 0 <= q < p < N})
