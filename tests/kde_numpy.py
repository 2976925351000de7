"""The device form of the Gaussian KDE (alabi_amd/csrc/kde.hip) in fp64 NumPy: the specification of the kernels and the yardstick
of the statistical criterion of tests/test_gpu_kde_truth.py.  Same steps, same layout, same constants; the order of the additions
inside a part and libm's exp2 in place of exp2s_tab256 are the only liberties (they change individual roundings, not their number).

``defect=`` plants one of DEFECTS, for tests/test_kde_reference_host.py: each is a mistake the kernels could make and the suite has
to notice."""
from __future__ import annotations

import math

import numpy as np

KDE_LOG0 = -1.0e300
KDE_TAIL = -650.0
KDE_LN2_256 = 0.0027076061740622863
KDE_TARGET_WGS = 2048
EXP2S256_SCALE = 369.3299304675746           # 256 / ln2
EXP2S_CLAMP = -280064.0                      # exp2s_tab256 clamps its argument here (2^-1094: 0 after ldexp)

DEFECTS = ("drop_last_part", "pad_weight", "no_shift_back", "shift_f32", "first_part_max", "no_centre", "logw_f32", "stale_kstep")


def kde_rows(d):
    return (d + 2 + 3) // 4 * 4


def kde_qt(rows):
    """Query tiles per wavefront: four while rows / 4 <= 8 (d <= 30), two above."""
    return 4 if rows // 4 <= 8 else 2


def kde_plan(Npad, M, rows):
    """(parts, pts): the sample axis in ``parts`` runs of ``pts`` samples, a function of the shapes only."""
    qpb = 4 * 16 * kde_qt(rows)
    wgs = (M + qpb - 1) // qpb
    tiles = Npad // 16
    parts = 1
    if wgs < KDE_TARGET_WGS:
        parts = (KDE_TARGET_WGS + wgs - 1) // wgs
        parts = min(parts, tiles // 8)
        parts = max(parts, 1)
    pts = (tiles + parts - 1) // parts * 16
    return (Npad + pts - 1) // pts, pts


def whiten(P, c, L):
    """Rows of L^-1 (p - c) by forward substitution, and their squared norms accumulated coordinate by coordinate."""
    d = L.shape[0]
    out = np.empty_like(P)
    nn = np.zeros(P.shape[0])
    for k in range(d):
        v = P[:, k] - c[k]
        for j in range(k):
            v = v - L[k, j] * out[:, j]
        out[:, k] = v / L[k, k]
        nn = out[:, k] * out[:, k] + nn
    return out, nn


def prepare_samples(X, logw, L, defect=None):
    """(Sa [rows][Npad], centre): augmented sample rows (z, -|z|^2/2 + log w, 1, 0..); padding and zero weights carry KDE_LOG0."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    N, d = X.shape
    rows, Npad = kde_rows(d), (N + 15) // 16 * 16
    c = np.zeros(d) if defect == "no_centre" else np.sum(X, axis=0) / N
    lw = np.full(N, -math.log(float(N))) if logw is None else np.array(logw, dtype=np.float64)
    if defect == "logw_f32":
        lw = lw.astype(np.float32).astype(np.float64)
    lw = np.where(lw > KDE_LOG0, lw, KDE_LOG0)           # -inf and NaN -> the finite sentinel
    z, zz = whiten(X, c, L)
    Sa = np.zeros((rows, Npad))
    Sa[:d, :N] = z.T
    Sa[d, :] = KDE_LOG0
    Sa[d, :N] = np.where(lw > KDE_LOG0, -0.5 * zz + lw, KDE_LOG0)
    if defect == "pad_weight":
        Sa[d, N:] = -math.log(float(N))
    Sa[d + 1, :] = 1.0
    return Sa, c


def prepare_queries(Q, c, L):
    """Qa [M][rows]: (u, 1, -|u|^2/2, 0..) * 256/ln2."""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    M, d = Q.shape
    u, uu = whiten(Q, c, L)
    Qa = np.zeros((M, kde_rows(d)))
    Qa[:, :d] = u * EXP2S256_SCALE
    Qa[:, d] = EXP2S256_SCALE
    Qa[:, d + 1] = -0.5 * uu * EXP2S256_SCALE
    return Qa


def partial(Sa, Qa, parts, pts, d, defect=None):
    """(psum, pmax) [parts][M]: per part the sum of 2^(q'.s'/256) and the largest q'.s' (scaled)."""
    rows, Npad = Sa.shape
    M = Qa.shape[0]
    psum = np.zeros((parts, M)); pmax = np.full((parts, M), -np.inf)
    A = Qa
    if defect == "stale_kstep" and rows == d + 2 and rows >= 8:
        A = Qa.copy()
        A[:, rows - 4:] = Qa[:, rows - 8:rows - 4]       # the last k-step's A operand read from the one before
    for part in range(parts):
        lo, hi = part * pts, min(Npad, (part + 1) * pts)
        if defect == "drop_last_part" and part == parts - 1 and parts > 1 and parts * pts > Npad:
            continue
        acc = np.zeros((M, hi - lo))
        for k in range(rows):
            acc = A[:, k][:, None] * Sa[k, lo:hi][None, :] + acc
        with np.errstate(under="ignore", over="ignore"):
            psum[part] = np.sum(np.exp2(np.maximum(acc, EXP2S_CLAMP) * 0.00390625), axis=1)
        pmax[part] = acc.max(axis=1)
    return psum, pmax


def _log_norm(L):
    half = 0.0
    for k in range(L.shape[0]):
        half += math.log(L[k, k] * math.sqrt(2.0 * math.pi))
    return -half


def _norm(L):
    d = L.shape[0]
    norm = math.pow(2.0 * math.pi, -0.5 * d)
    for k in range(d):
        norm /= L[k, k]
    return norm


def evaluate(X, logw, L, Q, log_out, defect=None):
    """logpdf[M] (log_out) or pdf[M] as kde_run computes them: first pass, combine (mode 0 or 1), and for logpdf the shifted pass
    over the flagged queries and the second combine (mode 2)."""
    L = np.ascontiguousarray(L, dtype=np.float64)
    d = L.shape[0]
    Sa, c = prepare_samples(X, logw, L, defect)
    Qa = prepare_queries(Q, c, L)
    M = Qa.shape[0]
    parts, pts = kde_plan(Sa.shape[1], M, Sa.shape[0])
    psum, pmax = partial(Sa, Qa, parts, pts, d, defect)
    s = np.zeros(M)
    for k in range(parts):
        s = s + psum[k]
    if not log_out:
        return s * _norm(L)                                                   # mode 0
    log_norm = _log_norm(L)
    w = pmax[0] if defect == "first_part_max" else pmax.max(axis=0)           # mode 1
    tail = w * KDE_LN2_256 < KDE_TAIL
    shift = np.where(tail, w, 0.0)
    with np.errstate(divide="ignore"):
        out = np.log(s) + log_norm
    if np.any(tail):
        Qt = Qa[tail].copy()
        Qt[:, d + 1] -= shift[tail]
        ps2, _ = partial(Sa, Qt, parts, pts, d, defect)
        s2 = np.zeros(Qt.shape[0])
        for k in range(parts):
            s2 = s2 + ps2[k]
        with np.errstate(divide="ignore", over="ignore"):
            if defect == "no_shift_back":
                out[tail] = np.log(s2) + log_norm
            elif defect == "shift_f32":
                out[tail] = (np.log(s2) + log_norm) + shift[tail].astype(np.float32).astype(np.float64) * KDE_LN2_256
            else:
                out[tail] = np.log(s2) + (shift[tail] * KDE_LN2_256 + log_norm)   # the device's fma: one rounding fewer
    return out


def logpdf(X, logw, L, Q, defect=None):
    return evaluate(X, logw, L, Q, True, defect)


def pdf(X, logw, L, Q, defect=None):
    return evaluate(X, logw, L, Q, False, defect)
