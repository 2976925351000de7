"""Named cases for the Gaussian KDE against its truth (tests/kde_reference.py), shared by tests/test_kde_reference_host.py and
tests/test_gpu_kde_truth.py.  Small shapes only: the truth costs N M d extended operations, at most 2e7 here.

Dimensions: every KS = rows / 4 of kde_partial_kernel once and every boundary (d = 2, 6, 14, 30, 34, 62: rows == d + 2, no zero
rows; 30 | 31: four query tiles per wavefront | two; 63, 64 share KS = 17).  Sample counts: d + 2 (one part, ill-conditioned L),
256 (two parts of 128, no padding samples), 2065 (Npad 2080: 15 parts of 144, the last one 64 samples).  Query counts around the
wave (16 QT) and workgroup (64 QT) sizes of both QT.  TABLE names the pairs.

Queries: the mixture of tests/test_gpu_metrics.py (half within a bandwidth of a sample, half uniform over the data's box).  Cases
with three whole waves of queries carry a ladder: wave 0 sits within half a whitened unit of samples (none flagged), wave 1 climbs
a ray out of the outermost sample with the largest exponent stepping from about -400 to -900 (flagged and unflagged together),
wave 2 goes on from -1100 to -3000 (all flagged).  ``reference`` asserts this from the truth's exponents.

Weights: none | uniform(0.05, 1) | "decades": uniform, but eight samples carry 1e-286 .. 1e-300 and the two lightest sit 70 and
80 whitened units from the centre; the last eight queries sit ON those eight samples (own log w below -650: dominated from afar
for the six inside the data, by their own term for the two outside) | "zeros": uniform with five exact zeros, among them the
sample nearest to query 0 | "bimodal": the first 144 samples (part 0 of the split) are a light cluster 100 units from the rest.
Offsets: +1e4 with every input on a 2^-30 grid (d = 2 and 34)."""
from __future__ import annotations

import functools
import math

import numpy as np

import kde_numpy
import kde_reference as kr

GRID = 2.0 ** -30

# name -> (d, N ("d+2" or a count), M, weights, offset)
_T = {
    1: [("d+2", 1, None), (256, 257, "uniform"), (2065, 64, "decades")],
    2: [("d+2", 63, "uniform"), (256, 65, None), (2065, 257, "zeros")],
    3: [("d+2", 64, None), (2065, 257, "uniform")],
    6: [("d+2", 65, None), (256, 1, "uniform"), (2065, 63, "decades")],
    10: [("d+2", 257, "uniform"), (2065, 65, None)],
    14: [("d+2", 63, "uniform"), (256, 257, "zeros")],
    18: [("d+2", 1, None), (2065, 64, "uniform")],
    22: [(256, 65, "decades"), (2065, 257, None)],
    26: [("d+2", 257, "uniform"), (256, 63, None)],
    29: [("d+2", 64, None), (2065, 65, "zeros")],
    30: [("d+2", 63, None), (256, 64, "uniform"), (2065, 257, "decades")],
    31: [("d+2", 33, None), (256, 32, "uniform"), (2065, 129, "decades")],
    34: [("d+2", 31, "uniform"), (2065, 128, None)],
    38: [("d+2", 1, None), (256, 127, "zeros")],
    42: [("d+2", 129, "uniform"), (2065, 33, "uniform")],
    46: [("d+2", 32, "uniform"), (256, 128, None)],
    50: [("d+2", 31, None), (2065, 127, "uniform")],
    54: [("d+2", 33, None), (256, 129, "decades")],
    58: [("d+2", 128, "uniform"), (2065, 1, None)],
    62: [("d+2", 127, None), (256, 31, "uniform"), (2065, 129, "zeros")],
    63: [("d+2", 129, "uniform"), (2065, 32, None)],
    64: [("d+2", 128, None), (256, 33, "zeros"), (2065, 127, "uniform")],
}
DIMS = tuple(_T)
TABLE = {}
for _d, _rows in _T.items():
    for _n, _m, _w in _rows:
        _N = _d + 2 if _n == "d+2" else _n
        TABLE[f"d{_d}-n{_N}-m{_m}-{_w or 'plain'}"] = (_d, _N, _m, _w, False)
TABLE["d2-n2065-m64-plain-offset"] = (2, 2065, 64, None, True)
TABLE["d34-n2065-m32-plain-offset"] = (34, 2065, 32, None, True)
TABLE["d2-n2065-m64-bimodal"] = (2, 2065, 64, "bimodal", False)
NAMES = tuple(TABLE)
OFFSET_CASES = tuple(n for n in NAMES if TABLE[n][4])

# Criterion 2 of tests/test_gpu_kde_truth.py: rms error of the device <= MARGIN x rms error of kde_numpy, per case.  Twice the
# largest ratio measured on the MI355X, rounded up (NOTES.md "Gaussian KDE and metrics" has the table); never above 10.
MARGIN = 4                                   # largest measured: 1.89 (d64-n256-m33-zeros); 49 cases between 0.24 and 1.89
# Excepted from criterion 2 by name: the cases with ONE query.  The rms over one query is a single draw from the error's
# distribution, for the device and for the restatement alike, and the ratio of two single draws has no bound worth the name: on the
# MI355X d38-n40-m1-plain gave 38.5 because kde_numpy happened to land 5.7e-5 of the bound from the truth there (the device's
# 0.0022 of the bound is what every neighbouring case shows).  Criterion 1 holds for them like for every other case.
CRITERION_2_EXCEPT = tuple(n for n in NAMES if TABLE[n][2] == 1)
assert CRITERION_2_EXCEPT == ("d1-n3-m1-plain", "d6-n256-m1-uniform", "d18-n20-m1-plain", "d38-n40-m1-plain", "d58-n2065-m1-plain")
SEED = 0
UNDERFLOW_LOG = -1074 * math.log(2.0)


def shape(name):
    """d -> rows -> KS, QT, and the plan: what the case exercises."""
    d, N, M, _, _ = TABLE[name]
    rows = kde_numpy.kde_rows(d)
    Npad = (N + 15) // 16 * 16
    parts, pts = kde_numpy.kde_plan(Npad, M, rows)
    return dict(d=d, N=N, M=M, rows=rows, KS=rows // 4, QT=kde_numpy.kde_qt(rows), Npad=Npad, parts=parts, pts=pts)


def _data(rng, d, n):
    A = rng.normal(size=(d, d)) / np.sqrt(d) + np.eye(d)
    return (A @ rng.normal(size=(d, n)) + rng.normal(size=(d, 1))).T


def _mixture(rng, X, m, h):
    """Half near samples (within a bandwidth), half uniform over the data's box (tests/test_gpu_metrics.py::_queries)."""
    n, d = X.shape
    near = X[rng.integers(0, n, m)] + h[None, :] * rng.normal(size=(m, d))
    lo, hi = X.min(0), X.max(0)
    box = lo + (hi - lo) * rng.uniform(size=(m, d))
    return np.where((rng.uniform(size=m) < 0.5)[:, None], near, box)


def _bandwidth(X, weights):
    """(logw [N] or None, cho_cov) as DeviceKDE forms them on the host (alabi_amd/kde.py; bit-equal to scipy's, which
    tests/test_metrics_host.py asserts): the fp64 inputs of the truth."""
    from alabi_amd.kde import kde_bandwidth, kde_factor, kde_weights
    N, d = X.shape
    wn, neff = kde_weights(weights, N)

    class _K:
        pass
    k = _K()
    k.d, k.n, k.neff = d, N, neff
    _, cho, _ = kde_bandwidth(np.cov(X.T, rowvar=1, bias=False, aweights=wn), kde_factor(None, k))
    if weights is None:
        return None, np.ascontiguousarray(cho)
    with np.errstate(divide="ignore"):
        return np.log(wn), np.ascontiguousarray(cho)


@functools.lru_cache(maxsize=None)
def build(name):
    """dict(X [N, d], weights [N] or None, logw, L (the library's), Q [M, d], wave, ladder (three whole waves lead Q),
    on_sample (query, sample) pairs)."""
    d, N, M, kind, offset = TABLE[name]
    rng = np.random.default_rng(SEED + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    X = _data(rng, d, N)
    if offset:
        X = np.round(X / GRID) * GRID
    w, on_sample, s0 = None, (), None
    if kind in ("uniform", "decades", "zeros"):
        w = rng.uniform(0.05, 1.0, N)
    if kind == "bimodal":
        X[:144] = 0.05 * rng.normal(size=(144, d)) + np.r_[-100.0, np.zeros(d - 1)]
        w = np.r_[np.full(144, 1e-3), np.ones(N - 144)]
    if kind == "decades":
        light = rng.choice(N, 8, replace=False)
        w[light] = 10.0 ** (-300.0 + 2.0 * np.arange(8)[::-1])            # 1e-286 .. 1e-300: every log w below -650
        Lu = np.linalg.cholesky(np.atleast_2d(np.cov(X.T)) * N ** (-2.0 / (d + 4)))
        for i, r in ((6, 70.0), (7, 80.0)):                               # too light to move the weighted covariance
            u = rng.normal(size=d)
            X[light[i]] = X.mean(0) + Lu @ (r * u / np.linalg.norm(u))
    if kind == "zeros":
        zero = rng.choice(N, 5, replace=False)
        w[zero] = 0.0
        s0 = int(zero[0])
    logw, L = _bandwidth(X + 1e4 if offset else X, w)
    body = X[w > 1e-200] if kind == "decades" else X
    Q = _mixture(rng, body, M, np.sqrt(np.sum(L * L, axis=1)))          # sqrt(diag(covariance)), covariance = L L^T
    wave = 16 * kde_numpy.kde_qt(kde_numpy.kde_rows(d))
    ladder = M >= 3 * wave
    if ladder:
        Q[:wave] = X[rng.integers(0, N, wave)] + 0.5 / math.sqrt(d) * (rng.normal(size=(wave, d)) @ L.T)
        z = np.linalg.solve(L, (body - body.mean(0)).T).T
        j = int(np.argmax(np.sum(z * z, axis=1)))
        v = L @ (z[j] / np.linalg.norm(z[j]))
        t = np.r_[np.sqrt(2.0 * np.linspace(400.0, 900.0, wave)), np.sqrt(2.0 * np.linspace(1100.0, 3000.0, wave))]
        Q[wave:3 * wave] = body[j][None, :] + t[:, None] * v[None, :]
    if kind == "decades":
        qi = np.arange(M - 8, M)
        Q[qi] = X[light]
        on_sample = tuple(zip(qi.tolist(), light.tolist()))
    if kind == "zeros":                                                   # query 0 sits 0.01 whitened units from a weightless sample
        u = rng.normal(size=d)
        Q[0] = X[s0] + L @ (0.01 * u / np.linalg.norm(u))
    if offset:
        Q = np.round(Q / GRID) * GRID
    # keep every density two binades clear of 2^-1074 (logpdf = -744.44), where "exactly 0" and "a denormal" meet: a query that
    # lands there moves 2 % further from the centre until it does not (fp64 is ample to decide this)
    centre = body.mean(0)
    for _ in range(40):
        near = np.abs(kde_numpy.logpdf(X, logw, L, Q) - UNDERFLOW_LOG) < 3.0
        if not np.any(near):
            break
        Q[near] = centre + 1.02 * (Q[near] - centre)
        if offset:
            Q = np.round(Q / GRID) * GRID
    if offset:
        X = X + 1e4
        Q = Q + 1e4
    for a in (X, Q):
        a.setflags(write=False)
    return dict(X=X, weights=w, logw=logw, L=L, Q=Q, wave=wave, ladder=ladder, on_sample=on_sample, zero_nearest=s0)


def bandwidth(name):
    c = build(name)
    return c["logw"], c["L"]


def logw_array(logw, N):
    """The truth's log w: the class's array, or fl(-log N) for every sample when unweighted (alabi_kde_set_data's logw_const)."""
    return np.full(N, -math.log(float(N))) if logw is None else logw


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything both test files need, computed once and left unchanged: the truth, the bounds, the restatement and its errors."""
    c = build(name)
    X, Q = c["X"], c["Q"]
    logw, L = bandwidth(name)
    lw = logw_array(logw, X.shape[0])
    tr = kr.truth(X, lw, L, Q)
    keep = tr.keep
    out = dict(c, logw=logw, lw=lw, L=L, truth=tr, keep=keep,
               tol_log=kr.tolerance_logpdf(X, lw, L, Q, tr), tol_pdf=kr.tolerance_pdf(X, lw, L, Q, tr),
               np_log=kde_numpy.logpdf(X, logw, L, Q), np_pdf=kde_numpy.pdf(X, logw, L, Q))
    out["np_err_log"] = np.abs((out["np_log"][keep].astype(kr.LD) - tr.logpdf).astype(np.float64))
    # the conditions the case table promises, from the truth's own exponents
    assert np.all(np.isfinite(tr.logpdf.astype(np.float64))), name
    edge = np.abs(tr.logpdf.astype(np.float64) - UNDERFLOW_LOG) < 2.0 * math.log(2.0)
    assert not np.any(edge), name                        # no truth within two binades of 2^-1074: "exactly 0" is unambiguous
    s = shape(name)
    if s["N"] == 2065:
        assert s["parts"] > 1 and s["parts"] * s["pts"] > s["Npad"], name
    if s["N"] == 256:
        assert (s["parts"], s["pts"]) == (2, 128) and s["Npad"] == 256, name
    if c["ladder"] and kr.QUERY_STRIDE == 1:
        wv = c["wave"]
        flagged = tr.mx.astype(np.float64) < kde_numpy.KDE_TAIL
        assert not np.any(flagged[:wv]), name
        assert np.any(flagged[wv:2 * wv]) and not np.all(flagged[wv:2 * wv]), name
        assert np.all(flagged[2 * wv:3 * wv]), name
    if c["on_sample"] and kr.QUERY_STRIDE == 1:
        own = [int(tr.arg[q]) == n for q, n in c["on_sample"]]
        assert all(lw[n] < kde_numpy.KDE_TAIL for _, n in c["on_sample"]), name
        assert own[-1] and (len(own) == 1 or not all(own)), name
    return out


def rms(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.sqrt(np.mean(x * x)))
