"""fp64 statement of the device optimiser behind ``EnsembleSampler.maximize`` (ens_map_kernel, alabi_amd/csrc/ens_map.hip): the
specification the kernel follows and is tested against.  Plain NumPy, no fma emulation: the device's sums run in another order, so
the log-probability is compared to a tolerance and only the discrete decisions (step length, held set, update flag) exactly --
which is why tests/test_map_host.py shows that no traced decision is a near tie.

Projected BFGS ascent of the fused log-probability WITHOUT the box gate (value and gradient: ``target.value_grad``, the contract
of lp_grad_eval) on the shrunk box [lo + 1e-9 w, hi - 1e-9 w], w = hi - lo.  With x the point, f = lnp(x), g its gradient and B
the dense approximation of the inverse of -Hessian:

    start      outside the OPEN box [lo, hi], or f or g not finite: status 3, every output NaN.  Otherwise x = clip(x0).
    held       coordinate k is held when it sits on a face of the shrunk box and the gradient points outward:
               (x_k <= lo'_k and g_k < 0) or (x_k >= hi'_k and g_k > 0).  pg = g with the held coordinates zeroed.
    stop       max|pg| <= gtol: status 0.  Then: ``maxiter`` steps taken: status 1.
    reset      B = diag(0.1 w_k / max|pg|): the first trial moves no coordinate by more than a tenth of the box.  B is reset at the
               start, when the held set changes, when p is no ascent direction, and for the second attempt of a failed search.
    direction  p = B pg on the free coordinates, 0 on the held ones; an ascent direction iff pg . p > 0.
    search     t = 1, 1/2, 1/4, ... (at most 30 trials): xn = clip(x + t p), step = xn - x, dd = g . step.  The trial is
               accepted when fn >= f + 1e-4 dd (Armijo on the projected step).  Where the values cannot tell -- |fn - f| <=
               1e-8 max(1, |f|), the last steps of a converging run, whose gain is of the size of the rounding of f -- the
               gradient decides instead: accepted when the slope along the step has not turned round by more than it was,
               gn . step >= -(1 - 2e-4) dd.  On a parabola that IS Armijo's condition (f(1) - f(0) = (dd + gn . step) / 2; the
               approximate Wolfe condition of Hager & Zhang 2005).  Their curvature condition is left out: a backtracking search
               cannot lengthen a step that is too short, and such a step still ascends.  A search ends without a step when no
               coordinate moves or after the 30th trial; it is repeated once with B reset unless B was fresh already; then
               status 2 and the point is kept.
    update     s = step, y = g - gn on the free coordinates (0 on the held ones); applied only when s.y > 1e-10 |s| |y|:
               a fresh B becomes (s.y / y.y) I first, then B <- B - rho (s (By)^T + (By) s^T) + rho (1 + rho y.By) s s^T,
               rho = 1 / s.y.  s, y and rho are temporaries: nothing of B is written when the update is refused.
    result     never worse than the clipped start: if f ended below it (possible only through the approximate Wolfe branch, by
               1e-8 relative per step at the most) the start is returned.

Differences from scipy's L-BFGS-B: dense BFGS instead of the limited-memory compact form; the active set is the held set of the
current point instead of the generalised Cauchy point and subspace minimisation; plain backtracking instead of the More-Thuente
search; no factr stop.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

ARMIJO, FLAT, CURV, SHRINK, FIRST, LS_MAX = 1e-4, 1e-8, 1e-10, 1e-9, 0.1, 30
CONVERGED, MAXITER, NO_ASCENT, BAD_START = 0, 1, 2, 3


def shrunk_box(bounds):
    lo, hi = bounds[:, 0], bounds[:, 1]
    w = hi - lo
    return lo + SHRINK * w, hi - SHRINK * w, w


def held_mask_int(held):
    return int(sum(1 << int(k) for k in np.nonzero(held)[0]))


def maximize_one(target, x0, bounds, maxiter=200, gtol=1e-8, ntrace=0):
    """One start.  Returns x, lp, iterations, evaluations, status, grad_norm, held (bool [d]), trace [(lp, t, held mask, updated)]
    of the first ``ntrace`` iterations (``trace_x``: the points; ``trace_flat``: whether the gradient decided the step) and
    ``margins``: the smallest distance of a traced decision from its threshold (armijo,
    flat: relative to max(1, |f|); wolfe: relative to |dd|; curv: of s.y / |s||y| from 1e-10; wall: |g_k| / max|g| of a coordinate
    on a face; gtol: of max|pg| from gtol, relative to gtol)."""
    bounds = np.asarray(bounds, dtype=np.float64)
    d = len(bounds)
    lo, hi = bounds[:, 0], bounds[:, 1]
    los, his, w = shrunk_box(bounds)
    x0 = np.asarray(x0, dtype=np.float64)
    nan = SimpleNamespace(x=np.full(d, np.nan), lp=np.nan, iterations=0, evaluations=0, status=BAD_START, grad_norm=np.nan,
                          held=np.zeros(d, bool), trace=[], trace_x=[], trace_flat=[], margins={})
    if not np.all((x0 > lo) & (x0 < hi)):
        return nan
    nev = [0]

    def ev(q):
        nev[0] += 1
        with np.errstate(all="ignore"):
            L, g, _ = target.value_grad(q[None, :])
        return float(L[0]), np.asarray(g[0], dtype=np.float64)

    x = np.minimum(np.maximum(x0, los), his)
    f, g = ev(x)
    if not (np.isfinite(f) and np.all(np.isfinite(g))):
        nan.evaluations = 1
        return nan
    x_start, f_start = x.copy(), f
    margins = dict(armijo=np.inf, flat=np.inf, wolfe=np.inf, curv=np.inf, wall=np.inf, gtol=np.inf)
    trace, trace_x, trace_flat, B, fresh, prev, it = [], [], [], None, True, None, 0
    while True:
        on_wall = (x <= los) | (x >= his)
        held = ((x <= los) & (g < 0.0)) | ((x >= his) & (g > 0.0))
        pg = np.where(held, 0.0, g)
        gnorm = float(np.max(np.abs(pg)))
        if it < ntrace and on_wall.any():
            margins["wall"] = min(margins["wall"], float(np.min(np.abs(g[on_wall])) / np.max(np.abs(g))))
        if it <= ntrace and ntrace:
            margins["gtol"] = min(margins["gtol"], abs(gnorm - gtol) / gtol)
        if gnorm <= gtol:
            status = CONVERGED
            break
        if it >= maxiter:
            status = MAXITER
            break
        if prev is not None and np.any(held != prev):
            fresh = True
        prev = held
        accepted = False
        for attempt in range(2):
            if attempt == 1:
                if fresh:
                    break
                fresh = True
            if fresh:
                B = np.diag(FIRST * w / gnorm)
            p = np.where(held, 0.0, B @ pg)
            if not float(pg @ p) > 0.0:
                B = np.diag(FIRST * w / gnorm)
                fresh = True
                p = np.where(held, 0.0, B @ pg)
            t = 1.0
            for _ in range(LS_MAX):
                xn = np.where(held, x, np.minimum(np.maximum(x + t * p, los), his))
                step = xn - x
                if float(np.max(np.abs(step))) == 0.0:
                    break
                dd = float(g @ step)
                fn, gn = ev(xn)
                ok = False
                if np.isfinite(fn) and np.all(np.isfinite(gn)):
                    scale = max(1.0, abs(f))
                    flat = abs(fn - f) <= FLAT * scale
                    dn = float(gn @ step)
                    ok = (dn >= -(1.0 - 2.0 * ARMIJO) * dd) if flat else (fn >= f + ARMIJO * dd)
                    if it < ntrace:
                        margins["flat"] = min(margins["flat"], abs(abs(fn - f) - FLAT * scale) / scale)
                        if flat:
                            margins["wolfe"] = min(margins["wolfe"], abs(dn + (1.0 - 2.0 * ARMIJO) * dd) / abs(dd))
                        else:
                            margins["armijo"] = min(margins["armijo"], abs(fn - f - ARMIJO * dd) / scale)
                if ok:
                    accepted = True
                    break
                t *= 0.5
            if accepted:
                break
        if not accepted:
            status = NO_ASCENT
            break
        s = step
        y = np.where(held, 0.0, g - gn)
        sy, ss, yy = float(s @ y), float(s @ s), float(y @ y)
        lim = CURV * np.sqrt(ss * yy)
        updated = sy > lim
        if it < ntrace and ss * yy > 0.0:
            margins["curv"] = min(margins["curv"], abs(sy / np.sqrt(ss * yy) - CURV))
        if updated:
            if fresh:
                B = np.eye(d) * (sy / yy)
                fresh = False
            rho = 1.0 / sy
            By = B @ y
            c = rho * (1.0 + rho * float(y @ By))
            B = B - rho * (np.outer(s, By) + np.outer(By, s)) + c * np.outer(s, s)
        x, f, g = xn, fn, gn
        if it < ntrace:
            trace.append((f, t, held_mask_int(held), bool(updated)))
            trace_x.append(x.copy())
            trace_flat.append(bool(flat))
        it += 1
    if f < f_start:
        x, f = x_start, f_start
    return SimpleNamespace(x=x, lp=f, iterations=it, evaluations=nev[0], status=status, grad_norm=gnorm, held=held, trace=trace,
                           trace_x=trace_x, trace_flat=trace_flat, margins=margins)


def maximize(target, starts, bounds, maxiter=200, gtol=1e-8, ntrace=0):
    """Every start on its own, as the device runs one workgroup per start."""
    return [maximize_one(target, s, bounds, maxiter, gtol, ntrace) for s in np.atleast_2d(starts)]
