"""fp64 statement of the NUTS warm-up (``EnsembleSampler.tune_nuts`` / ``find_step_size``, ``alabi_ens_nuts_adapt`` /
``alabi_ens_find_step_size``): the CPU statement that ens_nuts_adapt_kernel and ens_step_search_kernel
(alabi_amd/csrc/ens_nuts_adapt.hip) and the host side in alabi_amd/sampler.py are tested against.  Built on tests/nuts_numpy.py (the
transition, the draws), tests/hmc_adapt_numpy.py (the dual-averaging update, the schedule, the shrinkage) and tests/hmc_numpy.py
(targets, Philox helpers), which it imports and leaves as they are.  Plain NumPy; nothing of alabi_amd is imported.

A warm-up transition of walker w with the state (m, H-bar, ln e, ln e-bar, mu) is nuts_numpy.transition with e_w = exp(ln e_w) f, f
the step's jitter factor (e_table / p0: 1 without jitter).  With leaves_t >= 1 the leaves it made and a the per-leaf statistic
(min(1, exp(delta)) in the open box, 0 outside, 0 for the divergent leaf, which counts as a leaf)

    a_t = (sum of a over these leaves, summed from 0 in the order the leaves were made) / leaves_t

and the state takes hmc_adapt_numpy.da_update with a_t.

The step-size search (Stan's find_reasonable heuristic) of walker x with lp = the caller's logp, g = grad lnp(x), from ln e:
iteration i = 0, 1, ...: z ~ N(0, I) fresh (Philox counter (step, global walker id, 11 + 16 (64 (i + 1) + k)) for coordinate k);
H0 = -lp + |z|^2 / 2; one leaf with e = exp(ln e); dH = H0 - (-lp_q + |z|^2 / 2), -inf for NaN or an end point outside the open box;
iteration 0 fixes dir = +1 if dH > ln 0.8 else -1; the loop ends at the first iteration where dir = +1 and not dH > ln 0.8, or
dir = -1 and not dH < ln 0.8; otherwise ln e += dir ln 2; 40 such steps at the most.  iters = the steps taken (40: the cap).  Every
comparison's margin |dH - ln 0.8| is recorded in ``rec["search"]``; the walker does not move and no global step is consumed.

The warm-up (``warmup``) mirrors hmc_adapt_numpy.warmup; with ``search`` the search runs before the first segment and after every
mass-matrix update (but the last segment's), each walker restarting from its own value (m = 0, H-bar = 0, ln e = ln e-bar = ln e_w,
mu = ln 10 + ln e_w).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import hmc_adapt_numpy as han
import hmc_numpy as hm
import nuts_numpy as nn
from hmc_adapt_numpy import da_update    # the update is stated once, there

wk = hm.wk
LN_TARGET = float(np.log(0.8))
LN2 = float(np.log(2.0))
SEARCH_CAP = 40
DEFAULT_PAR = han.DEFAULT_PAR
M, HBAR, LN_E, LN_EBAR, MU = han.M, han.HBAR, han.LN_E, han.LN_EBAR, han.MU


def searched_state(ln_e):
    v = np.asarray(ln_e, dtype=np.float64)
    st = np.zeros((len(v), 5))
    st[:, LN_E] = st[:, LN_EBAR] = v
    st[:, MU] = np.log(10.0) + v
    return st


# ------------------------------------------------------------------------------------------------------- one transition
def adapt_step_arrays(target, coords, logp, grad, C, e, z0, dirw, u_leaf, u_tree, max_depth, state, par, rec=None):
    """One warm-up transition of every walker, e [W] its step sizes: nuts_numpy's transition, a_t and the state's update.
    Returns coords, logp, grad, trace [W, 4], a_sum [W] (over the leaves), a_t [W], state."""
    W = len(coords)
    out_c, out_lp, out_g = np.array(coords, copy=True), np.array(logp, copy=True), np.array(grad, copy=True)
    trace, a_sum = np.zeros((W, 4), dtype=np.int64), np.zeros(W)
    for w in range(W):
        out_c[w], out_lp[w], out_g[w], trace[w], a_sum[w] = nn.transition(target, coords[w], float(logp[w]), grad[w], C, float(e[w]), z0[w],
                                                                           dirw[w], u_leaf[w], u_tree[w], max_depth, rec=rec)
    a_t = a_sum / trace[:, 1]
    return out_c, out_lp, out_g, trace, a_sum, a_t, da_update(state, a_t, par)


def run_nuts_adapt(target, p0, nsteps, seed, move, par, state, step0=0, logp0=None, id0=0, nwalkers=None, rec=None, trace=None):
    """``nsteps`` warm-up transitions with the production draws (``nn.draw_nuts_randoms``).  ``move`` = (cov, step size, max_depth,
    jitter or None, weight), one move; its step size is the table's p0, of which only the jitter factor e_table / p0 is used.
    ``p0`` [E W, d] holds E ensembles of ``nwalkers`` walkers, global walker ids from ``id0``.  ``trace`` (a list): per transition
    (coords, logp, state before it).  Returns chain, chain_logp, nacc, coords, logp, state, alpha [nsteps, E W] (a_t), diverged
    [nsteps, E W] (the transition ended in a divergent leaf), counts [E W, 3] (leaves, depths, divergent), a_sum [E W] (over all
    leaves, transition by transition as the device's running sum)."""
    coords = np.array(p0, dtype=np.float64, copy=True)
    n, d = coords.shape
    W = n if nwalkers is None else int(nwalkers)
    assert n % W == 0
    _, cum, tp0, tp1, scales = nn.move_table([move], d)
    C, D = scales[0][0], int(np.floor(tp1[0]))
    logp = han.gated(target, coords) if logp0 is None else np.array(logp0, dtype=np.float64)
    grad = target.value_grad(coords)[1]
    state = np.array(state, dtype=np.float64, copy=True)
    chain, chain_lp, alphas = np.empty((nsteps, n, d)), np.empty((nsteps, n)), np.empty((nsteps, n))
    nacc, counts, a_run = np.zeros(n, dtype=np.int64), np.zeros((n, 3), dtype=np.int64), np.zeros(n)
    diverged = np.zeros((nsteps, n), dtype=bool)
    for t in range(nsteps):
        f, z0, dirw = np.empty(n), np.empty((n, d)), np.empty(n, dtype=np.uint32)
        u_leaf, u_tree = np.empty((n, (1 << D) - 1)), np.empty((n, D))
        for k in range(n // W):
            g0, sl = int(id0) + k * W, slice(k * W, (k + 1) * W)
            _, e_table, z0[sl], dirw[sl], u_leaf[sl], u_tree[sl] = nn.draw_nuts_randoms(seed, step0 + t, np.arange(W) + g0, g0, cum, tp0, tp1, d)
            f[sl] = e_table / tp0[0]
        if trace is not None:
            trace.append((coords, logp, state))
        coords, logp, grad, tr, a_sum, alphas[t], state = adapt_step_arrays(target, coords, logp, grad, C, np.exp(state[:, LN_E]) * f, z0,
                                                                            dirw, u_leaf, u_tree, D, state, par, rec)
        nacc += tr[:, 3]
        counts[:, 0] += tr[:, 1]; counts[:, 1] += tr[:, 0]; counts[:, 2] += tr[:, 2] == nn.STOP_DIVERGENT
        diverged[t] = tr[:, 2] == nn.STOP_DIVERGENT
        # the device adds leaf by leaf to ONE running sum; adding the transition's own sum differs from that in the last bits only
        a_run += a_sum
        chain[t], chain_lp[t] = coords, logp
    return SimpleNamespace(chain=chain, chain_logp=chain_lp, nacc=nacc, coords=coords, logp=logp, state=state, alpha=alphas,
                           counts=counts, a_sum=a_run, diverged=diverged)


# ------------------------------------------------------------------------------------------------------------ the search
def search_normals(seed, step, gids, i, d):
    """The momentum normals of iteration i for the walkers ``gids``: stream 11 beyond the words the moves read."""
    return wk._normal(wk._philox(seed, step, np.asarray(gids), hm.STREAM_HMC_Z + 16 * (64 * (i + 1) + np.arange(d))))


def search_dh(target, x, lp, g, C, e, z):
    """dH of one leaf from (x, z) with the step size e: NaN and an end point outside the open box count as -inf."""
    lo, hi = target.bounds[:, 0], target.bounds[:, 1]
    with np.errstate(all="ignore"):
        H0 = -lp + 0.5 * float(z @ z)
        z = z + (0.5 * e) * (g @ C)
        q = x + e * (C @ z)
        lv, gv, _ = target.value_grad(q[None, :])
        z = z + (0.5 * e) * (gv[0] @ C)
        dH = H0 - (-float(lv[0]) + 0.5 * float(z @ z))
    if np.isnan(dH) or not bool(np.all((q > lo) & (q < hi))):
        dH = -np.inf
    return dH


def find_step_size(target, coords, logp, C, ln_e, seed, step, id0=0, rec=None):
    """The search of every walker (global ids id0 ...) from ln_e [n]; returns (ln_e [n], iters [n])."""
    coords = np.asarray(coords, dtype=np.float64)
    n, d = coords.shape
    grad = target.value_grad(coords)[1]
    out, iters = np.array(ln_e, dtype=np.float64, copy=True), np.zeros(n, dtype=np.int32)
    for w in range(n):
        le, i, direction = float(out[w]), 0, 0
        while True:
            z = search_normals(seed, step, [int(id0) + w], i, d)[0]
            dH = search_dh(target, coords[w], float(logp[w]), grad[w], C, float(np.exp(le)), z)
            if rec is not None:
                rec.setdefault("search", []).append(abs(dH - LN_TARGET))
            if i == 0:
                direction = 1 if dH > LN_TARGET else -1
            if (direction > 0 and not dH > LN_TARGET) or (direction < 0 and not dH < LN_TARGET):
                break
            le += LN2 if direction > 0 else -LN2
            i += 1
            if i == SEARCH_CAP:
                break
        out[w], iters[w] = le, i
    return out, iters


def honesty(rec, min_margin):
    """nuts_numpy.honesty plus every search comparison's |dH - ln 0.8| > min_margin."""
    out = nn.honesty(rec, min_margin)
    s = np.asarray(rec.get("search", [np.inf]), dtype=np.float64)
    out["min_search"] = float(s.min())
    out["ok"] = bool(out["ok"] and out["min_search"] > min_margin)
    return out


# ------------------------------------------------------------------------------------------------------ the whole warm-up
def warmup(target, p0, nwarmup, seed, move, par=DEFAULT_PAR, metric="diag", nwalkers=None, step0=0, search=True):
    """The whole warm-up from ``p0`` [E W, d]; ``move`` as for ``run_nuts_adapt``.  Returns step_size, cov (None: not adapted),
    window_ends, step_sizes, mean_accept_stat, mean_depth and divergences (of the last segment), search_iters, coords, logp, state
    and move, the tuned move."""
    cov, eps0, D, jitter, _ = move
    coords = np.array(p0, dtype=np.float64, copy=True)
    n, d = coords.shape
    W = n if nwalkers is None else int(nwalkers)
    logp = han.gated(target, coords)
    search_iters = []

    def searched(eps, cov_now, step):
        C = hm.gm.scale_factor(cov_now, d)[0]
        ln_e, it = np.empty(n), np.empty(n, dtype=np.int32)
        for k in range(n // W):
            sl = slice(k * W, (k + 1) * W)
            ln_e[sl], it[sl] = find_step_size(target, coords[sl], logp[sl], C, np.full(W, np.log(eps)), seed, step, id0=k * W)
        search_iters.append(it)
        return searched_state(ln_e)

    state = searched(eps0, cov, step0) if search else han.initial_state(n, eps0)
    init, ends = han.schedule(nwarmup)
    if metric is None or not ends:
        segs = [(0, nwarmup, False)]
    else:
        segs = [(0, init, False)] + [(a, b, True) for a, b in zip([init] + ends[:-1], ends)] + [(ends[-1], nwarmup, False)]
        segs = [s for s in segs if s[1] > s[0]]
    new_cov, step_sizes, window_ends, r = None, [], [], None
    for k, (first, end, is_window) in enumerate(segs):
        r = run_nuts_adapt(target, coords, end - first, seed, (cov, eps0, D, jitter, 1.0), par, state, step0=step0 + first, logp0=logp,
                           nwalkers=nwalkers)
        coords, logp, state = r.coords, r.logp, r.state
        if is_window:
            cov = new_cov = han.shrunk_covariance(r.chain.reshape(-1, d), metric)
            pooled = float(np.exp(np.mean(state[:, LN_EBAR])))
            step_sizes.append(pooled); window_ends.append(end)
            if k < len(segs) - 1:
                state = searched(pooled, cov, step0 + end) if search else han.restart_state(n, pooled)
    eps = float(np.exp(np.mean(state[:, LN_EBAR])))
    n_last = segs[-1][1] - segs[-1][0]
    return SimpleNamespace(step_size=eps, cov=new_cov, window_ends=window_ends, step_sizes=step_sizes,
                           mean_accept_stat=float(np.mean(r.alpha)), mean_depth=float(r.counts[:, 1].sum()) / (n_last * n),
                           divergences=int(r.counts[:, 2].sum()), search_iters=search_iters, coords=coords, logp=logp, state=state,
                           move=(cov, eps, D, jitter, 1.0))
