"""fp64 statement of the Gaussian Metropolis move (``alabi_amd.moves.GaussianMove``, kind 5 of the library's move table): the CPU
statement that ens_mh_kernel (alabi_amd/csrc/ens_mh.hip) and the Gaussian branch of the launch-per-half-step kernels
(alabi_amd/csrc/ensemble.hip: wk_proposal) are tested against.  Built on tests/walk_kde_numpy.py, tests/snooker_numpy.py,
tests/de_move_numpy.py and oracle/stretch_oracle.py, which it leaves as they are.

PARITY UNPINNED against emcee itself: emcee is not installed here.  The move is the one of emcee 3 ``moves/gaussian.py`` as the
project states it (DESIGN.md section 6 lists where emcee's source differs):

    q = x + f C z,   C C^T = cov,   z standard normal,   log factor 0,   accept iff lnp(q) - lnp(x) > ln u'

``cov`` a scalar (C = sqrt(cov) I), a vector of variances (C = diag(sqrt(cov))) or a matrix (C its lower Cholesky factor).
``mode`` 0 "vector" moves every coordinate; 1 "random" one coordinate, drawn per walker and step; 2 "sequential" coordinate
t mod d with t the ABSOLUTE step index (step0 + local step), the same for all walkers.  A matrix allows mode 0 only.
``factor`` None: f = 1; otherwise f = exp(v), v ~ U(-ln factor, ln factor), ONE draw per step and ensemble.

Arithmetic, in this order (fma = one rounding):
    s_k = sum_{i <= k} C[k, i] z_i        i ascending, s = fma(C[k, i], z_i, s) from s = 0; a diagonal C has the single term
    q_k = fma(f, s_k, x_k)
    modes 1 and 2: only the chosen coordinate changes, the others are copied bit for bit.
NumPy has no fma: ``fma`` below is the emulation of Boldo & Melquiond (2008) -- exact product, two exact sums, one addition rounded
to odd, one rounded to nearest --, pinned to exact rational arithmetic in tests/test_gaussian_move_host.py.

A proposal reads no other walker, so the red-blue split does not matter: a full step is the rule applied to split 0 and then to
split 1 (what the launch-per-half-step kernels do), which is the rule applied to every walker (what ens_mh_kernel does).

Draws.  Philox counter (step, global walker id, stream word), word = S + 16 b; streams 0-8 are those of the other moves, untouched:
    S = 2, b = 0:   the accept uniform u' = u53(r0, r1), at the walker                       (as for every move)
    S = 3, b = 0:   the step's move, at the ensemble's walker 0                              (as for every move)
    S = 9, b = 0:   v = (2 u53(r0, r1) - 1) ln factor, at the ensemble's walker 0; not drawn when factor is None
    S = 9, b = 1:   the coordinate of mode 1, (r0 d) >> 32, at the walker
    S = 10, b = k:  z_k = sqrt(-2 ln(1 - u53(r0, r1))) cos(2 pi u53(r2, r3)), at the walker  (Box-Muller as stream 4)
"""
from __future__ import annotations

import numpy as np

import snooker_numpy as sn
import walk_kde_numpy as wk
from oracle.stretch_oracle import u53

STREAM_GAUSS, STREAM_GAUSS_Z = 9, 10
KIND_GAUSS = 5
MODES = {"vector": 0, "random": 1, "sequential": 2}
_S32 = np.uint64(32)
_SPLIT = 134217729.0       # 2^27 + 1 (Veltkamp)


# ------------------------------------------------------------------------------------------------------------------- fma
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ca = _SPLIT * a; ah = ca - (ca - a); al = a - ah
    cb = _SPLIT * b; bh = cb - (cb - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """round(a b + c) with one rounding, element-wise (finite values away from overflow and underflow)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, ul)
    vh, vl = _two_sum(uh, th)
    s, err = _two_sum(tl, vl)                               # tl + vl rounded to odd
    bits = np.array(s, dtype=np.float64, copy=True).view(np.int64)
    need = (err != 0.0) & ((bits & 1) == 0)
    away = (err > 0.0) == (s > 0.0)                         # the exact sum lies further from zero than s
    bits = np.where(need, np.where(away, bits + 1, bits - 1), bits)
    return vh + bits.view(np.float64)


# ------------------------------------------------------------------------------------------------------------- the table
def scale_factor(cov, d):
    """(C [d, d] lower triangular, diagonal) of a covariance given as a scalar, a vector of variances or a matrix."""
    c = np.asarray(cov, dtype=np.float64)
    if c.ndim == 2:
        assert c.shape == (d, d)
        return np.tril(np.linalg.cholesky(c)), False
    return np.diag(np.broadcast_to(np.sqrt(c), (d,)).astype(np.float64)), True


def move_table(moves, ndim, W):
    """walk_kde_numpy.move_table that also takes ("gauss", cov, mode, factor, w): kind 5, p0 = ln factor (0 for None), p1 = the
    mode's number.  Returns kinds, cum, p0, p1 and, per move, (C, diagonal) or None."""
    kinds, p0, p1, w, scales = [], [], [], [], []
    for m in moves:
        if m[0] == "gauss":
            kinds.append(KIND_GAUSS); p0.append(0.0 if m[3] is None else float(np.log(float(m[3])))); p1.append(float(MODES[m[2]]))
            scales.append(scale_factor(m[1], ndim))
        else:
            k, _, a, b = wk.move_table([m], ndim, W)
            kinds.append(int(k[0])); p0.append(float(a[0])); p1.append(float(b[0])); scales.append(None)
        w.append(float(m[-1]))
    w = np.asarray(w, dtype=np.float64)
    return np.asarray(kinds), np.cumsum(w / w.sum()), np.asarray(p0), np.asarray(p1), scales


# ------------------------------------------------------------------------------------------------------------- the draws
def draw_gauss_randoms(seed, step, gids, g0, ln_factor, mode, d):
    """The Gaussian move's draws of one step for the walkers ``gids`` (global ids) of the ensemble whose walker 0 is ``g0``:
    f (scalar), coord [n] int32 (-1: every coordinate) and z [n, d]."""
    gids = np.asarray(gids)
    f = 1.0
    if ln_factor != 0.0:
        r = wk._philox(seed, step, [int(g0)], [STREAM_GAUSS])[0, 0]
        f = float(np.exp((2.0 * u53(r[0], r[1]) - 1.0) * ln_factor))
    coord = np.full(len(gids), -1, dtype=np.int32)
    if mode == 1:
        r = wk._philox(seed, step, gids, [STREAM_GAUSS + 16])[:, 0, :]
        coord = ((r[:, 0].astype(np.uint64) * np.uint64(d)) >> _S32).astype(np.int32)
    elif mode == 2:
        coord[:] = int(step) % d
    z = wk._normal(wk._philox(seed, step, gids, STREAM_GAUSS_Z + 16 * np.arange(d)))
    return f, coord, z


# -------------------------------------------------------------------------------------------------------------- the rule
def gaussian_proposal(x, C, f, coord, z, diagonal=None):
    """q [n, d] for the walkers x [n, d]: the stated arithmetic.  ``coord`` [n]: the coordinate that moves, -1 for all."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    C = np.asarray(C, dtype=np.float64)
    if diagonal is None:
        diagonal = not np.any(C - np.diag(np.diag(C)))
    s = np.zeros((n, d))
    for k in range(d):
        if diagonal:
            s[:, k] = fma(C[k, k], z[:, k], 0.0)
        else:
            acc = np.zeros(n)
            for i in range(k + 1):
                acc = fma(C[k, i], z[:, i], acc)
            s[:, k] = acc
    q = fma(f, s, x)
    coord = np.asarray(coord).reshape(n)
    keep = (coord[:, None] >= 0) & (np.arange(d)[None, :] != coord[:, None])
    return np.where(keep, x, q)


def gaussian_step_arrays(coords, logp, order, n0, C, f, coord, z, u_acc, lnprob, margin_out=None, diagonal=None):
    """One full Gaussian Metropolis step from pre-drawn arrays keyed by walker id (the contract of
    alabi_ens_step_with_randoms_gauss): the rule applied to the walkers of split 0 (order[:n0]) and then to those of split 1.
    ``margin_out`` (a list): every non-empty half appends lnp(q) - lnp(x) - ln u' of its proposals.  Returns coords, logp,
    accepted and the proposals q [W, d]."""
    coords = np.array(coords, dtype=np.float64, copy=True)
    logp = np.array(logp, dtype=np.float64, copy=True)
    W, d = coords.shape
    accepted = np.zeros(W, dtype=bool)
    qall = np.full((W, d), np.nan)
    coord = np.asarray(coord); z = np.asarray(z); u_acc = np.asarray(u_acc)
    for S in (np.asarray(order[:n0]), np.asarray(order[n0:])):
        if len(S) == 0:
            continue
        q = gaussian_proposal(coords[S], C, f, coord[S], z[S], diagonal)
        new_logp = np.asarray(lnprob(q), dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            lnpdiff = 0.0 + new_logp - logp[S]
            acc = lnpdiff > np.log(u_acc[S])
            if margin_out is not None:
                margin_out.append(lnpdiff - np.log(u_acc[S]))
        qall[S] = q
        coords[S[acc]] = q[acc]
        logp[S[acc]] = new_logp[acc]
        accepted[S[acc]] = True
    return coords, logp, accepted, qall


# --------------------------------------------------------------------------------------------------------------- the run
def run_ensemble_moves(p0, nsteps, lnprob_batch, seed, moves, thin_by=1, step0=0, logp0=None, id0=0, count_moves=None,
                       margin_out=None):
    """The array-driven run with the counter-based draws for move sets that hold Gaussian moves (``moves``: see ``move_table``),
    step for step -- the device's production contract.  The non-Gaussian steps of a mixture are those of
    walk_kde_numpy.run_ensemble_moves, called through their step functions.  ``id0``: the global id of this ensemble's walker 0.
    Returns chain, chain_logp, n_accept [W], coords, logp."""
    coords = np.array(p0, dtype=np.float64, copy=True)
    W, d = coords.shape
    kinds, cum, tp0, tp1, scales = move_table(moves, d, W)
    logp = np.asarray(lnprob_batch(coords), dtype=np.float64) if logp0 is None else np.array(logp0, dtype=np.float64)
    nstore = nsteps // thin_by
    chain = np.empty((nstore, W, d))
    chain_lp = np.empty((nstore, W))
    nacc = np.zeros(W, dtype=np.int64)
    block = 256
    for t in range(nsteps):
        if t % block == 0:
            dr = sn.draw_steps_batched(seed, step0 + t, min(block, nsteps - t), W, cum, id0)
        k = t % block
        mi = int(dr["move"][k])
        if count_moves is not None:
            count_moves[mi] = count_moves.get(mi, 0) + 1
        order, n0, u_acc = dr["order"][k], dr["n0"], dr["u_acc"][k]
        if kinds[mi] == KIND_GAUSS:
            f, coord, z = draw_gauss_randoms(seed, step0 + t, np.arange(W) + int(id0), id0, tp0[mi], int(tp1[mi]), d)
            C, diagonal = scales[mi]
            coords, logp, acc, _ = gaussian_step_arrays(coords, logp, order, n0, C, f, coord, z, u_acc, lnprob_batch,
                                                        margin_out=margin_out, diagonal=diagonal)
        elif kinds[mi] == 0:
            coords, logp, acc = wk.stretch_step_arrays(coords, logp, order, n0, dr["u_z"][k], dr["partner"][k], u_acc, lnprob_batch,
                                                       tp0[mi], margin_out=margin_out)
        elif kinds[mi] == 1:
            gamma = tp0[mi] * (1.0 + tp1[mi] * dr["n"][k])
            coords, logp, acc = wk.dm.de_step_arrays(coords, logp, order, n0, dr["partner"][k], dr["j2"][k], gamma, u_acc, lnprob_batch,
                                                     margin_out=margin_out)
        elif kinds[mi] == 2:
            coords, logp, acc, _ = sn.snooker_step_arrays(coords, logp, order, n0, dr["partner"][k], dr["j2"][k], dr["j3"][k], tp0[mi],
                                                          u_acc, lnprob_batch, margin_out=margin_out)
        elif kinds[mi] == wk.KIND_WALK:
            draws = wk._whole_half_draws(seed, step0 + t, W, order, n0, wk.KIND_WALK, tp0[mi], d, id0)
            coords, logp, acc = wk._walk_step(coords, logp, order, n0, draws, u_acc, lnprob_batch, margin_out)
        else:
            draws = wk._whole_half_draws(seed, step0 + t, W, order, n0, wk.KIND_KDE, 0, d, id0)
            row = np.zeros(W, dtype=np.int32); z = np.zeros((W, d))
            for S, (r_, z_) in draws:
                row[S] = r_; z[S] = z_
            coords, logp, acc, _, _ = wk.kde_step_arrays(coords, logp, order, n0, (tp0[mi], tp1[mi]), row, z, u_acc, lnprob_batch,
                                                         margin_out=margin_out)
        nacc += acc
        if (t + 1) % thin_by == 0:
            chain[(t + 1) // thin_by - 1] = coords
            chain_lp[(t + 1) // thin_by - 1] = logp
    return chain, chain_lp, nacc, coords, logp
