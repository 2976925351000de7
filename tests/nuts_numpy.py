"""fp64 statement of the NUTS move (``alabi_amd.moves.NUTSMove``, kind 7 of the library's move table): the CPU statement that
ens_nuts_kernel (alabi_amd/csrc/ens_nuts.hip) is tested against.  Plain NumPy on tests/hmc_numpy.py's targets and Philox helpers,
which it leaves as they are.  Multinomial NUTS (Betancourt 2017, as in Stan) in the project's whitened momentum.

One transition of walker x with lp = the caller's logp, g = grad lnp(x), C C^T = cov, step size e, max_depth Dmax:

    z0 ~ N(0, I);  H0 = -lp + |z0|^2 / 2;  left end = right end = (x, z0, g);  rho = z0;  proposal = (x, lp, g);  ln W = 0
    doubling j = 0 ... Dmax - 1: bit j of the direction word set -> forward from the right end (s = e), else backward from the left
    end (s = -e); 2^j leaves, each   z += (s / 2) C^T g;  q += s C z;  (lp_q, g) = lnp, grad lnp at q;  z += (s / 2) C^T g
        delta = H0 - (-lp_q + |z|^2 / 2);  divergent iff not (delta > -1000): drop the subtree, end the transition
        ln w = delta where q lies in the open box, else -inf;  a = min(1, exp(delta)) in the box, else 0 (0 for a divergent leaf)
        ln w > -inf:  ln W' = logaddexp(ln W', ln w);  the leaf is the subtree's candidate iff ln u_leaf < ln w - ln W'
        rho' += z;  an aligned block of 2^k leaves (k >= 1) that ends here turns iff rho_block . z_first <= 0 or
        rho_block . z_last <= 0: drop the subtree, end the transition
    a complete subtree: proposal = candidate iff ln W' > -inf and ln u_tree,j < ln W' - ln W;  ln W = logaddexp(ln W, ln W');
        rho += rho';  the extended end moves;  stop iff rho . z_left <= 0 or rho . z_right <= 0
    the walker becomes the proposal with the lp and g of its leaf; "taken" iff the proposal was ever replaced.

lnp is hmc_numpy's target WITHOUT the box gate; the box enters through the weights alone.

The U-turn test inside a subtree is stated twice.  ``form="blocks"``: every z of the subtree is kept and rho_block is summed over
the block.  ``form="checkpoints"`` (the device's): leaf n even stores (z, running rho' including it) in slot popcount(n); leaf n
odd with t trailing one bits checks slots popcount(n >> 1) down to popcount(n >> 1) - t + 1, slot i with rho = running -
ckpt_sum[i] + ckpt_z[i].  Both make the same checks in the same order (smallest block first).

Draws.  Philox counter (step, global walker id, stream word), word = S + 16 b:
    S = 3, 11, 12:   the step's move, the momentum normals and the jitter as for the HMC move (hmc_numpy); stream 2 is not read
    S = 13, b = 0:   bit j of r0 is the direction of doubling j
    S = 14, b = n:   u_leaf = u53(r0, r1) of the leaf with ordinal n within the transition (0 ... 2^Dmax - 2)
    S = 15, b = j:   u_tree,j = u53(r0, r1)

Every decision's margin is recorded in ``rec`` (a dict of lists): "cmp" ln u - threshold of every leaf and tree comparison;
"uturn" (dot product, 100 x 1e-7 x (|rho|_1 + m |z|_1)) of every U-turn product, m the number of points in rho; "wall" the
smallest distance of a leaf's coordinates from a wall; "delta" every leaf's delta; "events" what the case set must cover.
"""
from __future__ import annotations

import numpy as np

import hmc_numpy as hm
from oracle.stretch_oracle import u53

wk = hm.wk
STREAM_DIR, STREAM_LEAF, STREAM_TREE = 13, 14, 15
KIND_NUTS = 7
MAX_DEPTH = 10
STOP_DEPTH, STOP_TREE, STOP_SUBTREE, STOP_DIVERGENT = 0, 1, 2, 3
DIVERGENT_BELOW = -1000.0
UTURN_EPS = 100 * 1e-7     # the project's margin factor x its 1e-7 agreement of momenta


def move_table(moves, ndim):
    """``moves``: [(cov, step_size or None, max_depth, jitter or None, weight)] -> kinds, cum, p0, p1, [(C, diagonal)]."""
    _, cum, p0, p1, scales = hm.move_table(moves, ndim)
    return np.full(len(moves), KIND_NUTS), cum, p0, p1, scales


def _rec(rec, key, value):
    if rec is not None:
        rec.setdefault(key, []).append(value)


def _uturn(rho, z_first, z_last, m, rec):
    """The test of a block (or of the tree) with ``m`` points in rho; records both products with their bounds."""
    d1, d2 = float(rho @ z_first), float(rho @ z_last)
    l1 = float(np.sum(np.abs(rho)))
    _rec(rec, "uturn", (d1, UTURN_EPS * (l1 + m * float(np.sum(np.abs(z_first))))))
    _rec(rec, "uturn", (d2, UTURN_EPS * (l1 + m * float(np.sum(np.abs(z_last))))))
    return d1 <= 0.0 or d2 <= 0.0


def transition(target, x, lp, g, C, e, z0, dirw, u_leaf, u_tree, max_depth, form="checkpoints", rec=None):
    """One transition of ONE walker.  x, g, z0 [d]; dirw the direction word; u_leaf [2^max_depth - 1]; u_tree [max_depth].
    Returns (x', lp', g', trace, a_sum) with trace = (depth reached, leaves made, stop reason, 1 if a leaf was taken)."""
    assert form in ("checkpoints", "blocks") and 1 <= max_depth <= MAX_DEPTH
    lo, hi = target.bounds[:, 0], target.bounds[:, 1]
    H0 = -lp + 0.5 * float(z0 @ z0)
    left = right = (np.array(x, dtype=np.float64), np.array(z0, dtype=np.float64), np.array(g, dtype=np.float64))
    rho = np.array(z0, dtype=np.float64)
    prop, lnW = (left[0], float(lp), left[2]), 0.0
    leaves = depth = taken = 0
    a_sum, reason = 0.0, STOP_DEPTH
    with np.errstate(all="ignore"):
        for j in range(max_depth):
            fwd = bool((int(dirw) >> j) & 1)
            s = e if fwd else -e
            q, z, gq = right if fwd else left
            rho_s, lnWs, cand = np.zeros_like(rho), -np.inf, None
            zs, ck_z, ck_r = [], {}, {}
            has_out, dropped = False, False
            for n in range(1 << j):
                z = z + (0.5 * s) * (gq @ C)                     # C^T g
                q = q + s * (C @ z)
                lv, gv, _ = target.value_grad(q[None, :])
                lpq, gq = float(lv[0]), gv[0]
                z = z + (0.5 * s) * (gq @ C)
                delta = H0 - (-lpq + 0.5 * float(z @ z))
                ordinal = leaves
                leaves += 1
                _rec(rec, "delta", delta)
                if not (delta > DIVERGENT_BELOW):
                    reason, dropped = STOP_DIVERGENT, True
                    break
                _rec(rec, "wall", float(min(np.min(np.abs(q - lo)), np.min(np.abs(q - hi)))))
                if bool(np.all((q > lo) & (q < hi))):
                    a_sum += min(1.0, float(np.exp(delta)))
                    lnWs = float(np.logaddexp(lnWs, delta))
                    thr = delta - lnWs
                    lnu = float(np.log(u_leaf[ordinal]))
                    _rec(rec, "cmp", lnu - thr)
                    if lnu < thr:
                        cand = (q, lpq, gq)
                else:
                    has_out = True
                rho_s = rho_s + z
                turn = False
                if form == "blocks":
                    zs.append(z)
                    k = 1
                    while (n + 1) % (1 << k) == 0:                  # the aligned blocks that end at leaf n, smallest first
                        blk = zs[n + 1 - (1 << k):]
                        turn |= _uturn(np.sum(blk, axis=0), blk[0], z, 1 << k, rec)
                        k += 1
                elif n % 2 == 0:
                    slot = bin(n).count("1")
                    ck_z[slot], ck_r[slot] = z, rho_s
                else:
                    base, i = bin(n >> 1).count("1"), 0
                    while (n >> i) & 1:
                        zf = ck_z[base - i]
                        turn |= _uturn(rho_s - ck_r[base - i] + zf, zf, z, 2 << i, rec)
                        i += 1
                if turn:
                    reason, dropped = STOP_SUBTREE, True
                    break
            if dropped:
                break
            if lnWs > -np.inf:
                thr = lnWs - lnW
                lnu = float(np.log(u_tree[j]))
                _rec(rec, "cmp", lnu - thr)
                if lnu < thr:
                    prop, taken = cand, 1
            if has_out:
                _rec(rec, "events", "kept_subtree_with_out_of_box_leaf")
            lnW = float(np.logaddexp(lnW, lnWs))
            rho = rho + rho_s
            if fwd:
                right = (q, z, gq)
            else:
                left = (q, z, gq)
            depth = j + 1
            _rec(rec, "events", "forward" if fwd else "backward")
            if _uturn(rho, left[1], right[1], (2 << j), rec):
                reason = STOP_TREE
                break
    _rec(rec, "events", ("stop", reason))
    _rec(rec, "events", ("depth", depth))
    if not taken:
        _rec(rec, "events", "stays")
    return prop[0], prop[1], prop[2], (depth, leaves, reason, taken), a_sum


def nuts_step_arrays(target, coords, logp, grad, C, e, z0, dirw, u_leaf, u_tree, max_depth, form="checkpoints", rec=None):
    """One transition of every walker from pre-drawn arrays keyed by walker id (the contract of
    alabi_ens_step_with_randoms_nuts).  Returns coords, logp, grad, trace [W, 4] (int), a_sum [W]."""
    W = len(coords)
    out_c, out_lp, out_g = np.array(coords, copy=True), np.array(logp, copy=True), np.array(grad, copy=True)
    trace, a_sum = np.zeros((W, 4), dtype=np.int64), np.zeros(W)
    for w in range(W):
        out_c[w], out_lp[w], out_g[w], trace[w], a_sum[w] = transition(target, coords[w], float(logp[w]), grad[w], C, e, z0[w], dirw[w],
                                                                       u_leaf[w], u_tree[w], max_depth, form, rec)
    return out_c, out_lp, out_g, trace, a_sum


# --------------------------------------------------------------------------------------------------------------- the draws
def draw_nuts_randoms(seed, step, gids, g0, cum, p0, p1, d, max_depth=None):
    """The production draws of one step for the walkers ``gids`` of the ensemble whose walker 0 is ``g0``: the move's index, e,
    z0 [n, d], the direction words [n] (uint32), u_leaf [n, 2^D - 1] and u_tree [n, D], D = the move's max_depth (or ``max_depth``)."""
    gids = np.asarray(gids)
    mi, e, z0, _ = hm.draw_hmc_randoms(seed, step, gids, g0, cum, p0, p1, d)
    D = int(np.floor(p1[mi])) if max_depth is None else int(max_depth)
    dirw = wk._philox(seed, step, gids, [STREAM_DIR])[:, 0, 0].astype(np.uint32)
    r = wk._philox(seed, step, gids, STREAM_LEAF + 16 * np.arange((1 << D) - 1))
    u_leaf = u53(r[..., 0], r[..., 1])
    r = wk._philox(seed, step, gids, STREAM_TREE + 16 * np.arange(D))
    return mi, e, z0, dirw, u_leaf, u53(r[..., 0], r[..., 1])


# ----------------------------------------------------------------------------------------------------------------- the run
def run_nuts(target, p0, nsteps, seed, moves, thin_by=1, step0=0, logp0=None, id0=0, count_moves=None, rec=None, form="checkpoints"):
    """The run with the counter-based draws, transition for transition -- the device's production contract.  ``moves``: see
    ``move_table``.  Returns chain, chain_logp, n_accept [W], coords, logp, counts [W, 3] (leaves, depths, divergent), a_sum [W]."""
    coords = np.array(p0, dtype=np.float64, copy=True)
    W, d = coords.shape
    _, cum, tp0, tp1, scales = move_table(moves, d)
    logp = np.asarray(target(coords), dtype=np.float64) if logp0 is None else np.array(logp0, dtype=np.float64)
    grad = target.value_grad(coords)[1]
    nstore = nsteps // thin_by
    chain, chain_lp = np.empty((nstore, W, d)), np.empty((nstore, W))
    nacc, counts, a_sum = np.zeros(W, dtype=np.int64), np.zeros((W, 3), dtype=np.int64), np.zeros(W)
    for t in range(nsteps):
        mi, e, z0, dirw, u_leaf, u_tree = draw_nuts_randoms(seed, step0 + t, np.arange(W) + int(id0), id0, cum, tp0, tp1, d)
        if count_moves is not None:
            count_moves[mi] = count_moves.get(mi, 0) + 1
        coords, logp, grad, trace, a = nuts_step_arrays(target, coords, logp, grad, scales[mi][0], e, z0, dirw, u_leaf, u_tree,
                                                        int(np.floor(tp1[mi])), form, rec)
        nacc += trace[:, 3]
        counts[:, 0] += trace[:, 1]; counts[:, 1] += trace[:, 0]; counts[:, 2] += trace[:, 2] == STOP_DIVERGENT
        a_sum += a
        if (t + 1) % thin_by == 0:
            chain[(t + 1) // thin_by - 1] = coords
            chain_lp[(t + 1) // thin_by - 1] = logp
    return chain, chain_lp, nacc, coords, logp, counts, a_sum


# ------------------------------------------------------------------------------------------------------------ honesty
def honesty(rec, min_margin):
    """The four margin conditions of a model run as a dict of the worst figures and ``ok``."""
    cmp_ = np.abs(np.asarray(rec.get("cmp", [np.inf]), dtype=np.float64))
    ut = np.asarray(rec.get("uturn", [(np.inf, 0.0)]), dtype=np.float64)
    wall = np.asarray(rec.get("wall", [np.inf]), dtype=np.float64)
    delta = np.asarray(rec.get("delta", [0.0]), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        far = np.where(np.isnan(delta), np.inf, np.abs(delta - DIVERGENT_BELOW))
    slack = np.abs(ut[:, 0]) - ut[:, 1]
    out = dict(min_cmp=float(cmp_.min()), min_uturn_slack=float(slack.min()), min_wall=float(wall.min()), min_delta_gap=float(far.min()))
    out["ok"] = bool(out["min_cmp"] > min_margin and out["min_uturn_slack"] > 0.0 and out["min_wall"] > 1e-5 and out["min_delta_gap"] >= 1.0)
    return out
