"""fp64 statement of the snooker update (ter Braak & Vrugt 2008, eq. 4) on the red-blue split of the GPU ensemble sampler, the
CPU statement ``alabi_amd.moves.SnookerMove`` is tested against (ens_draw_kernel, snooker_coord and the three-partner
half-step / propose kernels in alabi_amd/csrc/ensemble.hip).  Built on tests/de_move_numpy.py, which it leaves as it is.

The move.  Every walker s of the active set S takes three DISTINCT walkers z, z1, z2 of the complementary set C:

    delta = s - z          n = |delta|          e = delta / n
    p     = e.z1 - e.z2                          (projections of z1, z2 on the line through s and z)
    q     = s + (gamma p) e
    lnfac = (d - 1) (ln|q - z| - ln n)
    accept iff lnfac + lnp(q) - lnp(s) > ln u'

with the fixed step gamma = ``gammas`` (1.7 by default).  This is the PUBLISHED rule, not emcee 3's ``DESnookerMove`` (recalled
from emcee 3.1 ``moves/de_snooker.py``: half of this log factor, the direction divided by sqrt(norm), a four-way split), and
tests/test_snooker_host.py shows that only the published factor leaves a Gaussian invariant.

Degenerate input needs no branch: n == 0 (s and z coincide) makes e and q NaN, |q - z| == 0 makes lnfac -inf, and for d == 1
0 * (-inf) = NaN; in each case the comparison above is false and the walker keeps its row.

Operation order (the device mirrors it, so proposals agree bit for bit; sqrt and / are correctly rounded on both sides): the
four sums |delta|^2, e.z1, e.z2 and |q - z|^2 are ``_seq_sum``: every product rounded, then added in coordinate order
k = 0 .. d-1 starting from 0.0, no fused multiply-add.  gamma p is formed first, then multiplied by e_k, then added to s_k.

Draws.  Streams 0-4 are those of de_move_numpy: j1 (the index of z) is the stretch partner, stream 1 word 2; j2 (z1) is DE's
second partner, stream 1 word 3, bumped past j1.  New is
  stream 5 at (step, gid):  j3' = (r0 (nc - 2)) >> 32, bumped past min(j1, j2) and then past max(j1, j2): j3 (z2) is uniform
  over the nc - 2 other walkers, the triple uniform over the nc (nc - 1) (nc - 2) ordered triples.
"""
from __future__ import annotations

import numpy as np

import de_move_numpy as dm
from oracle.stretch_oracle import _ctr, philox4x32_10, stretch_step_arrays

STREAM_SNOOKER = 5
_S32 = np.uint64(32)


def move_table(moves, ndim):
    """de_move_numpy.move_table that also takes ("snooker", gammas, w): kind 2, p0 = gammas, p1 = 0."""
    kinds, p0, p1, w = [], [], [], []
    for m in moves:
        if m[0] == "snooker":
            kinds.append(2); p0.append(float(m[1])); p1.append(0.0); w.append(float(m[2]))
        else:
            k, _, a, b = dm.move_table([m], ndim)
            kinds.append(int(k[0])); p0.append(float(a[0])); p1.append(float(b[0])); w.append(float(m[-1]))
    w = np.asarray(w, dtype=np.float64)
    return np.asarray(kinds), np.cumsum(w / w.sum()), np.asarray(p0), np.asarray(p1)


def _third_index(r0, nc, j1, j2):
    """j3 from the first word of stream 5: one of the nc - 2 indices that are neither j1 nor j2."""
    j3 = ((np.asarray(r0).astype(np.uint64) * (nc.astype(np.uint64) - np.uint64(2))) >> _S32).astype(np.int32)
    lo, hi = np.minimum(j1, j2), np.maximum(j1, j2)
    j3 = j3 + (j3 >= lo)
    j3 = j3 + (j3 >= hi)
    return j3.astype(np.int32)


def draw_snooker_randoms(seed, step, W, cum, id0=0):
    """The snooker move's counter-based draws of one step: (move index, j1[W], j2[W], j3[W]) keyed by WALKER id; all three
    index the complementary list of the walker's own set."""
    move, j1, j2, _, _ = dm.draw_move_randoms(seed, step, W, cum, id0=id0)
    order, n0 = dm.draw_step_randoms(seed, step, W, id0)[:2]
    nc = np.empty(W, dtype=np.int64)
    nc[order[:n0]] = W - n0
    nc[order[n0:]] = n0
    r = philox4x32_10(_ctr(step, np.arange(W) + int(id0), STREAM_SNOOKER), dm._key(seed))
    return move, j1, j2, _third_index(r[:, 0], nc, j1, j2)


def draw_steps_batched(seed, step0, nsteps, W, cum, id0=0):
    """de_move_numpy.draw_steps_batched plus ``j3`` [nsteps, W]; everything else is that function's, untouched."""
    dr = dm.draw_steps_batched(seed, step0, nsteps, W, cum, id0)
    n0 = dr["n0"]
    nc = np.empty((nsteps, W), dtype=np.int64)
    np.put_along_axis(nc, dr["order"][:, :n0].astype(np.int64), W - n0, axis=1)
    np.put_along_axis(nc, dr["order"][:, n0:].astype(np.int64), n0, axis=1)
    steps = [int(step0) + k for k in range(int(nsteps))]
    c = np.empty((nsteps, W, 4), dtype=np.uint64)
    c[..., 0] = np.array([s & 0xFFFFFFFF for s in steps], dtype=np.uint64)[:, None]
    c[..., 1] = np.array([(s >> 32) & 0xFFFFFFFF for s in steps], dtype=np.uint64)[:, None]
    c[..., 2] = (np.arange(W) + int(id0)).astype(np.uint64)[None, :]
    c[..., 3] = np.uint64(STREAM_SNOOKER)
    r = philox4x32_10(c, dm._key(seed))
    dr["j3"] = _third_index(r[..., 0], nc, dr["partner"], dr["j2"])
    return dr


def _seq_sum(x):
    """Sum over the last axis in index order, starting from 0.0: the order of the device's lane_seq_sum."""
    acc = np.zeros(x.shape[:-1], dtype=np.float64)
    for k in range(x.shape[-1]):
        acc = acc + x[..., k]
    return acc


def snooker_proposal(s, z, z1, z2, gamma):
    """(q, n, |q - z|) of the rows s, z, z1, z2 [ns, d], in the stated operation order."""
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = s - z
        n = np.sqrt(_seq_sum(delta * delta))
        e = delta / n[:, None]
        p = _seq_sum(e * z1) - _seq_sum(e * z2)
        gp = gamma * p
        q = s + gp[:, None] * e
        dq = q - z
        nq = np.sqrt(_seq_sum(dq * dq))
    return q, n, nq


def snooker_step_arrays(coords, logp, order, n0, j1, j2, j3, gamma, u_acc, lnprob_batch, jac=None, margin_out=None):
    """One full red-blue snooker step from pre-drawn arrays keyed by walker id (the contract of
    alabi_ens_step_with_randoms_snooker).  ``jac``: the multiplier of (ln|q - z| - ln n); None is the move's d - 1, anything else
    exists for the negative controls of the invariance test only.  ``margin_out`` (a list): every half step appends
    lnfac + lnp(q) - lnp(s) - ln u' of its proposals, as stretch_step_arrays does (NaN for a degenerate proposal).  Returns coords,
    logp, accepted and the proposals' lnfac."""
    coords = np.array(coords, dtype=np.float64, copy=True)
    logp = np.array(logp, dtype=np.float64, copy=True)
    W, d = coords.shape
    mult = float(d) - 1.0 if jac is None else float(jac)
    accepted = np.zeros(W, dtype=bool)
    lnfac = np.zeros(W)
    sets = [np.asarray(order[:n0]), np.asarray(order[n0:])]
    for split in range(2):
        S, Cs = sets[split], sets[1 - split]
        if len(S) == 0:
            continue
        s, c = coords[S], coords[Cs]
        q, n, nq = snooker_proposal(s, c[j1[S]], c[j2[S]], c[j3[S]], gamma)
        new_logp = np.asarray(lnprob_batch(q), dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = mult * (np.log(nq) - np.log(n))
            lnpdiff = f + new_logp - logp[S]
            acc = lnpdiff > np.log(u_acc[S])                  # false for NaN and for -inf: degenerate proposals are rejected
            if margin_out is not None:
                margin_out.append(lnpdiff - np.log(u_acc[S]))
        lnfac[S] = f
        coords[S[acc]] = q[acc]
        logp[S[acc]] = new_logp[acc]
        accepted[S[acc]] = True
    return coords, logp, accepted, lnfac


def run_ensemble_moves(p0, nsteps, lnprob_batch, seed, moves, thin_by=1, step0=0, logp0=None, id0=0, count_moves=None, jac=None,
                       margin_out=None):
    """de_move_numpy.run_ensemble_moves for the three kinds of move (``moves``: see ``move_table``): the array-driven run with
    the counter-based draws, step for step -- the device's production contract.  Returns chain, chain_logp, n_accept[W],
    coords, logp.  ``margin_out``: see ``snooker_step_arrays``; two arrays per step."""
    coords = np.array(p0, dtype=np.float64, copy=True)
    W, d = coords.shape
    kinds, cum, tp0, tp1 = move_table(moves, d)
    logp = np.asarray(lnprob_batch(coords), dtype=np.float64) if logp0 is None else np.array(logp0, dtype=np.float64)
    nstore = nsteps // thin_by
    chain = np.empty((nstore, W, d))
    chain_lp = np.empty((nstore, W))
    nacc = np.zeros(W, dtype=np.int64)
    block = 256
    for t in range(nsteps):
        if t % block == 0:
            dr = draw_steps_batched(seed, step0 + t, min(block, nsteps - t), W, cum, id0)
        k = t % block
        mi = int(dr["move"][k])
        if count_moves is not None:
            count_moves[mi] = count_moves.get(mi, 0) + 1
        order, n0, u_acc = dr["order"][k], dr["n0"], dr["u_acc"][k]
        if kinds[mi] == 0:
            coords, logp, acc = stretch_step_arrays(coords, logp, order, n0, dr["u_z"][k], dr["partner"][k], u_acc, lnprob_batch,
                                                    tp0[mi], margin_out=margin_out)
        elif kinds[mi] == 1:
            gamma = tp0[mi] * (1.0 + tp1[mi] * dr["n"][k])
            coords, logp, acc = dm.de_step_arrays(coords, logp, order, n0, dr["partner"][k], dr["j2"][k], gamma, u_acc, lnprob_batch,
                                                  margin_out=margin_out)
        else:
            coords, logp, acc, _ = snooker_step_arrays(coords, logp, order, n0, dr["partner"][k], dr["j2"][k], dr["j3"][k], tp0[mi],
                                                       u_acc, lnprob_batch, jac=jac, margin_out=margin_out)
        nacc += acc
        if (t + 1) % thin_by == 0:
            chain[(t + 1) // thin_by - 1] = coords
            chain_lp[(t + 1) // thin_by - 1] = logp
    return chain, chain_lp, nacc, coords, logp
