"""fp64 restatement of emcee's DEMove and of weighted move mixtures, the CPU statement the moves of the GPU ensemble
sampler are tested against (alabi_amd/moves.py, alabi_amd/csrc/ensemble.hip).

PARITY UNPINNED, as oracle/stretch_oracle.py says of the stretch move: emcee is not installed here.  Restated from emcee 3.1
``moves/de.py`` (DEMove.setup / get_proposal, _get_nondiagonal_pairs), ``moves/red_blue.py`` (RedBlueMove.propose) and
``ensemble.py`` (one move per step: ``self._random.choice(self._moves, p=self._weights)``), anchored on the reference call
site alabi/core.py:2144 (sampler_kwargs['moves']) -> :2319 (emcee.EnsembleSampler(..., **sampler_kwargs)).

Built on oracle.stretch_oracle's Philox, u53 and draw_step_randoms.  Streams 0-2 are the stretch oracle's; the moves add
  stream 3 at (step, id0):  u = u53(r0, r1), move index = #{k: cum[k] <= u} clipped to n - 1, cum = cumsum(w / sum w);
  words 2, 3 of the PROPOSE call (stream 1): j1 = (r2 nc) >> 32 (the stretch partner), j2' = (r3 (nc - 1)) >> 32,
      j2 = j2' + (j2' >= j1): uniform over the nc (nc - 1) ordered pairs of _get_nondiagonal_pairs;
  stream 4 at (step, gid):  n = sqrt(-2 log(1 - u53(r0, r1))) cos(2 pi u53(r2, r3)), gamma = g0 (1 + sigma n).
"""
from __future__ import annotations

import numpy as np

from oracle.stretch_oracle import (STREAM_PROPOSE, _ctr, draw_step_randoms, philox4x32_10, stretch_step_arrays, u53)

STREAM_MOVE, STREAM_GAMMA = 3, 4
TWO_PI = 6.283185307179586
_S32 = np.uint64(32)


def move_table(moves, ndim):
    """[(kind, params..., weight)] -> (kinds, cum, p0, p1).  ``moves`` items: ("stretch", a, w) or ("de", sigma, gamma0, w)."""
    kinds, p0, p1, w = [], [], [], []
    for m in moves:
        if m[0] == "stretch":
            kinds.append(0); p0.append(float(m[1])); p1.append(0.0); w.append(float(m[2]))
        else:
            g0 = 2.38 / np.sqrt(2 * ndim) if m[2] is None else float(m[2])
            kinds.append(1); p0.append(g0); p1.append(float(m[1])); w.append(float(m[3]))
    w = np.asarray(w, dtype=np.float64)
    return np.asarray(kinds), np.cumsum(w / w.sum()), np.asarray(p0), np.asarray(p1)


def _key(seed):
    return (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)


def draw_move_randoms(seed, step, W, cum, g0=1.0, sigma=0.0, id0=0):
    """The moves' counter-based draws of one step: (move index, j1[W], j2[W], n[W], gamma[W]), keyed by WALKER id.
    j1 / j2 index the complementary list of the walker's own set; gamma = g0 (1 + sigma n)."""
    key = _key(seed)
    cum = np.asarray(cum, dtype=np.float64)
    rm = philox4x32_10(_ctr(step, np.array([int(id0)]), STREAM_MOVE), key)
    um = u53(rm[:, 0], rm[:, 1])[0]
    move = min(int(np.sum(cum <= um)), len(cum) - 1)
    order, n0, _, partner, _ = draw_step_randoms(seed, step, W, id0)
    gids = np.arange(W) + int(id0)
    label = np.empty(W, dtype=np.int64)
    label[order[:n0]] = 0
    label[order[n0:]] = 1
    nc = np.where(label == 0, W - n0, n0).astype(np.uint64)
    rp = philox4x32_10(_ctr(step, gids, STREAM_PROPOSE), key)
    j1 = ((rp[:, 2].astype(np.uint64) * nc) >> _S32).astype(np.int32)
    assert np.array_equal(j1, partner)
    j2p = ((rp[:, 3].astype(np.uint64) * (nc - np.uint64(1))) >> _S32).astype(np.int32)
    j2 = (j2p + (j2p >= j1)).astype(np.int32)
    rg = philox4x32_10(_ctr(step, gids, STREAM_GAMMA), key)
    u1, u2 = u53(rg[:, 0], rg[:, 1]), u53(rg[:, 2], rg[:, 3])
    n = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(TWO_PI * u2)
    gamma = g0 * (1.0 + sigma * n)
    return move, j1, j2, n, gamma


def de_step_arrays(coords, logp, order, n0, j1, j2, gamma, u_acc, lnprob_batch, margin_out=None):
    """One full red-blue DE step from pre-drawn arrays keyed by walker id (the contract of alabi_ens_step_with_randoms_de):
    q = s + gamma (C[j2] - C[j1]); accept iff logp(q) - logp(s) > log(u').  ``margin_out`` (a list): every half step appends
    logp(q) - logp(s) - log(u') of its proposals, as stretch_step_arrays does."""
    coords = np.array(coords, dtype=np.float64, copy=True)
    logp = np.array(logp, dtype=np.float64, copy=True)
    W = coords.shape[0]
    accepted = np.zeros(W, dtype=bool)
    sets = [np.asarray(order[:n0]), np.asarray(order[n0:])]
    for split in range(2):
        S, Cs = sets[split], sets[1 - split]
        if len(S) == 0:
            continue
        s = coords[S]
        c = coords[Cs]
        pairs = np.stack([j1[S], j2[S]], axis=1)
        diffs = np.diff(c[pairs], axis=1).squeeze(axis=1)           # c[j2] - c[j1]
        q = s + gamma[S][:, None] * diffs
        new_logp = np.asarray(lnprob_batch(q), dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            lnpdiff = 0.0 + new_logp - logp[S]
            acc = lnpdiff > np.log(u_acc[S])
            if margin_out is not None:
                margin_out.append(lnpdiff - np.log(u_acc[S]))
        coords[S[acc]] = q[acc]
        logp[S[acc]] = new_logp[acc]
        accepted[S[acc]] = True
    return coords, logp, accepted


def emcee_literal_de_step(coords, logp, lnprob_one, random, sigma=1.0e-5, gamma0=None, record=None):
    """emcee 3.1 RedBlueMove.propose with DEMove.setup / get_proposal, draw for draw from a ``RandomState``: the shuffle of
    the labels, then per half the pairs table, ``random.choice(npairs, size=ns)``, ``random.randn(ns, 1)``, and one
    ``rand()`` per accept test."""
    coords = np.array(coords, dtype=np.float64, copy=True)
    logp = np.array(logp, dtype=np.float64, copy=True)
    nwalkers, ndim = coords.shape
    g0 = 2.38 / np.sqrt(2 * ndim) if gamma0 is None else gamma0            # DEMove.setup
    accepted = np.zeros(nwalkers, dtype=bool)
    all_inds = np.arange(nwalkers)
    inds = all_inds % 2
    random.shuffle(inds)
    if record is not None:
        record.update(inds=inds.copy(), j1=[], j2=[], gamma=[], u_acc=[])
    for split in range(2):
        S1 = inds == split
        sets = [coords[inds == j] for j in range(2)]
        s = sets[split]
        c = np.concatenate(sets[:split] + sets[split + 1:], axis=0)
        ns, nc = len(s), len(c)
        # DEMove.get_proposal
        pairs = _get_nondiagonal_pairs(nc)
        indices = random.choice(pairs.shape[0], size=ns, replace=True)
        pairs = pairs[indices]
        diffs = np.diff(c[pairs], axis=1).squeeze(axis=1)
        gamma = g0 * (1 + sigma * random.randn(ns, 1))
        q = s + gamma * diffs
        factors = np.zeros(ns, dtype=np.float64)
        new_log_probs = np.array([float(lnprob_one(v)) for v in q])
        uacc = np.empty(ns)
        for i, (j, f, nlp) in enumerate(zip(all_inds[S1], factors, new_log_probs)):
            lnpdiff = f + nlp - logp[j]
            uacc[i] = random.rand()
            with np.errstate(divide="ignore"):
                if lnpdiff > np.log(uacc[i]):
                    accepted[j] = True
        upd = all_inds[S1][accepted[S1]]
        m = accepted[S1]
        coords[upd] = q[m]
        logp[upd] = new_log_probs[m]
        if record is not None:
            record["j1"].append(pairs[:, 0]); record["j2"].append(pairs[:, 1])
            record["gamma"].append(gamma[:, 0]); record["u_acc"].append(uacc)
    return coords, logp, accepted


def _get_nondiagonal_pairs(n):
    """emcee 3.1 moves/de.py: the n (n - 1) ordered pairs (i, j), i != j."""
    rows, cols = np.tril_indices(n, -1)
    pairs = np.column_stack([rows, cols, cols, rows]).reshape(-1, 2)
    return pairs


def literal_de_draws_to_arrays(record):
    """Re-key the draws recorded by ``emcee_literal_de_step`` by walker id."""
    inds = record["inds"]
    W = len(inds)
    ids = np.arange(W)
    order = np.concatenate([ids[inds == 0], ids[inds == 1]]).astype(np.int32)
    n0 = int(np.sum(inds == 0))
    j1 = np.empty(W, dtype=np.int32); j2 = np.empty(W, dtype=np.int32)
    gamma = np.empty(W); u_acc = np.empty(W)
    for split in range(2):
        S = ids[inds == split]
        j1[S] = record["j1"][split]; j2[S] = record["j2"][split]
        gamma[S] = record["gamma"][split]; u_acc[S] = record["u_acc"][split]
    return order, n0, j1, j2, gamma, u_acc


def draw_steps_batched(seed, step0, nsteps, W, cum, id0=0):
    """draw_step_randoms and draw_move_randoms for ``nsteps`` consecutive steps in one vectorised pass (the long statistical
    runs would otherwise spend their time in per-step Philox calls).  Returns a dict of arrays with a leading step axis:
    order, u_z, partner (= j1), u_acc, j2, n [nsteps, W], move [nsteps], and the scalar n0.  Pinned against the two
    single-step statements in tests/test_moves_host.py."""
    key = _key(seed)
    cum = np.asarray(cum, dtype=np.float64)
    steps = np.arange(int(step0), int(step0) + int(nsteps))
    ids = np.arange(W)

    def ctr(walkers, stream):
        c = np.empty((len(steps),) + walkers.shape + (4,), dtype=np.uint64)
        lo = np.array([s & 0xFFFFFFFF for s in steps.tolist()], dtype=np.uint64)
        hi = np.array([(s >> 32) & 0xFFFFFFFF for s in steps.tolist()], dtype=np.uint64)
        c[..., 0] = lo[:, None]
        c[..., 1] = hi[:, None]
        c[..., 2] = walkers.astype(np.uint64)[None, :]
        c[..., 3] = np.uint64(stream)
        return c
    gids = ids + int(id0)
    r = philox4x32_10(ctr(gids, 0), key).astype(np.uint64)
    k64 = (r[..., 0] << _S32) | r[..., 1]
    srt = np.argsort(k64, axis=1, kind="stable")                      # ties broken by walker id
    rank = np.empty_like(srt)
    np.put_along_axis(rank, srt, np.broadcast_to(ids, srt.shape), axis=1)
    label = rank % 2
    n0 = (W + 1) // 2
    order = np.argsort(label, axis=1, kind="stable").astype(np.int32)  # label-0 walkers in index order, then label-1
    rp = philox4x32_10(ctr(gids, STREAM_PROPOSE), key)
    u_z = u53(rp[..., 0], rp[..., 1])
    nc = np.where(label == 0, W - n0, n0).astype(np.uint64)
    j1 = ((rp[..., 2].astype(np.uint64) * nc) >> _S32).astype(np.int32)
    j2p = ((rp[..., 3].astype(np.uint64) * (nc - np.uint64(1))) >> _S32).astype(np.int32)
    j2 = (j2p + (j2p >= j1)).astype(np.int32)
    ra = philox4x32_10(ctr(gids, 2), key)
    u_acc = u53(ra[..., 0], ra[..., 1])
    rg = philox4x32_10(ctr(gids, STREAM_GAMMA), key)
    u1, u2 = u53(rg[..., 0], rg[..., 1]), u53(rg[..., 2], rg[..., 3])
    n = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(TWO_PI * u2)
    rm = philox4x32_10(ctr(np.array([int(id0)]), STREAM_MOVE), key)
    um = u53(rm[..., 0], rm[..., 1])[:, 0]
    move = np.minimum(np.sum(cum[None, :] <= um[:, None], axis=1), len(cum) - 1)
    return dict(order=order, n0=n0, u_z=u_z, partner=j1, u_acc=u_acc, j2=j2, n=n, move=move)


def run_ensemble_moves(p0, nsteps, lnprob_batch, seed, moves, thin_by=1, step0=0, logp0=None, id0=0, count_moves=None,
                       margin_out=None):
    """Array-driven run of a move mixture with the counter-based draws, step for step (device production contract).
    ``moves``: see ``move_table``.  Returns chain, chain_logp, n_accept[W], coords, logp as stretch_oracle.run_ensemble.
    ``margin_out``: see ``de_step_arrays``; two arrays per step."""
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
        else:
            gamma = tp0[mi] * (1.0 + tp1[mi] * dr["n"][k])
            coords, logp, acc = de_step_arrays(coords, logp, order, n0, dr["partner"][k], dr["j2"][k], gamma, u_acc, lnprob_batch,
                                               margin_out=margin_out)
        nacc += acc
        if (t + 1) % thin_by == 0:
            chain[(t + 1) // thin_by - 1] = coords
            chain_lp[(t + 1) // thin_by - 1] = logp
    return chain, chain_lp, nacc, coords, logp


# ---- the two-mode target of the mixing tests (tests/test_moves_host.py, tests/test_gpu_moves.py)
TWO_MODE_MOVES = [("de", 1e-5, None, 0.9), ("de", 1e-5, 1.0, 0.1)]   # ter Braak: gamma0 = 1 at weight 0.1


def two_mode_lnprob(q):
    """Two unit Gaussians in five dimensions at x_0 = +5 and x_0 = -5, equal weights."""
    r = np.sum(q[:, 1:] ** 2, axis=1)
    return np.logaddexp(-0.5 * ((q[:, 0] - 5.0) ** 2 + r), -0.5 * ((q[:, 0] + 5.0) ** 2 + r))


def two_mode_start(W=32, n_plus=4, seed=5):
    p0 = np.random.RandomState(seed).normal(size=(W, 5))
    p0[:, 0] += np.where(np.arange(W) < n_plus, 5.0, -5.0)
    return p0


def mode_share_and_crossings(chain):
    plus = chain[:, :, 0] > 0.0
    return float(plus.mean()), int(np.sum(plus[1:] != plus[:-1]))
