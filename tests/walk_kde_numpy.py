"""fp64 statement of emcee's WalkMove and KDEMove on the red-blue split of the GPU ensemble sampler: the CPU statement
``alabi_amd.moves.WalkMove`` / ``KDEMove`` are tested against (wk_proposal, ens_kde_prepass_kernel and the whole-half
instantiations of the half-step / propose kernels in alabi_amd/csrc/ensemble.hip).  Built on tests/snooker_numpy.py and
tests/de_move_numpy.py, which it leaves as they are.

PARITY UNPINNED against emcee itself, as de_move_numpy.py says of DEMove: emcee is not installed here.  Restated from emcee 3
``moves/walk.py`` (``random.multivariate_normal(x, np.cov(C[J], rowvar=False))``) and ``moves/kde.py`` (``gaussian_kde(C.T,
bw_method)``, ``resample``, ``logpdf(x) - logpdf(q)``), anchored on alabi/core.py:2144 -> :2319.  ``emcee_literal_walk_step`` and
``emcee_literal_kde_step`` are those lines with ``np.cov`` / ``scipy.stats.gaussian_kde``; tests/test_walk_kde_host.py pins the
forms below to them.

S is the active half, C the complementary one (in list order), Nc = |C|.

Walk (kind 3).  J = s0 distinct rows of C in ascending list position (s0 = Nc: all of them), z_m standard normal:
    mean_k = (c_{J0,k} + c_{J1,k} + ...) / s0             sum from 0.0 in the order m = 0 .. s0-1
    acc_k  = sum_m z_m (c_{Jm,k} - mean_k)                products rounded, added from 0.0 in the order m = 0 .. s0-1
    q_k    = x_k + (1 / sqrt(s0 - 1)) acc_k               log factor 0
With A = (C[J] - mean)^T / sqrt(s0 - 1), A A^T = np.cov(C[J], rowvar=False): q is a draw from N(x, cov) without a factorisation,
also where s0 <= d and the covariance has no Cholesky factor.

KDE (kind 4).  Once per half step:
    mean_k = (sum_j c_jk) / Nc                            sums over j = 0 .. Nc-1 from 0.0, products rounded
    cov_ab = (sum_j (c_ja - mean_a)(c_jb - mean_b)) / (Nc - 1)
    H      = (f f) cov                                    f: scipy's scotts_factor / silverman_factor / scalar at n = Nc
    L      = left-looking Cholesky of H: t_ij = H_ij - L_i0 L_j0 - L_i1 L_j1 - ... (k ascending), L_jj = sqrt(t_jj), L_ij = t_ij / L_jj
    y_j    = L^-1 (c_j - mean)                            forward substitution, k ascending
a pivot t_jj that is not positive and finite makes the half step singular: every proposal is rejected.  Per walker x of S:
    q_k    = c_rk + (L_k0 z_0 + ... + L_kk z_k)           sum from 0.0, m ascending
    lnfac  = LSE_j(-|L^-1(x - mean) - y_j|^2 / 2) - LSE_j(-|L^-1(q - mean) - y_j|^2 / 2)   = kde.logpdf(x) - kde.logpdf(q)
the two log-sum-exps are compared by tolerance (the device reduces them in a tree).

Draws.  Streams 0-5 are those of snooker_numpy / de_move_numpy, untouched.  New, with the Philox counter (step, gid, word) and
word = S + 16 b:
    S = 6, b = j >> 1:  64-bit key of row j of the complementary list: words (0, 1) for even j, (2, 3) for odd j.  j is in J iff the
                        rank of its key among the Nc keys (ties by j) is < s0; no key is drawn when s0 = Nc;
    S = 7, b = j:       z of row j: sqrt(-2 ln(1 - u53(r0, r1))) cos(2 pi u53(r2, r3)), Box-Muller as stream 4;
    S = 8, b = 0:       r = (r0 Nc) >> 32;   b = 1 + k: z_k as above.
Every subset of size s0 is equally likely: the keys are i.i.d., so their ranks are a uniform random permutation.
"""
from __future__ import annotations

import numpy as np
from scipy.special import logsumexp

import de_move_numpy as dm
import snooker_numpy as sn
from oracle.stretch_oracle import philox4x32_10, stretch_step_arrays, u53

STREAM_KEYS, STREAM_WALK_Z, STREAM_KDE = 6, 7, 8
KIND_WALK, KIND_KDE = 3, 4
_S32 = np.uint64(32)


# ---------------------------------------------------------------------------------------------------------------- the table
def kde_factor(bw_method, nc, d):
    """scipy.stats.gaussian_kde's factor with unit weights (neff = n = nc)."""
    if bw_method is None or bw_method == "scott":
        return float(np.power(float(nc), -1.0 / (d + 4)))
    if bw_method == "silverman":
        return float(np.power(float(nc) * (d + 2.0) / 4.0, -1.0 / (d + 4)))
    return float(bw_method)


def move_table(moves, ndim, W):
    """snooker_numpy.move_table that also takes ("walk", s or None, w): kind 3, p0 = s (0: all), p1 = 0, and
    ("kde", bw_method, w): kind 4, p0 / p1 = the factor of split 0 / split 1 (Nc = W - n0 / n0)."""
    n0 = (W + 1) // 2
    kinds, p0, p1, w = [], [], [], []
    for m in moves:
        if m[0] == "walk":
            kinds.append(KIND_WALK); p0.append(0.0 if m[1] is None else float(m[1])); p1.append(0.0)
        elif m[0] == "kde":
            kinds.append(KIND_KDE); p0.append(kde_factor(m[1], W - n0, ndim)); p1.append(kde_factor(m[1], n0, ndim))
        else:
            k, _, a, b = sn.move_table([m], ndim)
            kinds.append(int(k[0])); p0.append(float(a[0])); p1.append(float(b[0]))
        w.append(float(m[-1]))
    w = np.asarray(w, dtype=np.float64)
    return np.asarray(kinds), np.cumsum(w / w.sum()), np.asarray(p0), np.asarray(p1)


# ---------------------------------------------------------------------------------------------------------------- the draws
def _philox(seed, step, gid, words):
    """Philox outputs [len(gid), len(words), 4] at counters (step, gid, word)."""
    gid = np.asarray(gid, dtype=np.uint64).reshape(-1)
    words = np.asarray(words, dtype=np.uint64).reshape(-1)
    c = np.empty((len(gid), len(words), 4), dtype=np.uint64)
    c[..., 0] = np.uint64(int(step) & 0xFFFFFFFF)
    c[..., 1] = np.uint64((int(step) >> 32) & 0xFFFFFFFF)
    c[..., 2] = gid[:, None]
    c[..., 3] = words[None, :]
    return philox4x32_10(c, dm._key(seed))


def _normal(r):
    u1, u2 = u53(r[..., 0], r[..., 1]), u53(r[..., 2], r[..., 3])
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(dm.TWO_PI * u2)


def draw_walk_randoms(seed, step, gids, nc, s0):
    """Subset and normals of the walk move for the walkers ``gids`` (global ids) whose complementary list has ``nc`` rows:
    subset [n, s0] (ascending list positions), z [n, s0] (z[:, m] belongs to row subset[:, m])."""
    gids = np.asarray(gids)
    n = len(gids)
    j = np.arange(nc)
    if s0 == nc:
        subset = np.broadcast_to(j, (n, nc)).astype(np.int32)
    else:
        r = _philox(seed, step, gids, STREAM_KEYS + 16 * np.arange((nc + 1) // 2)).astype(np.uint64)
        even = (r[..., 0] << _S32) | r[..., 1]
        odd = (r[..., 2] << _S32) | r[..., 3]
        keys = np.stack([even, odd], axis=2).reshape(n, -1)[:, :nc]
        srt = np.argsort(keys, axis=1, kind="stable")                     # ties by j
        subset = np.sort(srt[:, :s0], axis=1).astype(np.int32)
    zall = _normal(_philox(seed, step, gids, STREAM_WALK_Z + 16 * j))     # [n, nc]
    return subset, np.take_along_axis(zall, subset.astype(np.int64), axis=1)


def draw_kde_randoms(seed, step, gids, nc, d):
    """Row and normals of the KDE move: r [n] into the complementary list, z [n, d]."""
    r = _philox(seed, step, gids, STREAM_KDE + 16 * np.arange(d + 1))
    row = ((r[:, 0, 0].astype(np.uint64) * np.uint64(nc)) >> _S32).astype(np.int32)
    return row, _normal(r[:, 1:, :])


# ---------------------------------------------------------------------------------------------------------------- the rules
def walk_proposal(x, crows, z):
    """q [n, d] from the walkers x [n, d], the subset's rows crows [n, s0, d] and their normals z [n, s0], in the stated order."""
    n, s0, d = crows.shape
    mean = np.zeros((n, d))
    for m in range(s0):
        mean = mean + crows[:, m, :]
    mean = mean / float(s0)
    acc = np.zeros((n, d))
    for m in range(s0):
        acc = acc + z[:, m, None] * (crows[:, m, :] - mean)
    scale = 1.0 / np.sqrt(float(s0) - 1.0)
    return x + scale * acc


def walk_step_arrays(coords, logp, order, n0, subset, z, u_acc, lnprob_batch, margin_out=None):
    """One full red-blue walk step from pre-drawn arrays keyed by walker id (the contract of alabi_ens_step_with_randoms_walk):
    subset [W, s0] indexes the walker's complementary list, z [W, s0] holds the rows' normals.  Returns coords, logp, accepted and
    the proposals q [W, d]."""
    coords = np.array(coords, dtype=np.float64, copy=True)
    logp = np.array(logp, dtype=np.float64, copy=True)
    W, d = coords.shape
    accepted = np.zeros(W, dtype=bool)
    qall = np.full((W, d), np.nan)
    sets = [np.asarray(order[:n0]), np.asarray(order[n0:])]
    for split in range(2):
        S, Cs = sets[split], sets[1 - split]
        if len(S) == 0:
            continue
        c = coords[Cs]
        q = walk_proposal(coords[S], c[np.asarray(subset)[S]], np.asarray(z)[S])
        new_logp = np.asarray(lnprob_batch(q), dtype=np.float64)
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


def kde_prepare(c, f):
    """(mean [d], L [d, d], y [Nc, d], singular) of the complementary rows c [Nc, d] and the factor f, in the stated order."""
    nc, d = c.shape
    mean = np.zeros(d)
    for j in range(nc):
        mean = mean + c[j]
    mean = mean / float(nc)
    cc = c - mean
    s = np.zeros((d, d))
    for j in range(nc):
        s = s + cc[j][:, None] * cc[j][None, :]
    H = (f * f) * (s / (float(nc) - 1.0))
    L = np.zeros((d, d))
    for j in range(d):
        t = H[j:, j].copy()
        for k in range(j):
            t = t - L[j:, k] * L[j, k]
        piv = t[0]
        if not (piv > 0.0) or not (piv < np.inf):
            return mean, None, None, True
        ljj = np.sqrt(piv)
        L[j, j] = ljj
        L[j + 1:, j] = t[1:] / ljj
    return mean, L, whiten(L, cc), False


def whiten(L, v):
    """L^-1 v for the rows v [n, d]: forward substitution, k ascending."""
    n, d = v.shape
    y = np.zeros((n, d))
    for i in range(d):
        t = v[:, i].copy()
        for k in range(i):
            t = t - L[i, k] * y[:, k]
        y[:, i] = t / L[i, i]
    return y


def kde_proposal(x, c, mean, L, y, row, z):
    """(q [n, d], lnfac [n]) for the walkers x [n, d]: q = c[row] + L z, lnfac = kde.logpdf(x) - kde.logpdf(q)."""
    n, d = x.shape
    q = np.empty((n, d))
    for k in range(d):
        acc = np.zeros(n)
        for m in range(k + 1):
            acc = acc + L[k, m] * z[:, m]
        q[:, k] = c[row, k] + acc
    yx, yq = whiten(L, x - mean), whiten(L, q - mean)
    ex = -0.5 * np.sum((yx[:, None, :] - y[None, :, :]) ** 2, axis=2)
    eq = -0.5 * np.sum((yq[:, None, :] - y[None, :, :]) ** 2, axis=2)
    return q, logsumexp(ex, axis=1) - logsumexp(eq, axis=1)


def kde_step_arrays(coords, logp, order, n0, factors, row, z, u_acc, lnprob_batch, margin_out=None, singular_out=None,
                    hastings=True):
    """One full red-blue KDE step from pre-drawn arrays keyed by walker id (the contract of alabi_ens_step_with_randoms_kde):
    ``factors`` = (f of split 0, f of split 1) or one scalar, row [W] indexes the walker's complementary list, z [W, d].  A
    singular half step rejects all its proposals and appends its split to ``singular_out`` (a list).  ``hastings=False`` puts 0
    in the place of the log factor and exists for the negative control of the invariance test only.  Returns coords, logp,
    accepted, the proposals q [W, d] and their lnfac [W] (NaN for a singular half step)."""
    coords = np.array(coords, dtype=np.float64, copy=True)
    logp = np.array(logp, dtype=np.float64, copy=True)
    W, d = coords.shape
    factors = (float(factors), float(factors)) if np.isscalar(factors) else (float(factors[0]), float(factors[1]))
    accepted = np.zeros(W, dtype=bool)
    qall = np.full((W, d), np.nan)
    lnfac = np.full(W, np.nan)
    sets = [np.asarray(order[:n0]), np.asarray(order[n0:])]
    for split in range(2):
        S, Cs = sets[split], sets[1 - split]
        if len(S) == 0:
            continue
        c = coords[Cs]
        with np.errstate(divide="ignore", invalid="ignore"):
            mean, L, y, singular = kde_prepare(c, factors[split])
        if singular:
            if singular_out is not None:
                singular_out.append(split)
            if margin_out is not None:
                margin_out.append(np.full(len(S), -np.inf))
            continue
        q, f = kde_proposal(coords[S], c, mean, L, y, np.asarray(row)[S], np.asarray(z)[S])
        if not hastings:
            f = np.zeros_like(f)
        new_logp = np.asarray(lnprob_batch(q), dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            lnpdiff = f + new_logp - logp[S]
            acc = lnpdiff > np.log(u_acc[S])
            if margin_out is not None:
                margin_out.append(lnpdiff - np.log(u_acc[S]))
        qall[S] = q
        lnfac[S] = f
        coords[S[acc]] = q[acc]
        logp[S[acc]] = new_logp[acc]
        accepted[S[acc]] = True
    return coords, logp, accepted, qall, lnfac


# ------------------------------------------------------------------------------------------------------- emcee, literally
def emcee_literal_walk_step(coords, logp, lnprob_one, random, s=None):
    """emcee 3 RedBlueMove.propose with WalkMove.get_proposal, draw for draw from a ``RandomState``."""
    coords = np.array(coords, dtype=np.float64, copy=True)
    logp = np.array(logp, dtype=np.float64, copy=True)
    nwalkers, ndim = coords.shape
    accepted = np.zeros(nwalkers, dtype=bool)
    all_inds = np.arange(nwalkers)
    inds = all_inds % 2
    random.shuffle(inds)
    for split in range(2):
        S1 = inds == split
        sets = [coords[inds == j] for j in range(2)]
        s_ = sets[split]
        c = np.concatenate(sets[:split] + sets[split + 1:], axis=0)
        ns, nc = len(s_), len(c)
        # WalkMove.get_proposal
        q = np.empty((ns, ndim), dtype=np.float64)
        s0 = nc if s is None else s
        for i in range(ns):
            sub = random.choice(nc, s0, replace=False)
            cov = np.atleast_2d(np.cov(c[sub], rowvar=False))
            q[i] = random.multivariate_normal(s_[i], cov)
        factors = np.zeros(ns, dtype=np.float64)
        new_log_probs = np.array([float(lnprob_one(v)) for v in q])
        for i, (j, f, nlp) in enumerate(zip(all_inds[S1], factors, new_log_probs)):
            lnpdiff = f + nlp - logp[j]
            if lnpdiff > np.log(random.rand()):
                accepted[j] = True
        m = accepted[S1]
        coords[all_inds[S1][m]] = q[m]
        logp[all_inds[S1][m]] = new_log_probs[m]
    return coords, logp, accepted


def emcee_literal_kde_step(coords, logp, lnprob_one, random, bw_method=None):
    """emcee 3 RedBlueMove.propose with KDEMove.get_proposal: gaussian_kde of the complementary set, resample, the two logpdfs."""
    from scipy.stats import gaussian_kde
    coords = np.array(coords, dtype=np.float64, copy=True)
    logp = np.array(logp, dtype=np.float64, copy=True)
    nwalkers, ndim = coords.shape
    accepted = np.zeros(nwalkers, dtype=bool)
    all_inds = np.arange(nwalkers)
    inds = all_inds % 2
    random.shuffle(inds)
    for split in range(2):
        S1 = inds == split
        sets = [coords[inds == j] for j in range(2)]
        s_ = sets[split]
        c = np.concatenate(sets[:split] + sets[split + 1:], axis=0)
        ns = len(s_)
        # KDEMove.get_proposal
        kde = gaussian_kde(c.T, bw_method=bw_method)
        q = kde.resample(ns, seed=random).T
        factors = kde.logpdf(s_.T) - kde.logpdf(q.T)
        new_log_probs = np.array([float(lnprob_one(v)) for v in q])
        for i, (j, f, nlp) in enumerate(zip(all_inds[S1], factors, new_log_probs)):
            lnpdiff = f + nlp - logp[j]
            if lnpdiff > np.log(random.rand()):
                accepted[j] = True
        m = accepted[S1]
        coords[all_inds[S1][m]] = q[m]
        logp[all_inds[S1][m]] = new_log_probs[m]
    return coords, logp, accepted


# --------------------------------------------------------------------------------------------------------------- the run
def _whole_half_draws(seed, step, W, order, n0, kind, s_par, d, id0):
    """The step's walk or KDE draws, per half: [(S, (subset [|S|, s0], z [|S|, s0]))] or [(S, (row [|S|], z [|S|, d]))] with S the
    half's walker ids.  The two halves of an odd W have different Nc, so with s = all their subsets differ in size."""
    order = np.asarray(order)
    halves = [(order[:n0], W - n0), (order[n0:], n0)]
    if kind == KIND_WALK:
        out = []
        for S, nc in halves:
            s0 = nc if s_par == 0 else int(s_par)
            out.append((S, draw_walk_randoms(seed, step, S + int(id0), nc, s0)))
        return out
    out = []
    for S, nc in halves:
        out.append((S, draw_kde_randoms(seed, step, S + int(id0), nc, d)))
    return out


def _walk_step(coords, logp, order, n0, draws, u_acc, lnprob_batch, margin_out):
    """walk_step_arrays with per-half subset sizes (s = all on an odd W)."""
    coords = coords.copy(); logp = logp.copy()
    W = coords.shape[0]
    accepted = np.zeros(W, dtype=bool)
    sets = [np.asarray(order[:n0]), np.asarray(order[n0:])]
    for split in range(2):
        S, (subset, z) = draws[split]
        if len(S) == 0:
            continue
        c = coords[sets[1 - split]]
        q = walk_proposal(coords[S], c[subset], z)
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


def run_ensemble_moves(p0, nsteps, lnprob_batch, seed, moves, thin_by=1, step0=0, logp0=None, id0=0, count_moves=None,
                       margin_out=None, singular_out=None, kde_hastings=True):
    """snooker_numpy.run_ensemble_moves for all five kinds of move (``moves``: see ``move_table``): the array-driven run with the
    counter-based draws, step for step -- the device's production contract.  Returns chain, chain_logp, n_accept[W], coords,
    logp.  ``margin_out``: two arrays per step.  ``singular_out`` (a list): (step, split) of every singular KDE half step.
    ``kde_hastings``: see ``kde_step_arrays`` (the negative control of the invariance test)."""
    coords = np.array(p0, dtype=np.float64, copy=True)
    W, d = coords.shape
    kinds, cum, tp0, tp1 = move_table(moves, d, W)
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
        if kinds[mi] == 0:
            coords, logp, acc = stretch_step_arrays(coords, logp, order, n0, dr["u_z"][k], dr["partner"][k], u_acc, lnprob_batch,
                                                    tp0[mi], margin_out=margin_out)
        elif kinds[mi] == 1:
            gamma = tp0[mi] * (1.0 + tp1[mi] * dr["n"][k])
            coords, logp, acc = dm.de_step_arrays(coords, logp, order, n0, dr["partner"][k], dr["j2"][k], gamma, u_acc, lnprob_batch,
                                                  margin_out=margin_out)
        elif kinds[mi] == 2:
            coords, logp, acc, _ = sn.snooker_step_arrays(coords, logp, order, n0, dr["partner"][k], dr["j2"][k], dr["j3"][k], tp0[mi],
                                                          u_acc, lnprob_batch, margin_out=margin_out)
        elif kinds[mi] == KIND_WALK:
            draws = _whole_half_draws(seed, step0 + t, W, order, n0, KIND_WALK, tp0[mi], d, id0)
            coords, logp, acc = _walk_step(coords, logp, order, n0, draws, u_acc, lnprob_batch, margin_out)
        else:
            draws = _whole_half_draws(seed, step0 + t, W, order, n0, KIND_KDE, 0, d, id0)
            row = np.zeros(W, dtype=np.int32); z = np.zeros((W, d))
            for S, (r_, z_) in draws:
                row[S] = r_; z[S] = z_
            sing = []
            coords, logp, acc, _, _ = kde_step_arrays(coords, logp, order, n0, (tp0[mi], tp1[mi]), row, z, u_acc, lnprob_batch,
                                                      margin_out=margin_out, singular_out=sing, hastings=kde_hastings)
            if singular_out is not None:
                singular_out.extend((step0 + t, s_) for s_ in sing)
        nacc += acc
        if (t + 1) % thin_by == 0:
            chain[(t + 1) // thin_by - 1] = coords
            chain_lp[(t + 1) // thin_by - 1] = logp
    return chain, chain_lp, nacc, coords, logp
