"""fp64 statement of the HMC move (``alabi_amd.moves.HMCMove``, kind 6 of the library's move table): the CPU statement that
ens_hmc_kernel (alabi_amd/csrc/ens_hmc.hip) is tested against.  Plain NumPy, no fma emulation: the device's sums run in another
order, so HMC proposals are compared to a tolerance, not bit for bit.  Built on tests/gaussian_move_numpy.py's draw helpers and on
oracle.utility_oracle.analytic_predict_grad's ``dmu``, which it leaves as they are.

One step for walker x with lp = lnp(x), g = grad lnp(x), C lower triangular with C C^T = cov (the mass matrix is cov^-1), in
whitened momentum z:

    z0 ~ N(0, I_d)                      e = step_size f   (f = 1, or exp(v), v ~ U(-ln jitter, ln jitter): one draw per step and ensemble)
    z = z0 + (e / 2) C^T g
    n_leapfrog times:   q = q + e C z (from q = x);   (lp_q, g_q) = lnp, grad lnp at q;   z = z + e C^T g_q   (e / 2 the last time)
    accept iff  lp_q - |z|^2 / 2 - lp + |z0|^2 / 2  >  ln u'   and q lies in the open box   (NaN anywhere rejects)

lnp is the fused log-probability WITHOUT the box gate (the trajectory follows the surrogate's smooth extension; only the end point
is tested): a mu + b with mu the GP mean, through the y map (nlog: -10^., log: 10^.), plus the normal priors.  Its gradient is the
chain rule: a dmu, times ln10 L under either map, minus (q_k - m_k) / s_k^2 per normal-prior coordinate.

Draws.  Philox counter (step, global walker id, stream word), word = S + 16 b; streams 0-10 are those of the other moves:
    S = 2, b = 0:    the accept uniform u' = u53(r0, r1), at the walker                       (as for every move)
    S = 3, b = 0:    the step's move, at the ensemble's walker 0                              (as for every move)
    S = 11, b = k:   z0_k = sqrt(-2 ln(1 - u53(r0, r1))) cos(2 pi u53(r2, r3)), at the walker (Box-Muller as stream 4)
    S = 12, b = 0:   v = (2 u53(r0, r1) - 1) ln jitter, at the ensemble's walker 0; not drawn when jitter is None
ln jitter is the value the library's table carries: rounded to a multiple of 2^-36 (``ln_jitter``).
"""
from __future__ import annotations

import numpy as np

import gaussian_move_numpy as gm
from oracle.stretch_oracle import u53
from oracle.utility_oracle import analytic_predict_grad

wk = gm.wk
STREAM_HMC_Z, STREAM_HMC_JITTER = 11, 12
KIND_HMC = 6
LN10 = float(np.log(10.0))


def ln_jitter(jitter):
    return 0.0 if jitter is None else float(np.round(np.log(float(jitter)) * 2.0 ** 36) / 2.0 ** 36)


def default_step_size(d):
    return float(d) ** -0.25


def move_table(moves, ndim):
    """``moves``: [(cov, step_size or None, n_leapfrog, jitter or None, weight)] -> kinds, cum, p0, p1, [(C, diagonal)]."""
    w = np.asarray([m[4] for m in moves], dtype=np.float64)
    p0 = np.asarray([default_step_size(ndim) if m[1] is None else float(m[1]) for m in moves])
    p1 = np.asarray([float(m[2]) + ln_jitter(m[3]) / 512.0 for m in moves])
    return np.full(len(moves), KIND_HMC), np.cumsum(w / w.sum()), p0, p1, [gm.scale_factor(m[0], ndim) for m in moves]


# ------------------------------------------------------------------------------------------------------------- the target
class GPTarget:
    """The fused log-probability of a problem of tests/moves_shapes_common.py and its gradient, without the box gate.
    ``affine`` = (a, b); ``ymap`` None / "nlog" / "log"; ``prior`` = (mean[d], std[d]) with NaN where there is none."""

    def __init__(self, prob, affine=(1.0, 0.0), ymap=None, prior=None):
        self.prob, self.affine, self.ymap, self.prior = prob, (float(affine[0]), float(affine[1])), ymap, prior
        self.bounds = prob.bounds
        self.y_std = float(np.std(prob.y))

    def inside(self, q):
        return np.all((q > self.bounds[:, 0]) & (q < self.bounds[:, 1]), axis=1)

    def value_grad(self, q):
        """(lnp [n], grad [n, d], GP mean [n]) at q [n, d]."""
        q = np.atleast_2d(np.asarray(q, dtype=np.float64))
        mu, _, dmu, _ = analytic_predict_grad(self.prob.oracle, self.prob.y, q)
        a, b = self.affine
        L = a * mu + b
        g = a * dmu
        if self.ymap is not None:
            L = (-1.0 if self.ymap == "nlog" else 1.0) * 10.0 ** L
            g = LN10 * L[:, None] * g
        if self.prior is not None:
            pm, ps = self.prior
            for k in np.nonzero(np.isfinite(pm) & np.isfinite(ps) & (ps > 0))[0]:
                t = (q[:, k] - pm[k]) / ps[k]
                L = L + (-0.5 * t * t - np.log(ps[k]) - 0.9189385332046727)
                g[:, k] = g[:, k] - (q[:, k] - pm[k]) / ps[k] ** 2
        return L, g, mu

    def __call__(self, q):
        """The gated log-probability (what compute_log_prob returns): -inf outside the open box."""
        q = np.atleast_2d(np.asarray(q, dtype=np.float64))
        ins = self.inside(q)
        out = np.full(len(q), -np.inf)
        if ins.any():
            out[ins] = self.value_grad(q[ins])[0]
        return out

    def gated_value_grad(self, q):
        """alabi_ens_log_prob_grad's contract: -inf and a zero gradient outside the open box."""
        L, g, _ = self.value_grad(q)
        ins = self.inside(np.atleast_2d(q))
        return np.where(ins, L, -np.inf), np.where(ins[:, None], g, 0.0)


class GaussianTarget:
    """An analytic Gaussian N(mean, cov) in a box (the invariance tests)."""

    def __init__(self, mean, cov, bounds):
        self.mean, self.prec, self.bounds, self.y_std = np.asarray(mean, float), np.linalg.inv(cov), np.asarray(bounds, float), 1.0

    def inside(self, q):
        return np.all((q > self.bounds[:, 0]) & (q < self.bounds[:, 1]), axis=1)

    def value_grad(self, q):
        r = q - self.mean
        g = -r @ self.prec
        L = 0.5 * np.einsum("nk,nk->n", r, g)
        return L, g, L


# ---------------------------------------------------------------------------------------------------------------- the rule
def leapfrog(target, x, g, C, e, z0, L):
    """(q, z, lp_q, g_q, mu_q) after L leapfrog steps from (x, z0) with the gradient g at x."""
    z = z0 + (0.5 * e) * (g @ C)                      # C^T g, row-wise
    q = np.array(x, dtype=np.float64, copy=True)
    lpq = gq = mu = None
    for l in range(L):
        q = q + e * (z @ C.T)                         # C z
        lpq, gq, mu = target.value_grad(q)
        z = z + (0.5 * e if l == L - 1 else e) * (gq @ C)
    return q, z, lpq, gq, mu


def hmc_step_arrays(target, coords, logp, grad, C, e, z0, L, u_acc, record=None):
    """One HMC step of every walker from pre-drawn arrays keyed by walker id (the contract of alabi_ens_step_with_randoms_hmc).
    ``record`` (a dict of lists): appends the accept-test margins, the end points' inside flags and their GP means.
    Returns coords, logp, grad, accepted."""
    with np.errstate(all="ignore"):
        q, z, lpq, gq, mu = leapfrog(target, coords, grad, C, e, z0, L)
        dh = lpq - 0.5 * np.sum(z * z, axis=1) - logp + 0.5 * np.sum(z0 * z0, axis=1)
        margin = dh - np.log(u_acc)
        ins = target.inside(q)
        acc = ins & (margin > 0)
    if record is not None:
        record.setdefault("margin", []).append(margin); record.setdefault("inside", []).append(ins)
        record.setdefault("mu", []).append(mu[ins])
    coords = np.where(acc[:, None], q, coords)
    return coords, np.where(acc, lpq, logp), np.where(acc[:, None], gq, grad), acc


def stats(record, target):
    """moves_shapes_common.stats for an HMC run: the smallest |margin| of an in-box accept test, the three outcomes, the spread
    of the GP mean over the in-box end points relative to y (``assert_honest``'s terms)."""
    m = np.concatenate(record["margin"]); ins = np.concatenate(record["inside"]); mu = np.concatenate(record["mu"])
    assert not np.any(np.isnan(m[ins]))
    return dict(min_margin=float(np.min(np.abs(m[ins]))) if ins.any() else np.inf, n_acc=int(np.sum(ins & (m > 0))),
                n_rej_in=int(np.sum(ins & ~(m > 0))), n_out=int(np.sum(~ins)),
                mu_spread=float(np.std(mu) / target.y_std) if len(mu) > 1 else 0.0)


# --------------------------------------------------------------------------------------------------------------- the draws
def draw_hmc_randoms(seed, step, gids, g0, cum, p0, p1, d):
    """The production draws of one step for the walkers ``gids`` of the ensemble whose walker 0 is ``g0``: the move's index, e,
    z0 [n, d] and u' [n]."""
    gids = np.asarray(gids)
    mi = 0
    if len(cum) > 1:
        r = wk._philox(seed, step, [int(g0)], [3])[0, 0]
        mi = min(int(np.sum(np.asarray(cum) <= u53(r[0], r[1]))), len(cum) - 1)
    lnj = (p1[mi] - np.floor(p1[mi])) * 512.0
    e = float(p0[mi])
    if lnj != 0.0:
        r = wk._philox(seed, step, [int(g0)], [STREAM_HMC_JITTER])[0, 0]
        e = float(p0[mi] * np.exp((2.0 * u53(r[0], r[1]) - 1.0) * lnj))
    z0 = wk._normal(wk._philox(seed, step, gids, STREAM_HMC_Z + 16 * np.arange(d)))
    r = wk._philox(seed, step, gids, [2])[:, 0, :]
    return mi, e, z0, u53(r[:, 0], r[:, 1])


# ----------------------------------------------------------------------------------------------------------------- the run
def run_hmc(target, p0, nsteps, seed, moves, thin_by=1, step0=0, logp0=None, id0=0, count_moves=None, record=None):
    """The run with the counter-based draws, step for step -- the device's production contract.  ``moves``: see ``move_table``.
    Returns chain, chain_logp, n_accept [W], coords, logp."""
    coords = np.array(p0, dtype=np.float64, copy=True)
    W, d = coords.shape
    _, cum, tp0, tp1, scales = move_table(moves, d)
    logp = np.asarray(target(coords), dtype=np.float64) if logp0 is None else np.array(logp0, dtype=np.float64)
    grad = target.value_grad(coords)[1]
    nstore = nsteps // thin_by
    chain, chain_lp = np.empty((nstore, W, d)), np.empty((nstore, W))
    nacc = np.zeros(W, dtype=np.int64)
    for t in range(nsteps):
        mi, e, z0, u = draw_hmc_randoms(seed, step0 + t, np.arange(W) + int(id0), id0, cum, tp0, tp1, d)
        if count_moves is not None:
            count_moves[mi] = count_moves.get(mi, 0) + 1
        coords, logp, grad, acc = hmc_step_arrays(target, coords, logp, grad, scales[mi][0], e, z0, int(np.floor(tp1[mi])), u, record)
        nacc += acc
        if (t + 1) % thin_by == 0:
            chain[(t + 1) // thin_by - 1] = coords
            chain_lp[(t + 1) // thin_by - 1] = logp
    return chain, chain_lp, nacc, coords, logp
