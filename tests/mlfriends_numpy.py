"""NumPy model of the MLFriends region of alabi_amd/csrc/nested_mlf.hip (ns_mlf_radius_kernel and the neighbour test of
ns_mlf_draw_kernel) on top of the ellipsoid move of tests/unif_numpy.py.  Shared by test_mlfriends_host.py (draws from a NumPy
generator) and test_gpu_mlfriends.py (the kernels' own Philox draws, so that they can be replayed round for round and candidate for
candidate).  Not a test module."""
import numpy as np

from unif_numpy import GeneratorUnifDraws, candidates, select

MLF_STEP = 0x80000001


def metric(points, ells):
    """(labels, metric_inv, w) as nested.mlfriends_metric states it, written out independently: the covariance of the points about
    the centre of their own ellipsoid, pooled with n - E degrees of freedom, its Cholesky factor inverted."""
    p = np.asarray(points, dtype=np.float64)
    n, E = p.shape[0], len(ells)
    m = np.stack([np.sum(np.einsum("ki,ni->nk", ells.inv_axes[e], p - ells.centres[e]) ** 2, axis=1) for e in range(E)])
    labels = np.argmin(m, axis=0)
    S = np.zeros((p.shape[1], p.shape[1]))
    for e in range(E):
        r = p[labels == e] - ells.centres[e]
        S += r.T @ r
    L = np.linalg.cholesky(S / (n - E))
    metric_inv = np.tril(np.linalg.inv(L))
    return labels, metric_inv, p @ metric_inv.T


def dist2(a, b):
    """|a_i - b_j|^2 [na, nb], accumulated in coordinate order as the kernels do."""
    s = np.zeros((a.shape[0], b.shape[0]))
    for k in range(a.shape[1]):
        t = a[:, k][:, None] - b[:, k][None, :]
        s = t * t + s
    return s


class PhiloxIndexDraws:
    """Round b's n indices from the kernel's stream: counter (call, b, 0x80000001, k), v = u53(r0, r1)."""

    def __init__(self, seed, call):
        self.seed, self.call = seed, call

    def indices(self, b, n):
        from nested_replay_numpy import _philox
        from oracle import stretch_oracle as so
        r = _philox(self.seed, self.call, np.full(n, b, dtype=np.int64), MLF_STEP, np.arange(n))
        return np.minimum(np.floor(so.u53(r[:, 0], r[:, 1]) * n).astype(np.int64), n - 1)


class GeneratorIndexDraws:
    def __init__(self, rng):
        self.rng = rng

    def indices(self, b, n):
        return np.minimum(np.floor(self.rng.random(n) * n).astype(np.int64), n - 1)


def radius2_rounds(w, B, draws):
    """(r2 [B], left_out [B]): per bootstrap round the largest squared distance from a point left out to the nearest point drawn
    (0 when none is left out), and the number of points left out."""
    w = np.asarray(w, dtype=np.float64)
    n = w.shape[0]
    D = dist2(w, w)
    r2, left = np.zeros(B), np.zeros(B, dtype=np.int64)
    for b in range(B):
        sel = np.zeros(n, dtype=bool)
        sel[draws.indices(b, n)] = True
        left[b] = int(np.sum(~sel))
        if left[b]:
            r2[b] = float(np.max(np.min(D[~sel][:, sel], axis=1)))
    return r2, left


def neighbour_margins(u, w, metric_inv, r2):
    """min_j |metric_inv u - w_j|^2 / r2 - 1 for every row of ``u``: <= 0 means a live point within r."""
    return nearest2(u, w, metric_inv) / r2 - 1.0


def nearest2(u, w, metric_inv):
    """min_j |metric_inv u - w_j|^2 for every row of ``u``."""
    u = np.asarray(u, dtype=np.float64).reshape(-1, w.shape[1])
    return np.min(dist2(u @ np.tril(metric_inv).T, w), axis=1) if len(u) else np.zeros(0)


def mlf_candidates(ells, ids, draws, w, metric_inv, r2):
    """The candidates ``ids`` with the neighbour test: (u, status, margins); margins gains ``unif_status`` (the status without the
    test) and ``near2`` (the squared distance to the nearest live point of the candidates that status was 2 for)."""
    u, status, margins = candidates(ells, ids, draws)
    two = status == 2
    near2 = nearest2(u[two], w, metric_inv)
    margins = dict(margins, unif_status=status.copy(), near2=near2)
    status = status.copy()
    status[np.flatnonzero(two)[~(near2 <= r2)]] = 1
    return u, status, margins


def mlfriends(ells, w, metric_inv, r2, lstar, K, logl_fn, draws, cand_id0=0, chunk=256, cap=None):
    """unif_numpy.unif with the neighbour test: (u, logl, n_eval, n_cand, counts[5], evaluations made)."""
    d = ells.centres.shape[1]
    cap = max(100000, 10000 * K) if cap is None else cap
    us, ls, tot, made, cid, launched = [np.zeros((0, d))], [np.zeros(0)], np.zeros(5, dtype=np.int64), 0, cand_id0, 0
    while tot[0] < K and launched < cap:
        u, status, _ = mlf_candidates(ells, cid + np.arange(chunk), draws, w, metric_inv, r2)
        logl = np.full(chunk, -np.inf)
        ev = status == 2
        if ev.any():
            logl[ev] = logl_fn(u[ev])
        made += int(ev.sum())
        ut, lt, c = select(u, logl, status, lstar, K - tot[0])
        us.append(ut); ls.append(lt)
        tot += c
        cid += chunk
        launched += chunk
    return np.vstack(us), np.concatenate(ls), int(tot[2]), int(tot[1]), tot, made


class MLFriendsCubeBackend:
    """A NestedSampler backend in NumPy: logL(u) = ``logl_theta(lo + u (hi - lo))``; ``unif`` and ``mlfriends`` by the models, from
    one generator, so that the two moves can be compared on the same backend class and settings."""

    def __init__(self, logl_theta, lo, hi, seed=0):
        self.logl_theta = logl_theta
        self.lo, self.hi = np.asarray(lo, float), np.asarray(hi, float)
        self.ndim = len(self.lo)
        self.rng = np.random.default_rng(seed)
        self.draws = GeneratorUnifDraws(self.rng, self.ndim)
        self.index_draws = GeneratorIndexDraws(self.rng)

    def theta(self, u):
        return self.lo + np.asarray(u) * (self.hi - self.lo)

    def logl(self, u):
        return self.logl_theta(self.theta(u))

    def prior(self, call, n):
        u = self.rng.random((n, self.ndim))
        return u, self.logl(u)

    def unif(self, call, ells, lstar, K):
        from unif_numpy import unif
        u, l, n_eval, n_cand, _, _ = unif(ells, lstar, K, self.logl, self.draws, chunk=max(64, 4 * K))
        return u, l, n_eval, n_cand

    def mlf_radius(self, call, w, B):
        return float(np.max(radius2_rounds(w, B, self.index_draws)[0]))

    def mlfriends(self, call, ells, w, metric_inv, r2, lstar, K):
        u, l, n_eval, n_cand, _, _ = mlfriends(ells, w, metric_inv, r2, lstar, K, self.logl, self.draws, chunk=max(64, 4 * K))
        return u, l, n_eval, n_cand
