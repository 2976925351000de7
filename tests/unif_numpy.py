"""NumPy model of the uniform-in-ellipsoids move of alabi_amd/csrc/nested_unif.hip (ns_unif_candidate + ns_unif_select_kernel),
vectorised over the candidates.  Shared by test_nested_unif_host.py (draws from a NumPy generator) and test_gpu_nested_unif.py (the
kernel's own Philox draws, so that the kernel can be replayed candidate for candidate).  Not a test module."""
import numpy as np


def candidates(ells, ids, draws, thin=True):
    """The candidates ``ids``: (u [M,d], status [M], margins).  ``draws.normals(ids) -> z [M,d]`` and ``draws.uniforms(ids) ->
    (v_ell, v_rad, v_thin)`` [M] each.  Status 0 outside the cube, 1 thinned, 2 to be evaluated.  margins: dict with ``m`` (list of
    the squared Mahalanobis radii tested against 1) and ``thin`` (v_thin q of the in-cube candidates)."""
    ids = np.asarray(ids)
    M, E, d = len(ids), len(ells), ells.centres.shape[1]
    z = draws.normals(ids)
    v_ell, v_rad, v_thin = draws.uniforms(ids)
    e = np.minimum(np.searchsorted(ells.cum, v_ell, side="right"), E - 1)      # the first index with v_ell < cum[e]
    n2 = np.zeros(M)
    for i in range(d):
        n2 = z[:, i] * z[:, i] + n2
    s = v_rad ** (1.0 / d) / np.sqrt(n2)
    u = ells.centres[e] + s[:, None] * np.einsum("nki,ni->nk", ells.axes[e], z)
    status = np.zeros(M, dtype=np.int32)
    inside = np.all((u > 0.0) & (u < 1.0), axis=1)
    q = np.ones(M)
    ms = []
    for e2 in range(E):
        y = np.einsum("ki,ni->nk", ells.inv_axes[e2], u - ells.centres[e2])
        m = np.sum(y * y, axis=1)
        other = inside & (e != e2)
        ms.append(m[other])
        q += other & (m <= 1.0)
    keep = v_thin * q < 1.0 if thin else np.ones(M, dtype=bool)
    status[inside & ~keep] = 1
    status[inside & keep] = 2
    return u, status, {"m": np.concatenate(ms) if ms else np.zeros(0), "thin": (v_thin * q)[inside]}


def select(u, logl, status, lstar, need):
    """ns_unif_select_kernel: (u_taken, logl_taken, counts[5] = taken, consumed, evaluated, outside, thinned)."""
    M = len(status)
    ok = np.flatnonzero((status == 2) & (logl > lstar))[:need]
    consumed = 0 if need <= 0 else (int(ok[-1]) + 1 if len(ok) == need else M)
    st = status[:consumed]
    return u[ok], logl[ok], np.array([len(ok), consumed, np.sum(st == 2), np.sum(st == 0), np.sum(st == 1)], dtype=np.int64)


def unif(ells, lstar, K, logl_fn, draws, cand_id0=0, chunk=256, cap=None, thin=True):
    """K points above ``lstar`` in candidate order, chunk by chunk: (u, logl, n_eval, n_cand, counts[5] summed over the chunks,
    evaluations made including discarded tails)."""
    d = ells.centres.shape[1]
    cap = max(100000, 10000 * K) if cap is None else cap
    us, ls, tot, made, cid, launched = [np.zeros((0, d))], [np.zeros(0)], np.zeros(5, dtype=np.int64), 0, cand_id0, 0
    while tot[0] < K and launched < cap:
        ids = cid + np.arange(chunk)
        u, status, _ = candidates(ells, ids, draws, thin)
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


class PhiloxUnifDraws:
    """The kernel's draws of call ``call``: normals from counter (call, id, 0, j), uniforms from (call, id, 0x80000000, 0 / 1)."""

    def __init__(self, seed, call, d):
        from nested_replay_numpy import PhiloxDraws
        self.p = PhiloxDraws(seed, call, 0, d)

    def normals(self, ids):
        return self.p.normals(np.zeros(len(ids), dtype=np.int64), np.asarray(ids))

    def uniforms(self, ids):
        from nested_replay_numpy import _philox
        from oracle import stretch_oracle as so
        ids = np.asarray(ids)
        r0 = _philox(self.p.seed, self.p.call, ids, 0x80000000, 0)
        r1 = _philox(self.p.seed, self.p.call, ids, 0x80000000, 1)
        return so.u53(r0[:, 0], r0[:, 1]), so.u53(r0[:, 2], r0[:, 3]), so.u53(r1[:, 0], r1[:, 1])


class GeneratorUnifDraws:
    """Draws from a NumPy generator (host tests: the key of a draw does not matter)."""

    def __init__(self, rng, d):
        self.rng, self.d = rng, d

    def normals(self, ids):
        return self.rng.standard_normal((len(ids), self.d))

    def uniforms(self, ids):
        v = self.rng.random((3, len(ids)))
        return v[0], v[1], v[2]


class UnifCubeBackend:
    """A NestedSampler backend in NumPy: logL(u) = ``logl_theta(lo + u (hi - lo))`` ([n,d] -> [n]), ``unif`` by the model above."""

    def __init__(self, logl_theta, lo, hi, seed=0):
        self.logl_theta = logl_theta
        self.lo, self.hi = np.asarray(lo, float), np.asarray(hi, float)
        self.ndim = len(self.lo)
        self.rng = np.random.default_rng(seed)
        self.draws = GeneratorUnifDraws(self.rng, self.ndim)

    def theta(self, u):
        return self.lo + np.asarray(u) * (self.hi - self.lo)

    def logl(self, u):
        return self.logl_theta(self.theta(u))

    def prior(self, call, n):
        u = self.rng.random((n, self.ndim))
        return u, self.logl(u)

    def unif(self, call, ells, lstar, K):
        u, l, n_eval, n_cand, _, _ = unif(ells, lstar, K, self.logl, self.draws, chunk=max(64, 4 * K))
        return u, l, n_eval, n_cand
