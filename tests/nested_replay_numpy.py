"""NumPy replays of the nested-sampling kernels' moves from the kernels' own Philox draws (key layout: alabi_amd/csrc/nested.hip).
The walk replay and its normals are copied from test_gpu_nested.py, the draws of the slice move from test_gpu_nested_slice.py;
the slice move itself is tests/rslice_numpy.py.  Not a test module."""
import numpy as np

from rslice_numpy import rslice


def _philox(seed, c0, c1, c2, c3):
    from oracle import stretch_oracle as so
    n = len(c1)
    ctr = np.zeros((n, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = c0, c1, c2, c3
    return so.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.uint64)


class PhiloxDraws:
    def __init__(self, seed, call, walk_id0, d):
        self.seed, self.call, self.walk_id0, self.d = seed, call, walk_id0, d

    def normals(self, s, idx):
        """z [n, d]: counter (call, walk id, s, pair j), Box-Muller on u53."""
        from oracle import stretch_oracle as so
        npair = (self.d + 1) // 2
        n = len(idx)
        r = _philox(self.seed, self.call, np.repeat(self.walk_id0 + idx, npair), np.repeat(s, npair),
                    np.tile(np.arange(npair), n)).reshape(n, npair, 4)
        u1 = so.u53(r[..., 0], r[..., 1])
        u2 = so.u53(r[..., 2], r[..., 3])
        rad = np.sqrt(-2.0 * np.log(1.0 - u1))
        ang = 6.283185307179586 * u2
        z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).reshape(n, 2 * npair)
        return z[:, :self.d]

    def uniform(self, s, m, idx):
        """counter (call, walk id, 0x80000000 | s, m), value u53(r0, r1)."""
        from oracle import stretch_oracle as so
        r = _philox(self.seed, self.call, self.walk_id0 + idx, 0x80000000 | np.asarray(s, dtype=np.int64), m)
        return so.u53(r[:, 0], r[:, 1])


def replay_walk(seed, call, walk_id0, u0, l0, lstar, chol, scale, walks, logl_fn):
    """``walks`` Metropolis steps of every walk: (u, logl, n_accept, n_eval)."""
    u, l = u0.copy(), l0.copy()
    K, d = u.shape
    dr = PhiloxDraws(seed, call, walk_id0, d)
    nacc, nev = np.zeros(K, int), np.zeros(K, int)
    for s in range(walks):
        z = dr.normals(np.full(K, s), np.arange(K))
        up = u + scale * (z @ chol.T)
        inside = np.all((up > 0) & (up < 1), axis=1)
        lp = np.full(K, -np.inf)
        if inside.any():
            lp[inside] = logl_fn(up[inside])
        ok = inside & (lp > lstar)
        u[ok], l[ok] = up[ok], lp[ok]
        nacc += ok
        nev += inside
    return u, l, nacc, nev


def replay_slice(seed, call, walk_id0, u0, l0, lstar, chol, scale, slices, logl_fn):
    """``slices`` slice updates of every walk: (u, logl, n_eval, n_expand, n_contract, n_capped)."""
    dr = PhiloxDraws(seed, call, walk_id0, u0.shape[1])
    return rslice(u0, l0, lstar, chol, scale, slices, logl_fn, dr.normals, dr.uniform)
