"""NumPy model of the random-direction slice move of alabi_amd/csrc/nested.hip (ns_slice_advance), vectorised over the K walks
of a launch.  Shared by test_nested_slice_host.py (draws from a NumPy generator) and test_gpu_nested_slice.py (the kernel's own
Philox draws, so that the kernel can be replayed query for query).  Not a test module."""
import numpy as np

INIT, LEFT, RIGHT, SHRINK, DONE = 0, 1, 2, 3, 4
CAP = 64                                    # contractions after which a slice gives up (ALABI_NS_SLICE_CAP)


def rslice(u0, logl0, lstar, chol, scale, slices, logl_fn, normals, uniform):
    """``slices`` slice updates of every walk.  ``normals(s [n], idx [n]) -> z [n,d]`` and ``uniform(s [n], m [n], idx [n]) -> [n]``
    give the draws of slice s of the walks idx (m = 0: the interval offset r, m >= 1: the m-th shrink draw);
    ``logl_fn(u [n,d]) -> [n]`` is only called for points strictly inside the cube.
    Returns (u, logl, n_eval, n_expand, n_contract, n_capped)."""
    u, l = np.array(u0, dtype=np.float64), np.array(logl0, dtype=np.float64)
    K, d = u.shape
    chol_t = np.asarray(chol, dtype=np.float64).T
    phase = np.full(K, INIT)
    s, m, ncs = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, np.int64)
    tl, tr, t = np.zeros(K), np.zeros(K), np.zeros(K)
    a, up = np.zeros((K, d)), np.zeros((K, d))
    nev, nexp, ncon, ncap = (np.zeros(K, np.int64) for _ in range(4))

    def contract(i):
        neg = t[i] < 0.0
        tl[i[neg]] = t[i[neg]]
        tr[i[~neg]] = t[i[~neg]]
        ncon[i] += 1
        ncs[i] += 1

    adv = np.ones(K, dtype=bool)            # walks that advance until their next in-cube query (or their end)
    while True:
        while adv.any():
            i = np.flatnonzero(adv)
            ini = i[phase[i] == INIT]
            fin = ini[s[ini] >= slices]
            phase[fin] = DONE
            adv[fin] = False
            ini = ini[s[ini] < slices]
            if ini.size:
                z = normals(s[ini], ini)
                a[ini] = scale * (z @ chol_t) / np.sqrt(np.sum(z * z, axis=1))[:, None]
                r = uniform(s[ini], np.zeros(ini.size, np.int64), ini)
                tl[ini], tr[ini], m[ini], ncs[ini], phase[ini] = -r, 1.0 - r, 1, 0, LEFT
            i = np.flatnonzero(adv)
            ph = phase[i].copy()
            sh = i[ph == SHRINK]
            capped = sh[ncs[sh] >= CAP]
            sh = sh[ncs[sh] < CAP]
            ncap[capped] += 1
            s[capped] += 1
            phase[capped] = INIT
            if sh.size:
                t[sh] = tl[sh] + uniform(s[sh], m[sh], sh) * (tr[sh] - tl[sh])
                m[sh] += 1
            le, ri = i[ph == LEFT], i[ph == RIGHT]
            t[le], t[ri] = tl[le], tr[ri]
            act = np.concatenate([le, ri, sh])
            if not act.size:
                continue
            up[act] = u[act] + t[act, None] * a[act]
            inside = np.all((up[act] > 0.0) & (up[act] < 1.0), axis=1)
            adv[act[inside]] = False
            out = act[~inside]              # outside the cube: ends the stepping / one contraction, without an evaluation
            pho = phase[out]
            phase[out[pho == LEFT]] = RIGHT
            phase[out[pho == RIGHT]] = SHRINK
            contract(out[pho == SHRINK])
        j = np.flatnonzero(phase != DONE)
        if not j.size:
            break
        lp = np.asarray(logl_fn(up[j]), dtype=np.float64).reshape(-1)
        nev[j] += 1
        above = lp > lstar
        ph = phase[j]
        for side, edge, step, nxt in ((LEFT, tl, -1.0, RIGHT), (RIGHT, tr, 1.0, SHRINK)):
            on = ph == side
            edge[j[on & above]] += step
            nexp[j[on & above]] += 1
            phase[j[on & ~above]] = nxt
        on = ph == SHRINK
        acc = j[on & above]
        u[acc], l[acc] = up[acc], lp[on & above]
        s[acc] += 1
        phase[acc] = INIT
        contract(j[on & ~above])
        adv[j] = True
    return u, l, nev, nexp, ncon, ncap


class GeneratorDraws:
    """Draws from a NumPy generator (host tests: the key of a draw does not matter)."""

    def __init__(self, rng, d):
        self.rng, self.d = rng, d

    def normals(self, s, idx):
        return self.rng.standard_normal((len(idx), self.d))

    def uniform(self, s, m, idx):
        return self.rng.random(len(idx))


class SliceCubeBackend:
    """A NestedSampler backend in NumPy: logL(u) = ``logl_theta(lo + u (hi - lo))`` ([n,d] -> [n]), ``rslice`` by the model above."""

    def __init__(self, logl_theta, lo, hi, seed=0):
        self.logl_theta = logl_theta
        self.lo, self.hi = np.asarray(lo, float), np.asarray(hi, float)
        self.ndim = len(self.lo)
        self.rng = np.random.default_rng(seed)
        self.draws = GeneratorDraws(self.rng, self.ndim)

    def theta(self, u):
        return self.lo + np.asarray(u) * (self.hi - self.lo)

    def logl(self, u):
        return self.logl_theta(self.theta(u))

    def prior(self, call, n):
        u = self.rng.random((n, self.ndim))
        return u, self.logl(u)

    def rslice(self, call, u0, logl0, lstar, chol, scale, slices):
        return rslice(u0, logl0, lstar, chol, scale, slices, self.logl, self.draws.normals, self.draws.uniform)


def separable_gaussian(d, seed=24):
    """The high-dimensional check problem: a normalised Gaussian with sigma_k = exp(U(-1,1)) in the box +-10 sigma, so that
    log Z = -sum log(hi - lo).  Returns (logl_theta, lo, hi, log Z)."""
    sig = np.exp(np.random.default_rng(seed).uniform(-1.0, 1.0, d))
    norm = -0.5 * d * np.log(2 * np.pi) - float(np.sum(np.log(sig)))

    def logl_theta(theta):
        return norm - 0.5 * np.sum((theta / sig) ** 2, axis=1)
    return logl_theta, -10.0 * sig, 10.0 * sig, -float(np.sum(np.log(20.0 * sig)))
