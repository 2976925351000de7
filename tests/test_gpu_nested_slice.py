"""Random-direction slice sampling on the GPU (sample="rslice"): ns_slice_kernel against the NumPy model of the move
(tests/rslice_numpy.py) fed with the same Philox draws and the oracle GP mean, the invariants of the move, the split path around
a host likelihood, and run_dynesty's evidence with it.  Helpers copied from test_gpu_nested.py."""
import math
from functools import partial

import numpy as np
import pytest

from conftest import make_problem
from rslice_numpy import rslice

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the kernel's draws (key layout: nested.hip)
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


def replay(seed, call, walk_id0, u0, l0, lstar, chol, scale, slices, logl_fn):
    dr = PhiloxDraws(seed, call, walk_id0, u0.shape[1])
    return rslice(u0, l0, lstar, chol, scale, slices, logl_fn, dr.normals, dr.uniform)


def _oracle(N, d, kernel="ExpSquaredKernel", seed=3):
    from oracle.gp_oracle import OracleGP
    X, y, h = make_problem(N, d, seed, log_wn=-4.0)
    o = OracleGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel).compute(X)
    return X, y, h, o


def _setup(N, d, kernel="ExpSquaredKernel", seed=3):
    from alabi_amd import HipGP
    X, y, h, o = _oracle(N, d, kernel, seed)
    g = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel)
    g.compute(X)
    return g, o, y


def _starts(o, y, box, K, rng, aff=(1.0, 0.0)):
    lo, w = box[:, 0], box[:, 1] - box[:, 0]
    u = rng.random((4 * K, box.shape[0]))
    l = aff[0] * o.predict(y, lo + u * w) + aff[1]
    lstar = float(np.quantile(l, 0.5))
    keep = np.flatnonzero(l > lstar)[:K]
    return u[keep], l[keep], lstar, np.linalg.cholesky(np.cov(u.T))


REPLAY_CASES = [(400, 4, "ExpSquaredKernel", 1), (2000, 10, "ExpSquaredKernel", 1), (5000, 10, "ExpSquaredKernel", 2),
                (400, 4, "Matern52Kernel", 1), (600, 24, "ExpSquaredKernel", None), (600, 48, "Matern32Kernel", None)]
K_REPLAY, SEED_REPLAY, CALL_REPLAY, SCALE_REPLAY = 64, 0x1234_5678_9ABC, 7, 1.0


def replay_case(N, d, kernel):
    """Inputs and NumPy replay of one case (no GPU needed)."""
    X, y, h, o = _oracle(N, d, kernel)
    box = np.array([[-3.0, 3.0]] * d)
    u0, l0, lstar, chol = _starts(o, y, box, K_REPLAY, np.random.default_rng(1))
    logl_fn = lambda uu: o.predict(y, box[:, 0] + uu * (box[:, 1] - box[:, 0]))  # noqa: E731
    ref = replay(SEED_REPLAY, CALL_REPLAY, 0, u0, l0, lstar, chol, SCALE_REPLAY, 3 + d, logl_fn)
    return (X, y, h, box, u0, l0, lstar, chol), ref


@pytest.mark.parametrize("N,d,kernel,path", REPLAY_CASES)
def test_slice_kernel_matches_numpy_replay(N, d, kernel, path):
    """The last two cases run the 256-lane dimension buckets (24, 48).  Tolerances: those of test_walk_matches_numpy_replay."""
    from alabi_amd import HipGP
    from alabi_amd.nested import GPUWalkBackend
    (X, y, h, box, u0, l0, lstar, chol), (ur, lr, ner, nxr, ncr, ncapr) = replay_case(N, d, kernel)
    # the inputs exercise both loops and never reach the contraction cap (which would hide a stuck walk)
    assert ncapr.sum() == 0 and nxr.sum() >= 1 and ncr.sum() >= 1
    g = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel)
    g.compute(X)
    be = GPUWalkBackend(g, y, box, seed=SEED_REPLAY, to_theta=lambda u: u)
    u, l, nev, nexp, ncon, ncap = be.rslice(CALL_REPLAY, u0, l0, lstar, chol, SCALE_REPLAY, 3 + d)
    if path is not None:
        assert be.last_path() == path
    print(N, d, kernel, "evals", nev.sum(), ner.sum(), "exp", nexp.sum(), "con", ncon.sum(),
          "du", np.max(np.abs(u - ur)), "dl", np.max(np.abs(l - lr) / np.abs(lr)))
    assert np.array_equal(nev, ner) and np.array_equal(nexp, nxr) and np.array_equal(ncon, ncr) and np.array_equal(ncap, ncapr)
    assert np.max(np.abs(u - ur)) <= 1e-13
    assert np.max(np.abs(l - lr) / np.abs(lr)) <= 1e-12
    be.close()


def test_slice_invariants_split_launches_and_surrogate_agreement():
    import torch
    from alabi_amd import EnsembleSampler
    from alabi_amd.nested import GPUWalkBackend
    g, o, y = _setup(400, 4)
    box = np.array([[-3.0, 3.0]] * 4)
    for aff, kind in (((1.0, 0.0), None), ((2.5, -1.0), None), ((0.1, 0.2), "nlog")):
        be = GPUWalkBackend(g, y, box, seed=99, to_theta=lambda u: u, logp_affine=aff, logp_map=kind)
        ens = EnsembleSampler(16, 4, g, y, box, seed=1, logp_affine=aff, logp_map=kind)
        u0, _ = be.prior(0, 128)
        l0 = ens.surrogate(box[:, 0] + u0 * 6.0).cpu().numpy()
        lstar = float(np.quantile(l0, 0.5))
        keep = np.flatnonzero(l0 > lstar)
        chol = np.linalg.cholesky(np.cov(u0.T))
        u, l, nev, nexp, ncon, ncap = be.rslice(3, u0[keep], l0[keep], lstar, chol, 1.0, 7)
        assert np.all((u > 0) & (u < 1)) and np.all(l > lstar)
        assert ncap.sum() == 0 and np.all(nev >= 7) and np.all(u != u0[keep])
        lens = ens.surrogate(torch.as_tensor(box[:, 0] + u * 6.0, device="cuda")).cpu().numpy()
        assert np.max(np.abs(l - lens) / np.maximum(np.abs(lens), 1e-300)) <= 1e-12
        # two launches split by walk_id0 = one launch, bit for bit
        K1 = len(keep) // 3
        a = be.rslice(3, u0[keep][:K1], l0[keep][:K1], lstar, chol, 1.0, 7, walk_id0=0)
        b = be.rslice(3, u0[keep][K1:], l0[keep][K1:], lstar, chol, 1.0, 7, walk_id0=K1)
        assert np.array_equal(np.vstack([a[0], b[0]]), u) and np.array_equal(np.concatenate([a[1], b[1]]), l)
        for x, y_, full in zip(a[2:], b[2:], (nev, nexp, ncon, ncap)):
            assert np.array_equal(np.concatenate([x, y_]), full)
        # no slices: the start, bit for bit, and nothing counted
        z = be.rslice(4, u0[keep], l0[keep], lstar, chol, 1.0, 0)
        assert np.array_equal(z[0], u0[keep]) and np.array_equal(z[1], l0[keep]) and all(c.sum() == 0 for c in z[2:])
        be.close()


def test_slice_split_path_replays_the_fused_draws():
    from alabi_amd.nested import GPUWalkBackend
    g, o, y = _setup(400, 4)
    box = np.array([[-3.0, 3.0]] * 4)
    u0, l0, lstar, chol = _starts(o, y, box, 40, np.random.default_rng(4))
    logl_fn = lambda uu: o.predict(y, box[:, 0] + uu * 6.0)  # noqa: E731
    be = GPUWalkBackend(g, y, box, seed=77, to_theta=lambda u: u, host_loglike=logl_fn)
    u, l, nev, nexp, ncon, ncap = be.rslice(2, u0, l0, lstar, chol, 1.0, 7)
    ur, lr, ner, nxr, ncr, ncapr = replay(77, 2, 0, u0, l0, lstar, chol, 1.0, 7, logl_fn)
    assert np.array_equal(nev, ner) and np.array_equal(nexp, nxr) and np.array_equal(ncon, ncr) and np.array_equal(ncap, ncapr)
    assert be.host_calls == ner.sum() > 0
    assert np.max(np.abs(u - ur)) <= 1e-13
    assert np.max(np.abs(l - lr) / np.abs(lr)) <= 1e-12
    # ... and the fused kernel itself, on the same GP: same counters, u, logL
    bf = GPUWalkBackend(g, y, box, seed=77, to_theta=lambda u: u)
    uf, lf, *cf = bf.rslice(2, u0, l0, lstar, chol, 1.0, 7)
    assert all(np.array_equal(x, y_) for x, y_ in zip(cf, (nev, nexp, ncon, ncap)))
    assert np.max(np.abs(u - uf)) <= 1e-13 and np.max(np.abs(l - lf) / np.abs(lf)) <= 1e-12
    z = be.rslice(5, u0, l0, lstar, chol, 1.0, 0)
    assert np.array_equal(z[0], u0) and np.array_equal(z[1], l0)
    be.close()
    bf.close()


# ------------------------------------------------------------------------ run_dynesty
def _gauss2(theta):
    t = np.asarray(theta, dtype=float).reshape(-1, 2)
    S = np.array([[1.0, 0.4], [0.4, 0.6]])
    r = t - np.array([0.5, -0.3])
    out = -0.5 * np.einsum("ni,ij,nj->n", r, np.linalg.inv(S), r)
    return out if np.ndim(theta) == 2 else float(out[0])


@pytest.fixture(scope="module")
def sm2(tmp_path_factory):
    from alabi_amd import SurrogateModel
    sm = SurrogateModel(lnlike_fn=_gauss2, bounds=[(-4.0, 4.0), (-4.0, 4.0)], savedir=str(tmp_path_factory.mktemp("ns2s")),
                        verbose=False, random_state=3, cache=True)
    sm.init_samples(ntrain=200)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1)
    n = 1000
    g = np.linspace(-4.0, 4.0, n + 1)
    c = 0.5 * (g[1:] + g[:-1])
    XX, YY = np.meshgrid(c, c, indexing="ij")
    pts = np.stack([XX.ravel(), YY.ravel()], axis=1)
    ll = np.asarray(sm.surrogate_log_likelihood(pts))
    m = ll.max()
    w = np.exp(ll - m)
    logz_grid = m + math.log(w.sum()) + 2 * math.log(8.0 / n) - math.log(64.0)
    w /= w.sum()
    mean = w @ pts
    cov = (pts - mean).T @ ((pts - mean) * w[:, None])
    return sm, logz_grid, mean, cov


@pytest.mark.parametrize("mode", ["static", "dynamic"])
def test_rslice_evidence_2d_matches_grid(sm2, mode):
    from alabi_amd import utility as ut
    sm, logz_grid, mean, cov = sm2
    pt = partial(ut.prior_transform_uniform, bounds=sm.bounds)
    sm.run_dynesty(prior_transform=pt, mode=mode, sampler_kwargs={"seed": 11, "sample": "rslice"}, min_ess=0)
    assert sm.dynesty_path == "fused"
    assert sm.dynesty_sampler.sample == "rslice" and sm.dynesty_sampler.slices == 15
    r = sm.dynesty_results
    print(mode, r.logz[-1], logz_grid, r.logzerr[-1], r.ncall, r.niter, r.n_stuck)
    assert abs(r.logz[-1] - logz_grid) <= 3 * r.logzerr[-1] + 0.02, (r.logz[-1], logz_grid, r.logzerr[-1])
    s = sm.dynesty_samples
    sd = np.sqrt(np.diag(cov))
    assert np.all(np.abs(s.mean(0) - mean) < 0.1 * sd + 3 * sd / math.sqrt(len(s) / 10))
    assert np.allclose(np.cov(s.T), cov, atol=0.15)


def test_rslice_is_reproducible_and_takes_slices(sm2):
    sm = sm2[0]
    kw = {"seed": 21, "sample": "rslice", "slices": 6, "nlive": 100}
    sm.run_dynesty(mode="static", sampler_kwargs=kw, min_ess=0)
    assert sm.dynesty_sampler.slices == 6
    a = (sm.dynesty_samples.copy(), sm.dynesty_logz, sm.dynesty_results.ncall)
    sm.run_dynesty(mode="static", sampler_kwargs=kw, min_ess=0)
    assert np.array_equal(a[0], sm.dynesty_samples) and a[1] == sm.dynesty_logz and a[2] == sm.dynesty_results.ncall


def test_rslice_callable_likelihood_with_custom_prior_transform(tmp_path):
    from alabi_amd import SurrogateModel
    d = 5
    sig = np.array([0.5, 1.0, 2.0, 0.8, 1.2])
    lo, hi = -10 * sig, 10 * sig
    calls = []

    def like(theta):
        assert np.shape(theta) == (d,)
        calls.append(1)
        return -0.5 * float(np.sum((theta / sig) ** 2))

    def pt(u):
        return lo + np.asarray(u) * (hi - lo)
    sm = SurrogateModel(lnlike_fn=lambda t: 0.0, bounds=np.stack([lo, hi], 1), savedir=str(tmp_path), verbose=False,
                        random_state=1)
    sm.run_dynesty(like_fn=like, prior_transform=pt, mode="static", sampler_kwargs={"seed": 2, "sample": "rslice"}, min_ess=0)
    assert sm.dynesty_path == "host-callback" and sm.like_fn_name == "custom"
    r = sm.dynesty_results
    logz_true = (d / 2) * math.log(2 * math.pi) + float(np.sum(np.log(sig))) - float(np.sum(np.log(hi - lo)))
    print(r.logz[-1], logz_true, r.logzerr[-1], r.ncall, r.n_stuck)
    assert abs(r.logz[-1] - logz_true) < 3 * r.logzerr[-1], (r.logz[-1], logz_true, r.logzerr[-1])
    assert r.ncall == len(calls)
