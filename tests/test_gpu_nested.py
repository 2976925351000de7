"""Nested sampling on the GPU: ns_walk_kernel against a NumPy replay of the same Philox draws with the oracle GP mean, the
walk invariants, and run_dynesty's evidence, calibration, callable path and outer API (alabi/core.py:2417-2787)."""
import math
import os
from functools import partial

import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ NumPy replay of the walk
def _normals(seed, call, wids, step, d):
    """z [len(wids), d] of one step: counter (call, walk id, step, pair j), Box-Muller on u53 (nested.hip)."""
    from oracle import stretch_oracle as so
    npair = (d + 1) // 2
    ctr = np.zeros((len(wids), npair, 4), dtype=np.uint64)
    ctr[..., 0] = call
    ctr[..., 1] = np.asarray(wids)[:, None]
    ctr[..., 2] = step
    ctr[..., 3] = np.arange(npair)[None, :]
    r = so.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.uint64)
    u1 = so.u53(r[..., 0], r[..., 1])
    u2 = so.u53(r[..., 2], r[..., 3])
    rad = np.sqrt(-2.0 * np.log(1.0 - u1))
    ang = 6.283185307179586 * u2
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).reshape(len(wids), 2 * npair)
    return z[:, :d]


def _replay(seed, call, walk_id0, u0, l0, lstar, chol, scale, walks, logl_fn):
    u, l = u0.copy(), l0.copy()
    K, d = u.shape
    nacc, nev = np.zeros(K, int), np.zeros(K, int)
    for s in range(walks):
        z = _normals(seed, call, walk_id0 + np.arange(K), s, d)
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


def _setup(N, d, kernel="ExpSquaredKernel", seed=3):
    from alabi_amd import HipGP
    from oracle.gp_oracle import OracleGP
    X, y, h = make_problem(N, d, seed, log_wn=-4.0)
    g = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel)
    g.compute(X)
    o = OracleGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel).compute(X)
    return g, o, y


def _starts(o, y, box, K, rng, aff=(1.0, 0.0)):
    lo, w = box[:, 0], box[:, 1] - box[:, 0]
    u = rng.random((4 * K, box.shape[0]))
    l = aff[0] * o.predict(y, lo + u * w) + aff[1]
    lstar = float(np.quantile(l, 0.5))
    keep = np.flatnonzero(l > lstar)[:K]
    return u[keep], l[keep], lstar, np.linalg.cholesky(np.cov(u.T))


@pytest.mark.parametrize("N,d,kernel,path", [(400, 4, "ExpSquaredKernel", 1), (2000, 10, "ExpSquaredKernel", 1),
                                              (5000, 10, "ExpSquaredKernel", 2), (400, 4, "Matern52Kernel", 1)])
def test_walk_matches_numpy_replay(N, d, kernel, path):
    from alabi_amd.nested import GPUWalkBackend
    g, o, y = _setup(N, d, kernel)
    box = np.array([[-3.0, 3.0]] * d)
    K, walks, seed, call = 64, 25, 0x1234_5678_9ABC, 7
    u0, l0, lstar, chol = _starts(o, y, box, K, np.random.default_rng(1))
    be = GPUWalkBackend(g, y, box, seed=seed, to_theta=lambda u: u)
    u, l, nacc, nev = be.walk(call, u0, l0, lstar, chol, 0.6, walks)
    assert be.last_path() == path
    logl_fn = lambda uu: o.predict(y, box[:, 0] + uu * (box[:, 1] - box[:, 0]))  # noqa: E731
    ur, lr, nr, er = _replay(seed, call, 0, u0, l0, lstar, chol, 0.6, walks, logl_fn)
    assert np.array_equal(nacc, nr) and np.array_equal(nev, er)
    assert nacc.sum() > 0 and (nacc == 0).sum() < K
    assert np.max(np.abs(u - ur)) <= 1e-13
    assert np.max(np.abs(l - lr) / np.abs(lr)) <= 1e-12
    be.close()


def test_walk_invariants_split_launches_and_surrogate_agreement():
    import torch
    from alabi_amd import EnsembleSampler
    from alabi_amd.nested import GPUWalkBackend
    g, o, y = _setup(400, 4)
    box = np.array([[-3.0, 3.0]] * 4)
    rng = np.random.default_rng(2)
    for aff, kind in (((1.0, 0.0), None), ((2.5, -1.0), None), ((0.1, 0.2), "nlog")):
        be = GPUWalkBackend(g, y, box, seed=99, to_theta=lambda u: u, logp_affine=aff, logp_map=kind)
        ens = EnsembleSampler(16, 4, g, y, box, seed=1, logp_affine=aff, logp_map=kind)
        u0, _ = be.prior(0, 128)
        l0 = ens.surrogate(box[:, 0] + u0 * 6.0).cpu().numpy()
        lstar = float(np.quantile(l0, 0.5))
        keep = np.flatnonzero(l0 > lstar)
        chol = np.linalg.cholesky(np.cov(u0.T))
        u, l, nacc, _ = be.walk(3, u0[keep], l0[keep], lstar, chol, 0.5, 25)
        assert np.all((u > 0) & (u < 1)) and np.all(l > lstar)
        lens = ens.surrogate(torch.as_tensor(box[:, 0] + u * 6.0, device="cuda")).cpu().numpy()
        assert np.max(np.abs(l - lens) / np.maximum(np.abs(lens), 1e-300)) <= 1e-12
        # two launches split by walk_id0 = one launch, bit for bit
        K1 = len(keep) // 3
        ua, la, na, _ = be.walk(3, u0[keep][:K1], l0[keep][:K1], lstar, chol, 0.5, 25, walk_id0=0)
        ub, lb, nb, _ = be.walk(3, u0[keep][K1:], l0[keep][K1:], lstar, chol, 0.5, 25, walk_id0=K1)
        assert np.array_equal(np.vstack([ua, ub]), u) and np.array_equal(np.concatenate([la, lb]), l)
        assert np.array_equal(np.concatenate([na, nb]), nacc)
        be.close()
    # zero accepts (every proposal leaves the cube) return the start bit for bit
    be = GPUWalkBackend(g, y, box, seed=5, to_theta=lambda u: u)
    u0, l0 = be.prior(1, 32)
    u, l, nacc, nev = be.walk(4, u0, l0, -np.inf, np.eye(4), 1e6, 10)
    assert np.all(nacc == 0) and np.array_equal(u, u0) and np.array_equal(l, l0)
    # prior draws: uniform in the cube, logL = the oracle's
    assert np.all((u0 >= 0) & (u0 < 1))
    assert np.allclose(l0, o.predict(y, box[:, 0] + u0 * 6.0), rtol=1e-12, atol=0)
    be.close()


def test_split_path_replays_the_fused_draws():
    from alabi_amd.nested import GPUWalkBackend
    g, o, y = _setup(400, 4)
    box = np.array([[-3.0, 3.0]] * 4)
    u0, l0, lstar, chol = _starts(o, y, box, 40, np.random.default_rng(4))
    logl_fn = lambda uu: o.predict(y, box[:, 0] + uu * 6.0)  # noqa: E731
    be = GPUWalkBackend(g, y, box, seed=77, to_theta=lambda u: u, host_loglike=logl_fn)
    u, l, nacc, nev = be.walk(2, u0, l0, lstar, chol, 0.6, 25)
    ur, lr, nr, er = _replay(77, 2, 0, u0, l0, lstar, chol, 0.6, 25, logl_fn)
    assert np.array_equal(nacc, nr) and np.array_equal(nev, er) and be.host_calls == er.sum()
    assert np.max(np.abs(u - ur)) <= 1e-13
    assert np.max(np.abs(l - lr) / np.abs(lr)) <= 1e-12
    be.close()


def test_walk_and_slice_bad_arguments_launch_nothing():
    import torch
    from alabi_amd import HipGP, _lib
    from alabi_amd.gp import _dev
    from alabi_amd.nested import GPUWalkBackend
    N, d, K, call = 400, 4, 8, 7
    g, o, y = _setup(N, d)
    box = np.array([[-3.0, 3.0]] * d)
    be = GPUWalkBackend(g, y, box, seed=5, to_theta=lambda u: u)
    ns, dev, lib, stream = be._ensure(), _dev(), _lib.lib(), _lib.current_stream()
    u0 = torch.as_tensor(np.random.default_rng(1).random((K, d)), device=dev)
    l0 = torch.zeros(K, dtype=torch.float64, device=dev)
    ch = torch.eye(d, dtype=torch.float64, device=dev)
    uo = torch.full((K, d), -7.0, dtype=torch.float64, device=dev)
    lo = torch.full((K,), -7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((4 * K,), -7, dtype=torch.int32, device=dev)
    good = dict(call=call, walk_id0=0, u0=_lib.ptr(u0), logl0=_lib.ptr(l0), K=K, logl_star=-1e300, chol=_lib.ptr(ch), scale=0.5,
                walks=3, u_out=_lib.ptr(uo), logl_out=_lib.ptr(lo), counts=_lib.ptr(cnt))

    def launch(fn, handle=ns, **kw):
        a = dict(good, **kw)
        return fn(handle, a["call"], a["walk_id0"], a["u0"], a["logl0"], a["K"], a["logl_star"], a["chol"], a["scale"], a["walks"],
                  a["u_out"], a["logl_out"], a["counts"], stream)
    # walk_id0 + K > 2^32 - 1 has no case: both are C ints, so the sum is at most 2^32 - 2 and that check cannot be reached
    bad = [dict(K=-1), dict(walks=-1), dict(walk_id0=-1), dict(call=-1), dict(logl_star=float("nan")), dict(u0=None),
           dict(u_out=None), dict(logl_out=None), dict(chol=None), dict(scale=0.0), dict(scale=float("inf"))]
    for fn, extra in ((lib.alabi_ns_walk, []), (lib.alabi_ns_slice, [dict(logl0=None), dict(walks=0x7FFFFFFF)])):
        for kw in bad + extra:
            assert launch(fn, **kw) == _lib.BAD_ARG, (fn.__name__, kw)
    torch.cuda.synchronize()
    assert torch.all(uo == -7.0) and torch.all(lo == -7.0) and torch.all(cnt == -7)
    none = dict(K=0, u0=None, logl0=None, chol=None, u_out=None, logl_out=None, counts=None)
    for fn in (lib.alabi_ns_walk, lib.alabi_ns_slice):
        assert launch(fn, **none) == _lib.OK
    # a GP that was never factorised: reported after the argument checks, and not at all when there is nothing to do
    bare = GPUWalkBackend(HipGP(d), None, box, seed=5, to_theta=lambda u: u, host_loglike=lambda u: np.zeros(len(u)))
    nb = bare._ensure()
    for fn in (lib.alabi_ns_walk, lib.alabi_ns_slice):
        assert launch(fn, handle=nb) == _lib.NOT_COMPUTED
        assert launch(fn, handle=nb, u0=None) == _lib.BAD_ARG
        assert launch(fn, handle=nb, **none) == _lib.OK
    torch.cuda.synchronize()
    assert torch.all(uo == -7.0) and torch.all(lo == -7.0) and torch.all(cnt == -7)
    be.close(); bare.close()


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
    sm = SurrogateModel(lnlike_fn=_gauss2, bounds=[(-4.0, 4.0), (-4.0, 4.0)], savedir=str(tmp_path_factory.mktemp("ns2")),
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
def test_evidence_2d_matches_grid(sm2, mode):
    from alabi_amd import utility as ut
    sm, logz_grid, mean, cov = sm2
    pt = partial(ut.prior_transform_uniform, bounds=sm.bounds)          # the tutorial's form: still the fused path
    sm.run_dynesty(prior_transform=pt, mode=mode, sampler_kwargs={"seed": 11}, min_ess=0)
    assert sm.dynesty_path == "fused"
    r = sm.dynesty_results
    assert abs(r.logz[-1] - logz_grid) <= 3 * r.logzerr[-1] + 0.02, (r.logz[-1], logz_grid, r.logzerr[-1])
    s = sm.dynesty_samples
    sd = np.sqrt(np.diag(cov))
    assert np.all(np.abs(s.mean(0) - mean) < 0.1 * sd + 3 * sd / math.sqrt(len(s) / 10))
    assert np.allclose(np.cov(s.T), cov, atol=0.15)


def test_logzerr_calibration_2d(sm2):
    sm, logz_grid, _, _ = sm2
    z = []
    for seed in range(8):
        sm.run_dynesty(mode="static", sampler_kwargs={"seed": 100 + seed}, min_ess=0)
        z.append((sm.dynesty_results.logz[-1] - logz_grid) / sm.dynesty_results.logzerr[-1])
    rms = float(np.sqrt(np.mean(np.square(z))))
    assert 0.4 <= rms <= 2.0, z


def test_callable_likelihood_with_custom_prior_transform(tmp_path):
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
    sm.run_dynesty(like_fn=like, prior_transform=pt, mode="static", sampler_kwargs={"seed": 2}, min_ess=0)
    assert sm.dynesty_path == "host-callback" and sm.like_fn_name == "custom"
    r = sm.dynesty_results
    logz_true = (d / 2) * math.log(2 * math.pi) + float(np.sum(np.log(sig))) - float(np.sum(np.log(hi - lo)))
    assert abs(r.logz[-1] - logz_true) < 3 * r.logzerr[-1], (r.logz[-1], logz_true, r.logzerr[-1])
    assert r.ncall == len(calls)


def test_outer_api_files_min_ess_true_and_reproducible(sm2):
    sm = sm2[0]
    sm.run_dynesty(mode="static", sampler_kwargs={"seed": 21}, min_ess=1500)
    for a in ("like_fn_name", "like_fn", "prior_transform", "prior_transform_comment", "dynesty_sampler", "dynesty_results",
              "dynesty_samples", "dynesty_logz", "dynesty_logz_err", "dynesty_samples_surrogate", "dynesty_run",
              "dynesty_runtime"):
        assert hasattr(sm, a), a
    assert sm.dynesty_run and sm.dynesty_samples.shape[0] >= 1500
    assert os.path.exists(f"{sm.savedir}/dynesty_samples_final_surrogate_iter_0.npz")
    assert os.path.exists(os.path.join(sm.savedir, sm.model_name + ".pkl"))
    a = (sm.dynesty_samples.copy(), sm.dynesty_logz)
    sm.run_dynesty(mode="static", sampler_kwargs={"seed": 21}, min_ess=1500)
    assert np.array_equal(a[0], sm.dynesty_samples) and a[1] == sm.dynesty_logz
    sm.run_dynesty(like_fn="true", mode="static", sampler_kwargs={"nlive": 60, "seed": 4}, min_ess=0, save_iter=200)
    assert sm.dynesty_samples_true is sm.dynesty_samples and sm.like_fn_name == "true"
    assert os.path.exists(f"{sm.savedir}/dynesty_samples_final_true.npz")
    assert os.path.exists(f"{sm.savedir}/dynesty_sampler_true_run1.pkl")


def test_c3_size_two_seeds_and_emcee(tmp_path):
    from alabi_amd import SurrogateModel
    d = 10
    rng = np.random.RandomState(0)
    A = rng.randn(d, d)
    prec = A @ A.T / d + 0.5 * np.eye(d)

    def like(theta):
        t = np.atleast_2d(theta)
        out = -0.5 * np.einsum("ni,ij,nj->n", t, prec, t)
        return out if np.ndim(theta) == 2 else float(out[0])
    sm = SurrogateModel(lnlike_fn=like, bounds=[(-2.0, 2.0)] * d, savedir=str(tmp_path), verbose=False, random_state=0,
                        cache=False)
    sm.init_samples(ntrain=2000)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1)
    res = []
    for seed in (1, 2):
        sm.run_dynesty(mode="static", sampler_kwargs={"nlive": 500, "seed": seed}, min_ess=0)
        res.append((sm.dynesty_logz, sm.dynesty_logz_err, sm.dynesty_samples.mean(0)))
        assert sm.dynesty_logz_err > 0 and sm.dynesty_results.status == "converged"
    assert abs(res[0][0] - res[1][0]) <= 3 * math.hypot(res[0][1], res[1][1]), res
    sm.run_emcee(nwalkers=64, nsteps=3000, min_ess=0)
    sd = sm.emcee_samples.std(0)
    # 0.1 posterior sd, plus the Monte Carlo error of the two estimates (about 3 sd / sqrt(3000))
    assert np.all(np.abs(res[0][2] - sm.emcee_samples.mean(0)) <= 0.1 * sd + 3 * sd / math.sqrt(3000)), \
        (res[0][2], sm.emcee_samples.mean(0), sd)
