"""Uniform draws inside bounding ellipsoids on the GPU (alabi_amd/csrc/nested_unif.hip): ns_unif_draw_kernel and
ns_unif_select_kernel against the NumPy model of tests/unif_numpy.py fed with the kernels' own Philox draws and the oracle GP mean,
the independence of the launch shape, the host-likelihood path, Gaussian priors, the argument checks, and run_pymultinest end to end
(alabi/core.py:2790-3238)."""
import functools
import math
import os
from functools import partial

import numpy as np
import pytest

from conftest import make_problem
from unif_numpy import PhiloxUnifDraws, candidates, select, unif

pytestmark = pytest.mark.gpu

M, K, SEED, CALL = 256, 48, 0x1234_5678_9ABC, 7
NAN = float("nan")
# The ellipsoids are fitted to prior draws above the median logL, in three groups along the first coordinate, and then shrunk
# about their centres by this factor per axis: the covariance ellipsoid that holds a uniform cloud in the cube has a radius near
# the cube's half diagonal, so the share of its volume inside the cube falls like the cube-to-ball ratio (about 5 % at d = 10, nothing in 256
# candidates at d = 24) and 256 candidates would not yield 48 points.  The replay asserts below check that the chosen geometry exercises every
# outcome; the factor is not a tolerance.
SHRINK = {4: 0.8, 10: 0.75, 24: 0.65}
CASES = [(400, 4, "ExpSquaredKernel", 1, 3), (2000, 10, "ExpSquaredKernel", 1, 3), (2049, 10, "ExpSquaredKernel", 2, 3),
         (400, 4, "Matern52Kernel", 1, 3), (600, 24, "ExpSquaredKernel", None, 3), (400, 4, "ExpSquaredKernel", 1, 1)]


@functools.lru_cache(maxsize=None)
def _oracle(N, d, kernel="ExpSquaredKernel"):
    from oracle.gp_oracle import OracleGP
    X, y, h = make_problem(N, d, 3, log_wn=-4.0)
    o = OracleGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel).compute(X)
    return X, y, h, o


def _gp(N, d, kernel="ExpSquaredKernel"):
    from alabi_amd import HipGP
    X, y, h, o = _oracle(N, d, kernel)
    g = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel)
    g.compute(X)
    return g, o, y


def _box(d):
    return np.array([[-3.0, 3.0]] * d)


def _ellipsoids(logl_fn, d, E, rng):
    """(ells, L*): E overlapping ellipsoids around prior draws above the median logL."""
    from alabi_amd.nested import Ellipsoids, bounding_ellipsoids
    u = rng.random((1500, d))
    l = logl_fn(u)
    lstar = float(np.median(l))
    up = u[l > lstar]
    up = up[np.argsort(up[:, 0])]
    parts = [bounding_ellipsoids(g, "single") for g in np.array_split(up, E)]
    g = SHRINK[d]
    ells = Ellipsoids(np.concatenate([p.centres for p in parts]), np.concatenate([p.axes * g for p in parts]),
                      np.concatenate([p.inv_axes / g for p in parts]), np.concatenate([p.logvol + d * math.log(g) for p in parts]))
    return ells, lstar


@functools.lru_cache(maxsize=None)
def unif_case(N, d, kernel, E, normal=()):
    """Inputs and NumPy replay of one case (no GPU needed): ells, L*, the logL function, and the replay of M candidates."""
    X, y, h, o = _oracle(N, d, kernel)
    box = _box(d)
    if normal:
        from alabi_amd import utility as ut
        data = [(0.5, 0.7) if k in normal else (None, None) for k in range(d)]
        theta = partial(ut.prior_transform_normal, bounds=box, data=data)
    else:
        theta = lambda u: box[:, 0] + u * (box[:, 1] - box[:, 0])  # noqa: E731
    logl_fn = lambda uu: o.predict(y, theta(uu))  # noqa: E731
    ells, lstar = _ellipsoids(logl_fn, d, E, np.random.default_rng(1))
    u, status, margins = candidates(ells, np.arange(M), PhiloxUnifDraws(SEED, CALL, d))
    logl = np.full(M, -np.inf)
    logl[status == 2] = logl_fn(u[status == 2])
    return ells, lstar, logl_fn, theta, (u, status, logl, margins)


def _assert_replay_is_decisive(ells, lstar, ref, need=K):
    u, status, logl, margins = ref
    ev = status == 2
    assert np.any(status == 0) and np.any(ev & (logl <= lstar)) and np.sum(ev & (logl > lstar)) >= need
    if len(ells) > 1:
        assert np.any(status == 1) and np.min(np.abs(margins["m"] - 1.0)) > 1e-9
        assert np.min(np.abs(margins["thin"] - 1.0)) > 1e-9
    assert np.min(np.abs(u - 0.0)) > 1e-9 and np.min(np.abs(u - 1.0)) > 1e-9
    assert np.min(np.abs(logl[ev] - lstar)) / abs(lstar) > 1e-9


def _draw(be, ells, m, cand_id0=0, call=CALL, evaluate=1):
    """One alabi_ns_unif_draw launch: (u, logl, status) on the host."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.gp import _dev
    ns, dev = be._ensure(), _dev()
    tab = [torch.as_tensor(a, device=dev) for a in (ells.centres, ells.axes, ells.inv_axes, ells.cum)]
    cu = torch.empty((m, be.ndim), dtype=torch.float64, device=dev)
    cl = torch.empty(m, dtype=torch.float64, device=dev)
    cs = torch.empty(m, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().alabi_ns_unif_draw(ns, call, cand_id0, m, evaluate, len(ells), *[_lib.ptr(t) for t in tab], _lib.ptr(cu),
                                             _lib.ptr(cl), _lib.ptr(cs), _lib.current_stream()), "alabi_ns_unif_draw")
    return cu.cpu().numpy(), cl.cpu().numpy(), cs.cpu().numpy()


def _select(be, u, logl, status, lstar, need):
    import torch
    from alabi_amd import _lib
    from alabi_amd.gp import _dev
    ns, dev = be._ensure(), _dev()
    cu, cl, cs = (torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (u, logl, status))
    uo = torch.full((max(need, 1), be.ndim), -7.0, dtype=torch.float64, device=dev)
    lo = torch.full((max(need, 1),), -7.0, dtype=torch.float64, device=dev)
    counts = torch.full((5,), -1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().alabi_ns_unif_select(ns, len(status), _lib.ptr(cu), _lib.ptr(cl), _lib.ptr(cs), float(lstar), need,
                                               _lib.ptr(uo), _lib.ptr(lo), _lib.ptr(counts), _lib.current_stream()),
               "alabi_ns_unif_select")
    c = counts.cpu().numpy()
    return uo.cpu().numpy()[:c[0]], lo.cpu().numpy()[:c[0]], c


@pytest.mark.parametrize("N,d,kernel,path,E", CASES)
def test_draw_and_select_match_numpy_replay(N, d, kernel, path, E):
    from alabi_amd.nested import GPUWalkBackend
    ells, lstar, logl_fn, _, ref = unif_case(N, d, kernel, E)
    _assert_replay_is_decisive(ells, lstar, ref)
    ur, sr, lr, _ = ref
    g, o, y = _gp(N, d, kernel)
    be = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=lambda u: u)
    u, logl, status = _draw(be, ells, M)
    if path is not None:
        assert be.last_path() == path
    assert np.array_equal(status, sr)
    assert np.max(np.abs(u - ur)) <= 1e-13
    ev = sr == 2
    assert np.all(np.isneginf(logl[~ev])) and np.max(np.abs(logl[ev] - lr[ev]) / np.abs(lr[ev])) <= 1e-12
    ut, lt, c = _select(be, u, logl, status, lstar, K)
    utr, ltr, cr = select(ur, lr, sr, lstar, K)
    assert np.array_equal(c, cr) and c[0] == K and c[1] < M
    assert np.max(np.abs(ut - utr)) <= 1e-13 and np.max(np.abs(lt - ltr) / np.abs(ltr)) <= 1e-12
    # the backend's own loop: the same points and counters
    ub, lb, n_eval, n_cand = be.unif(CALL, ells, lstar, K, chunk=M)
    assert np.array_equal(ub, ut) and np.array_equal(lb, lt) and (n_eval, n_cand) == (c[2], c[1])
    assert be.evals_launched == int(ev.sum())
    be.close()


def test_result_does_not_depend_on_the_launch_shape():
    from alabi_amd.nested import GPUWalkBackend
    N, d = 400, 4
    ells, lstar, _, _, ref = unif_case(N, d, "ExpSquaredKernel", 3)
    g, o, y = _gp(N, d)
    be = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=lambda u: u)
    u, logl, status = _draw(be, ells, M)
    parts = [_draw(be, ells, 64, cand_id0=64 * q) for q in range(4)]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), u)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), logl)
    assert np.array_equal(np.concatenate([p[2] for p in parts]), status)
    one = be.unif(CALL, ells, lstar, K, chunk=M)
    four = be.unif(CALL, ells, lstar, K, chunk=64)
    default = be.unif(CALL, ells, lstar, K)
    for other in (four, default):
        assert np.array_equal(one[0], other[0]) and np.array_equal(one[1], other[1]) and one[2:] == other[2:]
    # more points than the first chunk accepts: the search goes on into the next chunks, in candidate order
    first = int(np.sum((ref[1] == 2) & (ref[2] > lstar)))
    more = first + 20
    ub, lb, n_eval, n_cand = be.unif(CALL, ells, lstar, more, chunk=M)
    ur, lr, ne_r, nc_r, _, _ = unif(ells, lstar, more, ref_logl(N, d), PhiloxUnifDraws(SEED, CALL, d), chunk=M)
    assert len(lb) == more and n_cand > M and (n_eval, n_cand) == (ne_r, nc_r)
    assert np.max(np.abs(ub - ur)) <= 1e-13 and np.max(np.abs(lb - lr) / np.abs(lr)) <= 1e-12
    assert np.array_equal(ub[:K], one[0])
    # need = 0 takes nothing and counts nothing
    ut, lt, c = _select(be, u, logl, status, lstar, 0)
    assert len(lt) == 0 and np.array_equal(c, np.zeros(5, dtype=c.dtype))
    u0, l0, ne0, nc0 = be.unif(CALL, ells, lstar, 0)
    assert u0.shape == (0, d) and l0.shape == (0,) and (ne0, nc0) == (0, 0)
    # more asked than the candidates hold: everything is consumed
    ut, lt, c = _select(be, u, logl, status, lstar, M)
    assert c[0] == first and c[1] == M and c[2] + c[3] + c[4] == M
    be.close()


def ref_logl(N, d, kernel="ExpSquaredKernel"):
    return unif_case(N, d, kernel, 3)[2]


def test_host_likelihood_path_equals_the_fused_one():
    from alabi_amd.nested import GPUWalkBackend
    N, d = 400, 4
    ells, lstar, logl_fn, _, ref = unif_case(N, d, "ExpSquaredKernel", 3)
    g, o, y = _gp(N, d)
    fused = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=lambda u: u)
    split = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=lambda u: u, host_loglike=logl_fn)
    uf, lf, sf = _draw(fused, ells, M)
    us, ls, ss = _draw(split, ells, M, evaluate=0)
    assert np.array_equal(ss, sf) and np.array_equal(us, uf) and np.all(np.isneginf(ls))
    a = fused.unif(CALL, ells, lstar, K, chunk=M)
    b = split.unif(CALL, ells, lstar, K, chunk=M)
    assert np.array_equal(a[0], b[0]) and a[2:] == b[2:]
    assert np.max(np.abs(a[1] - b[1]) / np.abs(b[1])) <= 1e-12
    # the host evaluates every candidate of the chunk that passed the thinning test, the discarded tail included
    assert split.host_calls == int(np.sum(ref[1] == 2)) == split.evals_launched and fused.host_calls == 0
    fused.close(); split.close()


def test_gaussian_prior_coordinates():
    from alabi_amd.nested import GPUWalkBackend
    N, d, normal = 400, 4, (1, 3)
    ells, lstar, logl_fn, theta, ref = unif_case(N, d, "ExpSquaredKernel", 3, normal)
    _assert_replay_is_decisive(ells, lstar, ref)
    _, y, _, o = _oracle(N, d)
    g, _, _ = _gp(N, d)
    mean = np.array([0.5 if k in normal else NAN for k in range(d)])
    std = np.array([0.7 if k in normal else NAN for k in range(d)])
    be = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=theta, normal_prior=(mean, std))
    u, logl, n_eval, n_cand = be.unif(CALL, ells, lstar, K, chunk=M)
    utr, ltr, cr = select(ref[0], ref[2], ref[1], lstar, K)
    assert (n_eval, n_cand) == (cr[2], cr[1]) and np.max(np.abs(u - utr)) <= 1e-13
    assert np.max(np.abs(logl - o.predict(y, be.transform(u))) / np.abs(logl)) <= 1e-12
    be.close()
    # an all-NaN mean is the uniform backend bit for bit
    ells, lstar, _, _, _ = unif_case(N, d, "ExpSquaredKernel", 3)
    nan4 = np.full(d, NAN)
    a = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=lambda v: v)
    b = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=lambda v: v, normal_prior=(nan4, nan4))
    ra, rb = a.unif(CALL, ells, lstar, K, chunk=M), b.unif(CALL, ells, lstar, K, chunk=M)
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and ra[2:] == rb[2:]
    a.close(); b.close()


def test_bad_arguments_launch_nothing():
    import torch
    from alabi_amd import _lib
    from alabi_amd.gp import _dev
    from alabi_amd.nested import GPUWalkBackend
    N, d = 400, 4
    ells, _, _, _, _ = unif_case(N, d, "ExpSquaredKernel", 3)
    g, o, y = _gp(N, d)
    be = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=lambda u: u)
    ns, dev, lib = be._ensure(), _dev(), _lib.lib()
    tab = [torch.as_tensor(a, device=dev) for a in (ells.centres, ells.axes, ells.inv_axes, ells.cum)]
    cu = torch.full((8, d), -7.0, dtype=torch.float64, device=dev)
    cl = torch.full((8,), -7.0, dtype=torch.float64, device=dev)
    cs = torch.full((8,), -7, dtype=torch.int32, device=dev)
    out = (_lib.ptr(cu), _lib.ptr(cl), _lib.ptr(cs), _lib.current_stream())
    tp = [_lib.ptr(t) for t in tab]
    for E in (0, 33, -1):
        assert lib.alabi_ns_unif_draw(ns, CALL, 0, 8, 1, E, *tp, *out) == _lib.BAD_ARG
    assert lib.alabi_ns_unif_draw(ns, CALL, 0, -1, 1, 3, *tp, *out) == _lib.BAD_ARG
    for k in range(4):
        holed = list(tp)
        holed[k] = None
        assert lib.alabi_ns_unif_draw(ns, CALL, 0, 8, 1, 3, *holed, *out) == _lib.BAD_ARG
    torch.cuda.synchronize()
    assert torch.all(cu == -7.0) and torch.all(cl == -7.0) and torch.all(cs == -7)
    assert lib.alabi_ns_unif_select(ns, 8, _lib.ptr(cu), _lib.ptr(cl), _lib.ptr(cs), NAN, 1, _lib.ptr(cu), _lib.ptr(cl), _lib.ptr(cs),
                                    _lib.current_stream()) == _lib.BAD_ARG
    assert lib.alabi_ns_unif_draw(ns, CALL, 0, 0, 1, 3, *tp, None, None, None, _lib.current_stream()) == _lib.OK
    be.close()


# -------------------------------------------------------------------------------------------------------- run_pymultinest
def _gauss2(theta):
    t = np.asarray(theta, dtype=float).reshape(-1, 2)
    S = np.array([[1.0, 0.4], [0.4, 0.6]])
    r = t - np.array([0.5, -0.3])
    out = -0.5 * np.einsum("ni,ij,nj->n", r, np.linalg.inv(S), r)
    return out if np.ndim(theta) == 2 else float(out[0])


def _two_modes(theta):
    t = np.asarray(theta, dtype=float).reshape(-1, 2)
    a = -0.5 * np.sum((t - np.array([2.0, 0.0])) ** 2, axis=1) / 0.5
    b = -0.5 * np.sum((t + np.array([2.0, 0.0])) ** 2, axis=1) / 0.5
    out = np.logaddexp(a, b)
    return out if np.ndim(theta) == 2 else float(out[0])


def _grid_logz(sm, half, n=800):
    """log Z of the surrogate itself under the uniform prior on [-half, half]^2 (midpoint rule), and the mass at x0 > 0."""
    gx = np.linspace(-half, half, n + 1)
    c = 0.5 * (gx[1:] + gx[:-1])
    XX, YY = np.meshgrid(c, c, indexing="ij")
    pts = np.stack([XX.ravel(), YY.ravel()], axis=1)
    ll = np.asarray(sm.surrogate_log_likelihood(pts))
    m = ll.max()
    w = np.exp(ll - m)
    return m + math.log(w.sum()) - 2 * math.log(n), float(np.sum(w[pts[:, 0] > 0]) / w.sum())


def _model(fn, half, tmp, seed):
    from alabi_amd import SurrogateModel
    sm = SurrogateModel(lnlike_fn=fn, bounds=[(-half, half), (-half, half)], savedir=str(tmp), verbose=False, random_state=seed,
                        cache=True)
    sm.init_samples(ntrain=200)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1)
    return sm


def test_run_pymultinest_evidence_files_and_reproducibility(tmp_path):
    sm = _model(_gauss2, 4.0, tmp_path, 3)
    logz_grid, _ = _grid_logz(sm, 4.0)
    kw = {"n_live_points": 400, "seed": 11, "evidence_tolerance": 0.1}
    sm.run_pymultinest(sampler_kwargs=kw, min_ess=0)
    assert sm.pymultinest_run and sm.pymultinest_path == "fused" and sm.pymultinest_analyzer is None
    r = sm.pymultinest_results
    assert r.status == "converged" and r.ncall / r.niter < 25
    assert sm.pymultinest_logz == r.logz[-1] and sm.pymultinest_logz_err == r.logzerr[-1]
    assert abs(r.logz[-1] - logz_grid) <= 3 * r.logzerr[-1], (r.logz[-1], logz_grid, r.logzerr[-1])
    s = sm.pymultinest_samples
    assert s.shape[1] == 2 and np.array_equal(sm.pymultinest_weights, np.ones(len(s))) and sm.pymultinest_samples_surrogate is s
    assert sm.pymultinest_runtime > 0
    f = np.load(f"{sm.savedir}/pymultinest_samples_final_surrogate_iter_0.npz")
    assert sorted(f.files) == ["logz", "logz_err", "samples", "weights"] and np.array_equal(f["samples"], s)
    first = (s.copy(), sm.pymultinest_logz)
    sm.run_pymultinest(sampler_kwargs=kw, min_ess=0)
    assert np.array_equal(first[0], sm.pymultinest_samples) and first[1] == sm.pymultinest_logz
    # min_ess: further runs, combined with sample-count weights
    sm.run_pymultinest(sampler_kwargs={"n_live_points": 100, "seed": 5}, min_ess=1500, samples_file="mn.npz")
    assert sm.pymultinest_samples.shape[0] >= 1500 and os.path.exists(f"{sm.savedir}/mn.npz")
    assert sm.pymultinest_logz_err > 0


def test_run_pymultinest_two_modes(tmp_path):
    sm = _model(_two_modes, 4.0, tmp_path, 4)
    logz_grid, mass_grid = _grid_logz(sm, 4.0)
    sm.run_pymultinest(sampler_kwargs={"n_live_points": 400, "seed": 3, "evidence_tolerance": 0.1}, min_ess=0)
    r = sm.pymultinest_results
    assert sm.pymultinest_path == "fused" and r.status == "converged"
    assert abs(r.logz[-1] - logz_grid) <= 3 * r.logzerr[-1], (r.logz[-1], logz_grid, r.logzerr[-1])
    w = r.importance_weights()
    mass = float(np.sum(w[r.samples[:, 0] > 0]) / np.sum(w))
    assert abs(mass_grid - 0.5) < 0.03 and abs(mass - 0.5) <= 0.06, (mass, mass_grid)
    assert max(sm.pymultinest_sampler.n_ellipsoids) >= 2


def test_run_pymultinest_true_likelihood_with_custom_prior_transform(tmp_path):
    from alabi_amd import SurrogateModel
    sig = np.array([0.5, 1.0, 2.0])
    lo, hi = -10 * sig, 10 * sig
    calls = []

    def like(theta):
        assert np.shape(theta) == (3,)
        calls.append(1)
        return -0.5 * float(np.sum((theta / sig) ** 2))

    def pt(u):
        return lo + np.asarray(u) * (hi - lo)
    sm = SurrogateModel(lnlike_fn=like, bounds=np.stack([lo, hi], 1), savedir=str(tmp_path), verbose=False, random_state=1)
    sm.run_pymultinest(like_fn="true", prior_transform=pt, sampler_kwargs={"n_live_points": 200, "seed": 2}, min_ess=0)
    assert sm.pymultinest_path == "host-callback" and sm.like_fn_name == "true" and sm.pymultinest_samples_true is sm.pymultinest_samples
    r = sm.pymultinest_results
    logz_true = 1.5 * math.log(2 * math.pi) + float(np.sum(np.log(sig))) - float(np.sum(np.log(hi - lo)))
    assert abs(r.logz[-1] - logz_true) <= 3 * r.logzerr[-1], (r.logz[-1], logz_true, r.logzerr[-1])
    assert len(calls) >= r.ncall and os.path.exists(f"{sm.savedir}/pymultinest_samples_final_true.npz")
