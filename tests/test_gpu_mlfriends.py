"""The MLFriends region on the GPU (alabi_amd/csrc/nested_mlf.hip): ns_mlf_radius_kernel against the NumPy model of
tests/mlfriends_numpy.py fed the kernel's own Philox draws, ns_mlf_draw_kernel + ns_unif_select_kernel against the replay of the
same candidates with the oracle GP mean, the two limits of the radius, the independence of the launch shape, the host-likelihood
path, Gaussian priors, the argument checks, and run_ultranest end to end (alabi/core.py:3241-3690).  Shapes, seeds and the six GP
cases are those of test_gpu_nested_unif.py."""
import functools
import math
import os

import numpy as np
import pytest

import mlfriends_numpy as mn
from test_gpu_nested_unif import (CALL, CASES, K, M, SEED, _assert_replay_is_decisive, _box, _gauss2, _gp, _grid_logz, _model,
                                  _oracle, _select, _two_modes, unif_case)
from unif_numpy import PhiloxUnifDraws, select

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
NLIVE = 200
RADIUS_CASES = [(1, 2, 1), (63, 4, 30), (64, 4, 30), (65, 10, 30), (300, 10, 30), (1025, 24, 3), (300, 64, 2)]


def _bare_backend(d, seed=SEED):
    """A backend whose handle owns no training set: enough for the radius and for evaluate = 0."""
    from alabi_amd import HipGP
    from alabi_amd.nested import GPUWalkBackend
    return GPUWalkBackend(HipGP(d), np.zeros(1), _box(d), seed=seed, to_theta=lambda u: u, host_loglike=lambda u: np.zeros(len(u)))


def _radius_rounds(be, w, B, call=CALL):
    """One alabi_ns_mlf_radius launch: the B values on the host."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.gp import _dev
    ns, dev = be._ensure(), _dev()
    wd = torch.as_tensor(np.ascontiguousarray(w), device=dev)
    out = torch.full((B,), -7.0, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().alabi_ns_mlf_radius(ns, call, int(wd.shape[0]), _lib.ptr(wd), B, _lib.ptr(out), _lib.current_stream()),
               "alabi_ns_mlf_radius")
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def radius_case(n, d, B):
    """Whitened points and the model's rounds from the kernel's own draws (no GPU needed)."""
    w = np.random.default_rng(n + d).standard_normal((n, d))
    r2, left = mn.radius2_rounds(w, B, mn.PhiloxIndexDraws(SEED, CALL))
    return w, r2, left


@pytest.mark.parametrize("n,d,B", RADIUS_CASES)
def test_radius_matches_the_model_fed_the_kernels_draws(n, d, B):
    w, ref, left = radius_case(n, d, B)
    assert np.all(left > 0) if n > 1 else (np.all(left == 0) and np.all(ref == 0.0))
    be = _bare_backend(d)
    got = _radius_rounds(be, w, B)
    again = _radius_rounds(be, w, B)
    assert np.array_equal(got, again)
    if n > 1:
        assert np.max(np.abs(got - ref) / ref) <= 1e-13
    else:
        assert np.array_equal(got, ref)
    assert be.mlf_radius(CALL, w, B) == np.max(got)
    be.close()


# ---------------------------------------------------------------------------------------------------------- draw and select
@functools.lru_cache(maxsize=None)
def mlf_case(N, d, kernel, E, normal=()):
    """The unif case plus the region (no GPU needed): 200 of the above-median prior draws the ellipsoids were fitted to as the live
    points, their metric, and r^2 = the median, over the replay's would-be-status-2 candidates, of the squared distance to the
    nearest live point (the midpoint of the two middle values, so that no candidate sits on the boundary): about half of them lose
    their status, whatever d is.  Returns (ells, L*, logl_fn, theta, w, metric_inv, r2, replay)."""
    from alabi_amd.nested import mlfriends_metric
    ells, lstar, logl_fn, theta, _ = unif_case(N, d, kernel, E, normal)
    u = np.random.default_rng(1).random((1500, d))              # the draws of test_gpu_nested_unif._ellipsoids
    up = u[logl_fn(u) > lstar]
    up = up[np.argsort(up[:, 0])]
    live = up[np.linspace(0, len(up) - 1, NLIVE).astype(int)]
    _, minv, w = mlfriends_metric(live, ells)
    draws = PhiloxUnifDraws(SEED, CALL, d)
    _, _, marg = mn.mlf_candidates(ells, np.arange(M), draws, w, minv, INF)
    near = np.sort(marg["near2"])
    r2 = 0.5 * (near[len(near) // 2 - 1] + near[len(near) // 2])
    u, status, margins = mn.mlf_candidates(ells, np.arange(M), draws, w, minv, r2)
    logl = np.full(M, -np.inf)
    logl[status == 2] = logl_fn(u[status == 2])
    return ells, lstar, logl_fn, theta, w, minv, r2, (u, status, logl, margins)


def _assert_mlf_replay_is_decisive(ells, lstar, r2, ref):
    u, status, logl, margins = ref
    two = margins["unif_status"] == 2
    assert np.any(two & (status == 2)) and np.any(two & (status == 1))           # both outcomes of the neighbour test
    assert np.sum((status == 2) & (logl > lstar)) >= K
    assert np.min(np.abs(margins["near2"] / r2 - 1.0)) > 1e-9
    _assert_replay_is_decisive(ells, lstar, ref)


def _draw(be, ells, w, minv, r2, m, cand_id0=0, call=CALL, evaluate=1):
    """One alabi_ns_mlf_draw launch: (u, logl, status) on the host."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.gp import _dev
    ns, dev = be._ensure(), _dev()
    tab = [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (ells.centres, ells.axes, ells.inv_axes, ells.cum, w, minv)]
    cu = torch.empty((m, be.ndim), dtype=torch.float64, device=dev)
    cl = torch.empty(m, dtype=torch.float64, device=dev)
    cs = torch.empty(m, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().alabi_ns_mlf_draw(ns, call, cand_id0, m, evaluate, len(ells), *[_lib.ptr(t) for t in tab[:4]],
                                            int(tab[4].shape[0]), _lib.ptr(tab[4]), _lib.ptr(tab[5]), float(r2), _lib.ptr(cu),
                                            _lib.ptr(cl), _lib.ptr(cs), _lib.current_stream()), "alabi_ns_mlf_draw")
    return cu.cpu().numpy(), cl.cpu().numpy(), cs.cpu().numpy()


@pytest.mark.parametrize("N,d,kernel,path,E", CASES)
def test_draw_and_select_match_numpy_replay(N, d, kernel, path, E):
    from alabi_amd.nested import GPUWalkBackend
    ells, lstar, logl_fn, _, w, minv, r2, ref = mlf_case(N, d, kernel, E)
    _assert_mlf_replay_is_decisive(ells, lstar, r2, ref)
    ur, sr, lr, _ = ref
    g, o, y = _gp(N, d, kernel)
    be = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=lambda u: u)
    u, logl, status = _draw(be, ells, w, minv, r2, M)
    if path is not None:
        assert be.last_path() == path
    assert np.array_equal(status, sr)
    assert np.max(np.abs(u - ur)) <= 1e-13
    ev = sr == 2
    assert np.all(np.isneginf(logl[~ev])) and np.max(np.abs(logl[ev] - lr[ev]) / np.abs(lr[ev])) <= 1e-12
    ut, lt, c = _select(be, u, logl, status, lstar, K)
    utr, ltr, cr = select(ur, lr, sr, lstar, K)
    assert np.array_equal(c, cr) and c[0] == K
    assert np.max(np.abs(ut - utr)) <= 1e-13 and np.max(np.abs(lt - ltr) / np.abs(ltr)) <= 1e-12
    # the backend's own loop: the same points and counters
    ub, lb, n_eval, n_cand = be.mlfriends(CALL, ells, w, minv, r2, lstar, K, chunk=M)
    assert np.array_equal(ub, ut) and np.array_equal(lb, lt) and (n_eval, n_cand) == (c[2], c[1])
    assert be.evals_launched == int(ev.sum())
    be.close()


def test_infinite_radius_is_the_ellipsoid_move_and_zero_radius_rejects():
    from alabi_amd.nested import GPUWalkBackend
    from test_gpu_nested_unif import _draw as unif_draw
    N, d = 400, 4
    ells, lstar, _, _, w, minv, r2, ref = mlf_case(N, d, "ExpSquaredKernel", 3)
    g, o, y = _gp(N, d)
    be = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=lambda u: u)
    uu, lu, su = unif_draw(be, ells, M)
    ui, li, si = _draw(be, ells, w, minv, INF, M)
    assert np.array_equal(si, su) and np.array_equal(ui, uu) and np.array_equal(li, lu) and np.any(su == 2)
    u0, l0, s0 = _draw(be, ells, w, minv, 0.0, M)
    assert not np.any(s0 == 2) and np.array_equal(u0, uu) and np.all(np.isneginf(l0))
    assert np.array_equal(s0 == 0, su == 0)
    # the geometry kernel (evaluate = 0) in the same two limits
    gu, gl, gs = unif_draw(be, ells, M, evaluate=0)
    gi = _draw(be, ells, w, minv, INF, M, evaluate=0)
    assert np.array_equal(gi[2], gs) and np.array_equal(gi[0], gu) and np.array_equal(gs, su)
    assert not np.any(_draw(be, ells, w, minv, 0.0, M, evaluate=0)[2] == 2)
    be.close()


def test_result_does_not_depend_on_the_launch_shape():
    from alabi_amd.nested import GPUWalkBackend
    N, d = 400, 4
    ells, lstar, logl_fn, _, w, minv, r2, ref = mlf_case(N, d, "ExpSquaredKernel", 3)
    g, o, y = _gp(N, d)
    be = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=lambda u: u)
    u, logl, status = _draw(be, ells, w, minv, r2, M)
    parts = [_draw(be, ells, w, minv, r2, 64, cand_id0=64 * q) for q in range(4)]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), u)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), logl)
    assert np.array_equal(np.concatenate([p[2] for p in parts]), status)
    one = be.mlfriends(CALL, ells, w, minv, r2, lstar, K, chunk=M)
    four = be.mlfriends(CALL, ells, w, minv, r2, lstar, K, chunk=64)
    default = be.mlfriends(CALL, ells, w, minv, r2, lstar, K)
    for other in (four, default):
        assert np.array_equal(one[0], other[0]) and np.array_equal(one[1], other[1]) and one[2:] == other[2:]
    # more points than the first chunk accepts: the search goes on into the next chunks, in candidate order
    first = int(np.sum((ref[1] == 2) & (ref[2] > lstar)))
    more = first + 20
    ub, lb, n_eval, n_cand = be.mlfriends(CALL, ells, w, minv, r2, lstar, more, chunk=M)
    ur, lr, ne_r, nc_r, _, _ = mn.mlfriends(ells, w, minv, r2, lstar, more, logl_fn, PhiloxUnifDraws(SEED, CALL, d), chunk=M)
    assert len(lb) == more and n_cand > M and (n_eval, n_cand) == (ne_r, nc_r)
    assert np.max(np.abs(ub - ur)) <= 1e-13 and np.max(np.abs(lb - lr) / np.abs(lr)) <= 1e-12
    assert np.array_equal(ub[:K], one[0])
    u0, l0, ne0, nc0 = be.mlfriends(CALL, ells, w, minv, r2, lstar, 0)
    assert u0.shape == (0, d) and l0.shape == (0,) and (ne0, nc0) == (0, 0)
    be.close()


def test_host_likelihood_path_equals_the_fused_one():
    from alabi_amd.nested import GPUWalkBackend
    N, d = 400, 4
    ells, lstar, logl_fn, _, w, minv, r2, ref = mlf_case(N, d, "ExpSquaredKernel", 3)
    g, o, y = _gp(N, d)
    fused = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=lambda u: u)
    split = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=lambda u: u, host_loglike=logl_fn)
    uf, lf, sf = _draw(fused, ells, w, minv, r2, M)
    us, ls, ss = _draw(split, ells, w, minv, r2, M, evaluate=0)
    assert np.array_equal(ss, sf) and np.array_equal(us, uf) and np.all(np.isneginf(ls))
    a = fused.mlfriends(CALL, ells, w, minv, r2, lstar, K, chunk=M)
    b = split.mlfriends(CALL, ells, w, minv, r2, lstar, K, chunk=M)
    assert np.array_equal(a[0], b[0]) and a[2:] == b[2:]
    assert np.max(np.abs(a[1] - b[1]) / np.abs(b[1])) <= 1e-12
    # the host evaluates the candidates that passed the neighbour test, and no others
    assert split.host_calls == int(np.sum(ref[1] == 2)) == split.evals_launched and fused.host_calls == 0
    assert split.host_calls < int(np.sum(ref[3]["unif_status"] == 2))
    fused.close(); split.close()


def test_gaussian_prior_coordinates():
    from alabi_amd.nested import GPUWalkBackend
    N, d, normal = 400, 4, (1, 3)
    ells, lstar, logl_fn, theta, w, minv, r2, ref = mlf_case(N, d, "ExpSquaredKernel", 3, normal)
    _assert_mlf_replay_is_decisive(ells, lstar, r2, ref)
    _, y, _, o = _oracle(N, d)
    g, _, _ = _gp(N, d)
    mean = np.array([0.5 if k in normal else NAN for k in range(d)])
    std = np.array([0.7 if k in normal else NAN for k in range(d)])
    be = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=theta, normal_prior=(mean, std))
    u, logl, n_eval, n_cand = be.mlfriends(CALL, ells, w, minv, r2, lstar, K, chunk=M)
    utr, ltr, cr = select(ref[0], ref[2], ref[1], lstar, K)
    assert (n_eval, n_cand) == (cr[2], cr[1]) and np.max(np.abs(u - utr)) <= 1e-13
    assert np.max(np.abs(logl - o.predict(y, be.transform(u))) / np.abs(logl)) <= 1e-12
    be.close()


def test_bad_arguments_launch_nothing():
    import torch
    from alabi_amd import _lib
    from alabi_amd.gp import _dev
    from alabi_amd.nested import MLF_MAX_POINTS, GPUWalkBackend
    N, d = 400, 4
    ells, _, _, _, w, minv, r2, _ = mlf_case(N, d, "ExpSquaredKernel", 3)
    g, o, y = _gp(N, d)
    be = GPUWalkBackend(g, y, _box(d), seed=SEED, to_theta=lambda u: u)
    ns, dev, lib = be._ensure(), _dev(), _lib.lib()
    tab = [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (ells.centres, ells.axes, ells.inv_axes, ells.cum, w, minv)]
    cu = torch.full((8, d), -7.0, dtype=torch.float64, device=dev)
    cl = torch.full((8,), -7.0, dtype=torch.float64, device=dev)
    cs = torch.full((8,), -7, dtype=torch.int32, device=dev)
    out = (_lib.ptr(cu), _lib.ptr(cl), _lib.ptr(cs), _lib.current_stream())
    tp = [_lib.ptr(t) for t in tab]
    n = len(w)

    def call(E=3, m=8, nn=n, rr=r2, ptrs=tp):
        return lib.alabi_ns_mlf_draw(ns, CALL, 0, m, 1, E, *ptrs[:4], nn, ptrs[4], ptrs[5], rr, *out)
    assert MLF_MAX_POINTS == 16384
    for E in (0, 33, -1):
        assert call(E=E) == _lib.BAD_ARG
    assert call(m=-1) == _lib.BAD_ARG
    for nn in (0, -1, MLF_MAX_POINTS + 1):
        assert call(nn=nn) == _lib.BAD_ARG
    for rr in (NAN, -1e-300, -INF):
        assert call(rr=rr) == _lib.BAD_ARG
    for k in range(6):
        holed = list(tp)
        holed[k] = None
        assert call(ptrs=holed) == _lib.BAD_ARG
    r2o = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    stream = _lib.current_stream()
    for nn, B, wp, op in ((0, 4, tp[4], _lib.ptr(r2o)), (MLF_MAX_POINTS + 1, 4, tp[4], _lib.ptr(r2o)), (n, 0, tp[4], _lib.ptr(r2o)),
                          (n, -1, tp[4], _lib.ptr(r2o)), (n, 4, None, _lib.ptr(r2o)), (n, 4, tp[4], None)):
        assert lib.alabi_ns_mlf_radius(ns, CALL, nn, wp, B, op, stream) == _lib.BAD_ARG
    assert lib.alabi_ns_mlf_radius(None, CALL, n, tp[4], 4, _lib.ptr(r2o), stream) == _lib.BAD_ARG
    torch.cuda.synchronize()
    assert torch.all(cu == -7.0) and torch.all(cl == -7.0) and torch.all(cs == -7) and torch.all(r2o == -7.0)
    # legal: an infinite radius, and no candidates with no outputs
    assert call(rr=INF) == _lib.OK
    assert lib.alabi_ns_mlf_draw(ns, CALL, 0, 0, 1, 3, *tp[:4], n, tp[4], tp[5], r2, None, None, None, stream) == _lib.OK
    torch.cuda.synchronize()
    assert torch.all(cs != -7)
    be.close()


# ---------------------------------------------------------------------------------------------------------- run_ultranest
def test_run_ultranest_evidence_files_and_reproducibility(tmp_path):
    sm = _model(_gauss2, 4.0, tmp_path, 3)
    logz_grid, _ = _grid_logz(sm, 4.0)
    kw = {"sampler_kwargs": {"seed": 11}, "run_kwargs": {"min_num_live_points": 400}}
    sm.run_ultranest(min_ess=0, **kw)
    assert sm.ultranest_run and sm.ultranest_path == "fused" and sm.ultranest_sampler.sample == "mlfriends"
    r = sm.ultranest_results
    assert r.status in ("n_effective", "maxbatch") and r.nbatch <= 1 and r.ncall / r.niter < 25
    assert len(sm.ultranest_sampler.radius2) == len(sm.ultranest_sampler.n_ellipsoids) > 0
    assert sm.ultranest_logz == r.logz[-1] and sm.ultranest_logz_err == r.logzerr[-1]
    assert abs(r.logz[-1] - logz_grid) <= 3 * r.logzerr[-1], (r.logz[-1], logz_grid, r.logzerr[-1])
    s = sm.ultranest_samples
    assert s.shape[1] == 2 and np.array_equal(sm.ultranest_weights, np.full(len(s), 1.0 / len(s)))
    assert sm.ultranest_samples_surrogate is s and sm.ultranest_runtime > 0
    f = np.load(f"{sm.savedir}/ultranest_samples_final_surrogate_iter_0.npz")
    assert sorted(f.files) == ["logz", "logz_err", "samples", "weights"] and np.array_equal(f["samples"], s)
    assert float(f["logz"]) == sm.ultranest_logz and float(f["logz_err"]) == sm.ultranest_logz_err
    assert np.array_equal(f["weights"], sm.ultranest_weights)
    assert not any(name.startswith("ultranest_surrogate") for name in os.listdir(sm.savedir))       # no log directory
    first = (s.copy(), sm.ultranest_logz)
    sm.run_ultranest(min_ess=0, **kw)
    assert np.array_equal(first[0], sm.ultranest_samples) and first[1] == sm.ultranest_logz
    # a static run: no improvement loop
    sm.run_ultranest(min_ess=0, sampler_kwargs={"seed": 11}, run_kwargs={"min_num_live_points": 400, "max_num_improvement_loops": 0})
    r0 = sm.ultranest_results
    assert r0.nbatch == 0 and r0.status == "converged"
    assert abs(r0.logz[-1] - logz_grid) <= 3 * r0.logzerr[-1], (r0.logz[-1], logz_grid, r0.logzerr[-1])
    # min_ess: further runs, stacked, each run's weights 1 / its sample count, log Z of the best run
    sm.run_ultranest(sampler_kwargs={"seed": 5}, run_kwargs={"min_num_live_points": 100, "max_num_improvement_loops": 0},
                     min_ess=1500, samples_file="un.npz")
    assert sm.ultranest_samples.shape[0] >= 1500 and os.path.exists(f"{sm.savedir}/un.npz")
    nruns = sm.ultranest_weights.sum()
    assert abs(nruns - round(nruns)) < 1e-9 and round(nruns) >= 2 and sm.ultranest_logz_err > 0
    assert sm.ultranest_logz >= sm.ultranest_results.logz[-1]


def test_run_ultranest_two_modes(tmp_path):
    sm = _model(_two_modes, 4.0, tmp_path, 4)
    logz_grid, mass_grid = _grid_logz(sm, 4.0)
    sm.run_ultranest(sampler_kwargs={"seed": 3}, run_kwargs={"min_num_live_points": 400}, min_ess=0)
    r = sm.ultranest_results
    assert sm.ultranest_path == "fused" and r.status in ("n_effective", "maxbatch")
    assert abs(r.logz[-1] - logz_grid) <= 3 * r.logzerr[-1], (r.logz[-1], logz_grid, r.logzerr[-1])
    w = r.importance_weights()
    mass = float(np.sum(w[r.samples[:, 0] > 0]) / np.sum(w))
    assert abs(mass_grid - 0.5) < 0.03 and abs(mass - 0.5) <= 0.06, (mass, mass_grid)
    assert max(sm.ultranest_sampler.n_ellipsoids) >= 2


def test_run_ultranest_true_likelihood_with_custom_prior_transform(tmp_path):
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
    sm.run_ultranest(like_fn="true", prior_transform=pt, sampler_kwargs={"seed": 2},
                     run_kwargs={"min_num_live_points": 200, "max_num_improvement_loops": 0}, min_ess=0)
    assert sm.ultranest_path == "host-callback" and sm.like_fn_name == "true" and sm.ultranest_samples_true is sm.ultranest_samples
    r = sm.ultranest_results
    logz_true = 1.5 * math.log(2 * math.pi) + float(np.sum(np.log(sig))) - float(np.sum(np.log(hi - lo)))
    assert abs(r.logz[-1] - logz_true) <= 3 * r.logzerr[-1], (r.logz[-1], logz_true, r.logzerr[-1])
    assert len(calls) >= r.ncall and os.path.exists(f"{sm.savedir}/ultranest_samples_final_true.npz")


def test_run_ultranest_slice_steps_runs_the_slice_move(tmp_path):
    sm = _model(_gauss2, 4.0, tmp_path, 3)
    sm.run_ultranest(sampler_kwargs={"seed": 1}, run_kwargs={"min_num_live_points": 100, "max_num_improvement_loops": 0,
                                                             "frac_remain": 0.5}, min_ess=0, slice_steps=5)
    assert sm.ultranest_sampler.sample == "rslice" and sm.ultranest_sampler.slices == 5 and sm.ultranest_sampler.radius2 == []
    assert sm.ultranest_results.status == "converged" and np.isfinite(sm.ultranest_logz)
