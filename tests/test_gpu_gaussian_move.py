"""GPU parity of the Gaussian Metropolis move (alabi_amd.moves.GaussianMove: ens_mh_kernel and the Gaussian branch of the
launch-per-half-step kernels) against tests/gaussian_move_numpy.py, and the MHMove host loop, on the problems of
tests/moves_shapes_common.py (N = 65 / 130, length scale growing with d).  Tolerances are those of the other moves: proposals
from injected draws bit for bit, log-probabilities to 1e-8 (1 + max|logp|), production chains to 1e-7 with identical acceptance
counts; path 0 and path 4 bit for bit.  tests/test_gaussian_move_host.py asserts on the CPU that every model run used here is no
near tie and holds an accept, an in-box reject and an out-of-box proposal."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import gaussian_move_cases as gc
import gaussian_move_numpy as gm
import moves_shapes_common as ms

pytestmark = pytest.mark.gpu


def _dev(torch, *arrays):
    return [torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in arrays]


def _last_path(s):
    from alabi_amd import _lib
    path = C.c_int(-1)
    _lib.check(_lib.lib().alabi_ens_last_path(s._ens, C.byref(path)), "alabi_ens_last_path")
    return path.value


def _mh_plan(s):
    from alabi_amd import _lib
    plan = (C.c_int * 4)()
    _lib.check(_lib.lib().alabi_ens_mh_plan(s._ens, plan), "alabi_ens_mh_plan")
    return dict(zip(("threads", "chunk", "lds_bytes", "tiled"), (int(v) for v in plan)))


# ------------------------------------------------------------------------------------------------ 1. injected randoms
@pytest.mark.parametrize("d,W,form,mode,kernel", gc.STEP_CASES)
def test_step_with_injected_randoms(d, W, form, mode, kernel):
    """Same draws -> bit-identical accepted proposals, identical accept mask, log-probabilities within 1e-8 (1 + max|logp|),
    over 20 steps."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.moves import GaussianMove
    p0, lp0, cov, steps, st = gc.model_steps(d, W, form, mode, kernel)
    ms.assert_honest(st, (d, W, form, mode, kernel))
    prob = ms.problem(d, kernel)
    s = ms.sampler(prob, W, 1, moves=GaussianMove(cov, mode=mode))
    c_dev = torch.as_tensor(p0, device="cuda").clone()
    lp_dev = s.compute_log_prob(c_dev)
    assert np.max(np.abs(lp_dev.cpu().numpy() - lp0)) < 1e-8 * (1 + np.max(np.abs(lp0)))
    nacc = torch.zeros(W, dtype=torch.int64, device="cuda")
    lib, stream = _lib.lib(), _lib.current_stream()
    coords = p0
    for it, (dr, c_o, l_o, a_o) in enumerate(steps):
        dev = _dev(torch, dr.order, dr.coord, dr.z, dr.u_acc)
        rc = lib.alabi_ens_step_with_randoms_gauss(s._ens, _lib.ptr(c_dev), _lib.ptr(lp_dev), _lib.ptr(dev[0]), dr.n0, 0, float(dr.f),
                                                   _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]), _lib.ptr(nacc), stream)
        _lib.check(rc, "alabi_ens_step_with_randoms_gauss")
        torch.cuda.synchronize()
        c_g, l_g = c_dev.cpu().numpy(), lp_dev.cpu().numpy()
        a_g = np.any(c_g != coords, axis=1)
        scale = 1 + np.max(np.abs(l_o[np.isfinite(l_o)]))
        assert np.array_equal(a_g, a_o), f"accept mask differs at iteration {it}"
        assert np.array_equal(c_g, c_o), f"proposals differ at iteration {it}"
        assert np.max(np.abs(l_g - l_o)) < 1e-8 * scale
        coords = c_o
        lp_dev.copy_(torch.as_tensor(l_o, device="cuda"))
    assert int(nacc.sum()) == sum(int(a.sum()) for _, _, _, a in steps) > 0


def test_a_coordinate_out_of_range_is_a_no_op():
    import torch
    from alabi_amd import _lib
    from alabi_amd.moves import GaussianMove
    d, W = 5, 12
    prob = ms.problem(d, "ExpSquared")
    s = ms.sampler(prob, W, 1, moves=GaussianMove(np.full(d, 0.2), mode="random"))
    p0 = gc.start(prob, W, 3)
    c_dev = torch.as_tensor(p0, device="cuda").clone()
    lp_dev = s.compute_log_prob(c_dev)
    lp0 = lp_dev.cpu().numpy().copy()
    nacc = torch.zeros(W, dtype=torch.int64, device="cuda")
    dr = gc.injected_draws(W, d, "random", 5, 0)
    bad = np.where(np.arange(W) % 2 == 0, d, -2).astype(np.int32)
    dev = _dev(torch, dr.order, bad, dr.z, np.full(W, 1e-300))
    _lib.check(_lib.lib().alabi_ens_step_with_randoms_gauss(s._ens, _lib.ptr(c_dev), _lib.ptr(lp_dev), _lib.ptr(dev[0]), dr.n0, 0, 1.0,
                                                            _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]), _lib.ptr(nacc),
                                                            _lib.current_stream()), "alabi_ens_step_with_randoms_gauss")
    torch.cuda.synchronize()
    assert np.array_equal(c_dev.cpu().numpy(), p0) and np.array_equal(lp_dev.cpu().numpy(), lp0) and int(nacc.sum()) == 0
    assert _lib.lib().alabi_ens_step_with_randoms_gauss(s._ens, _lib.ptr(c_dev), _lib.ptr(lp_dev), _lib.ptr(dev[0]), dr.n0, 1, 1.0,
                                                        _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]), _lib.ptr(nacc),
                                                        _lib.current_stream()) == _lib.BAD_ARG       # the table has one move


def test_exported_draws_are_the_models():
    """alabi_ens_export_gauss_draws returns the model's coordinate bit for bit and its f and normals to a few ulp (libm)."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.moves import GaussianMove
    d, W, E, seed, step = 5, 6, 3, 77, (1 << 33) + 12
    prob = ms.problem(d, "ExpSquared")
    s = ms.sampler(prob, W, seed, n_ensembles=E, moves=GaussianMove(np.full(d, 0.3), mode="random", factor=2.0))
    s._ensure_ens()
    n = W * E
    order = torch.empty(n, dtype=torch.int32, device="cuda"); partner = torch.empty_like(order)
    u_z = torch.empty(n, dtype=torch.float64, device="cuda"); u_acc = torch.empty_like(u_z)
    n0 = C.c_int(0)
    lib, stream = _lib.lib(), _lib.current_stream()
    _lib.check(lib.alabi_ens_export_draws(s._ens, step, 2.0, _lib.ptr(order), C.byref(n0), _lib.ptr(u_z), _lib.ptr(partner),
                                          _lib.ptr(u_acc), None, None, stream), "alabi_ens_export_draws")
    f = torch.empty(E, dtype=torch.float64, device="cuda")
    coord = torch.empty(n, dtype=torch.int32, device="cuda")
    z = torch.empty((n, d), dtype=torch.float64, device="cuda")
    _lib.check(lib.alabi_ens_export_gauss_draws(s._ens, _lib.ptr(f), _lib.ptr(coord), _lib.ptr(z), stream), "alabi_ens_export_gauss_draws")
    torch.cuda.synchronize()
    for e in range(E):
        f_o, c_o, z_o = gm.draw_gauss_randoms(seed, step, np.arange(W) + e * W, e * W, np.log(2.0), 1, d)
        assert abs(f[e].item() - f_o) <= 4 * np.spacing(f_o) and 0.5 <= f_o <= 2.0
        assert np.array_equal(coord[e * W:(e + 1) * W].cpu().numpy(), c_o)
        assert np.max(np.abs(z[e * W:(e + 1) * W].cpu().numpy() - z_o)) < 1e-13


# ------------------------------------------------------------------- 2 and 3. production chains on path 4 and on path 0
ENS = "ens3"                                  # the n_ensembles = 3 run: one more case of the same harness
ALL_CHAINS = list(gc.CHAIN_CASES) + [ENS]


@lru_cache(maxsize=None)
def _model(name):
    """The model's side of a chain case.  The n_ensembles case is E single-ensemble model runs with id0 = e W, laid side by side
    as the device lays its ensembles (rows [e W, (e + 1) W) belong to ensemble e)."""
    from types import SimpleNamespace
    if name != ENS:
        d, kernel, W, moves, N = gc.CHAIN_CASES[name]
        run = gc.model_chain(name)
        return SimpleNamespace(W=W, E=1, prob=gc.case_problem(name), p0=run.p0, seed=run.seed, spec=run.spec, chain=run.chain,
                               logp=run.logp, nacc=run.nacc, cont=run.cont, nacc_cont=run.nacc_cont, stats=[run.stats],
                               counts=[run.counts])
    d, kernel, W, E, moves = gc.ENS_CASE
    p0, seed, runs = gc.model_ensembles()
    cat = lambda key, axis: np.concatenate([getattr(r, key) for r in runs], axis=axis)   # noqa: E731
    return SimpleNamespace(W=W, E=E, prob=ms.problem(d, kernel), p0=p0, seed=seed, spec=runs[0].spec, chain=cat("chain", 1),
                           logp=cat("logp", 1), nacc=cat("nacc", 0), cont=cat("cont", 1), nacc_cont=cat("nacc_cont", 0),
                           stats=[r.stats for r in runs], counts=[r.counts for r in runs])


@lru_cache(maxsize=None)
def _device_chain(name, path):
    """(chain, logp, counts after the run, continuation, thinned chain, last_path, plan) of a chain case on path 4 or path 0."""
    import torch  # noqa: F401
    from alabi_amd import _lib
    run = _model(name)

    def make():
        s = ms.sampler(run.prob, run.W, run.seed, n_ensembles=run.E, moves=gc.moves_objects(run.spec))
        if path == 0:
            s._ensure_ens()
            _lib.check(_lib.lib().alabi_ens_set_stream(s._ens, 0), "alabi_ens_set_stream")
        return s
    s = make()
    s.run_mcmc(run.p0, gc.CHAIN_STEPS, skip_initial_state_check=True)
    out = dict(chain=s.get_chain_device().clone(), logp=s.get_chain_device(log_prob=True).clone(), nacc=s._naccept.clone(),
               path=_last_path(s), plan=_mh_plan(s))
    s.run_mcmc(None, gc.CONT_STEPS)
    out["cont"] = s.get_chain_device()[gc.CHAIN_STEPS:].clone()
    out["nacc_cont"] = s._naccept.clone()
    t = make()
    t.run_mcmc(run.p0, gc.CHAIN_STEPS, thin_by=gc.THIN, skip_initial_state_check=True)
    out["thin"] = t.get_chain_device().clone()
    out["thin_logp"] = t.get_chain_device(log_prob=True).clone()
    return out


@pytest.mark.parametrize("name", ALL_CHAINS)
def test_production_chain_on_the_metropolis_kernel(name):
    """60 steps, a 10-step continuation (step0) and a run with thin_by = 3 on ens_mh_kernel against the model: chains within
    1e-7, identical acceptance counts, path 4; the tiled cases stream a second tile of the training set.  With n_ensembles = 3
    the factor and the move choice are per ensemble, drawn at its walker 0: three single-ensemble model runs with id0 = e W."""
    run = _model(name)
    for st in run.stats:
        ms.assert_honest(st, name)
    g = _device_chain(name, 4)
    assert g["path"] == 4
    assert g["plan"]["tiled"] == (1 if name.startswith("tiled") else 0), g["plan"]
    scale = 1 + np.max(np.abs(run.logp))
    assert np.max(np.abs(g["chain"].cpu().numpy() - run.chain)) < 1e-7
    assert np.max(np.abs(g["logp"].cpu().numpy() - run.logp)) < 1e-7 * scale
    assert np.array_equal(g["nacc"].cpu().numpy(), run.nacc)
    assert np.max(np.abs(g["cont"].cpu().numpy() - run.cont)) < 1e-7
    assert np.array_equal(g["nacc_cont"].cpu().numpy(), run.nacc + run.nacc_cont)
    assert np.max(np.abs(g["thin"].cpu().numpy() - run.chain[gc.THIN - 1::gc.THIN])) < 1e-7
    assert np.max(np.abs(g["thin_logp"].cpu().numpy() - run.logp[gc.THIN - 1::gc.THIN])) < 1e-7 * scale
    if len(run.spec) > 1:
        for counts in run.counts:
            assert set(counts) == set(range(len(run.spec))), counts
    if name == ENS:
        assert len({tuple(sorted(c.items())) for c in run.counts}) > 1       # the ensembles do not choose the same moves


@pytest.mark.parametrize("name", ALL_CHAINS)
def test_path_0_equals_path_4(name):
    """The same runs with one launch per half step (alabi_ens_set_stream(ens, 0)): the same bits."""
    import torch
    a, b = _device_chain(name, 4), _device_chain(name, 0)
    assert a["path"] == 4 and b["path"] == 0
    for key in ("chain", "logp", "nacc", "cont", "nacc_cont", "thin", "thin_logp"):
        assert torch.equal(a[key], b[key]), key


def test_a_call_split_in_two_is_the_same_bits(monkeypatch):
    """One 60-step call, 25 + 35 steps, and launches of at most 7 steps (ALABI_ENS_MH_CHUNK): identical chains."""
    import torch
    name = "two"
    d, kernel, W, moves, N = gc.CHAIN_CASES[name]
    run = gc.model_chain(name)
    prob = gc.case_problem(name)
    ref = _device_chain(name, 4)
    s = ms.sampler(prob, W, run.seed, moves=gc.moves_objects(run.spec))
    s.run_mcmc(run.p0, 25, skip_initial_state_check=True)
    s.run_mcmc(None, 35)
    assert torch.equal(s.get_chain_device(), ref["chain"]) and torch.equal(s._naccept, ref["nacc"])
    monkeypatch.setenv("ALABI_ENS_MH_CHUNK", "7")
    t = ms.sampler(prob, W, run.seed, moves=gc.moves_objects(run.spec))
    t.run_mcmc(run.p0, gc.CHAIN_STEPS, thin_by=gc.THIN, skip_initial_state_check=True)
    assert _mh_plan(t)["chunk"] == 7
    assert torch.equal(t.get_chain_device(), ref["thin"])


# ------------------------------------------------------------------------------------------------- 4. fused extras
@pytest.mark.parametrize("d,which", gc.EXTRAS)
def test_fused_extras_on_the_metropolis_kernel(d, which):
    run = gc.model_extras(d, which)
    ms.assert_honest(run.stats, (d, which))
    kw = {}
    if which == "prior":
        kw = dict(normal_prior=ms.normal_prior(d), logp_affine=ms.AFFINE)
    elif which in ("nlog", "log"):
        kw = dict(logp_map=which)
    s = ms.sampler(run.prob, 12, run.seed, moves=gc.moves_objects(run.spec), **kw)
    s.run_mcmc(run.p0, gc.CHAIN_STEPS, skip_initial_state_check=True)
    assert _last_path(s) == 4
    assert np.max(np.abs(s.get_chain() - run.chain)) < 1e-7
    assert np.array_equal(s._naccept.cpu().numpy(), run.nacc)
    lp = s.get_log_prob()
    assert np.max(np.abs(lp - run.logp)) < 1e-7 * (1 + np.max(np.abs(run.logp)))


# ------------------------------------------------------------------------------ 5. mixture with red-blue moves, path 0
@pytest.mark.parametrize("d", gc.MIX_DIMS)
def test_mixture_with_red_blue_moves(d):
    run = gc.model_mixture(d)
    ms.assert_honest(run.stats, ("mix", d))
    assert set(run.counts) == {0, 1, 2}, run.counts
    s = ms.sampler(run.prob, 12, run.seed, moves=gc.moves_objects(run.spec))
    s.run_mcmc(run.p0, gc.CHAIN_STEPS, skip_initial_state_check=True)
    assert _last_path(s) == 0
    assert np.max(np.abs(s.get_chain() - run.chain)) < 1e-7
    assert np.array_equal(s._naccept.cpu().numpy(), run.nacc)


# ----------------------------------------------------------------------------------------------- 6. host callables
def test_host_prior_equals_the_fused_prior():
    """A Gaussian set with a Python prior_fn through propose / accept against the fused run of the same normal prior."""
    from scipy.stats import norm
    d, W = 4, 12
    prob = ms.problem(d, "ExpSquared")
    pm, ps = ms.normal_prior(d)
    moves = gc.moves_objects(gc.spec_of(d, ("matrix", "vector", None, 1.0)))
    p0 = gc.start(prob, W, 31)

    def prior(q):
        inside = np.all((q > prob.bounds[:, 0]) & (q < prob.bounds[:, 1]), axis=1)
        v = np.zeros(len(q))
        for k in ms.PRIOR_DIMS[d]:
            v = v + norm.logpdf(q[:, k], pm[k], ps[k])
        return np.where(inside, v, -np.inf)
    fused = ms.sampler(prob, W, 9, moves=moves, normal_prior=(pm, ps))
    fused.run_mcmc(p0, 40, skip_initial_state_check=True)
    host = ms.sampler(prob, W, 9, moves=moves, prior_fn=prior)
    host.run_mcmc(p0, 40, skip_initial_state_check=True)
    assert host.last_path == "host-callback" and _last_path(fused) == 4
    assert np.max(np.abs(host.get_chain() - fused.get_chain())) < 1e-7
    assert np.array_equal(host._naccept.cpu().numpy(), fused._naccept.cpu().numpy())
    assert 0 < int(fused._naccept.sum()) < 40 * W


# ------------------------------------------------------------------------------------------------------ 7. MHMove
def _gauss_proposal(sig):
    def fn(coords, rng):
        return coords + sig * rng.standard_normal(coords.shape), np.zeros(len(coords))
    return fn


@pytest.mark.parametrize("foreign", [False, True])
def test_mhmove_on_the_device_log_probability(foreign):
    import torch
    from alabi_amd.moves import MHMove
    d, W, nsteps = 5, 8, 30
    prob = ms.problem(d, "ExpSquared")
    if foreign:
        class Anything:                                        # recognised by its callable get_proposal alone
            get_proposal = staticmethod(_gauss_proposal(0.4))
        move = Anything()
    else:
        move = MHMove(_gauss_proposal(0.4), ndim=d)
    s = ms.sampler(prob, W, 5, moves=move)
    s.run_mcmc(gc.start(prob, W, 5), nsteps, skip_initial_state_check=True)
    assert s.last_path == "host-mh"
    chain, lp = s.get_chain(), s.get_log_prob()
    assert chain.shape == (nsteps, W, d)
    worst = 0.0
    for t in range(nsteps):
        ref = s.compute_log_prob(torch.as_tensor(chain[t], device="cuda")).cpu().numpy()
        worst = max(worst, float(np.max(np.abs(ref - lp[t]))))
    assert worst < 1e-8 * (1 + np.max(np.abs(lp)))
    af = s.acceptance_fraction
    assert 0.0 < af.mean() < 1.0
    moved = np.any(chain[1:] != chain[:-1], axis=2).sum(axis=0) + np.any(chain[0] != gc.start(prob, W, 5), axis=1)
    assert np.array_equal(moved, s._naccept.cpu().numpy())


# ---------------------------------------------------------------------------------------------------- 8. run_emcee
def test_run_emcee_with_a_gaussian_move(tmp_path):
    """SurrogateModel.run_emcee(sampler_kwargs={"moves": GaussianMove(cov)}) on the 2-D problem of
    tests/test_gpu_surrogate_model.py (Rosenbrock, 50 training points)."""
    from alabi_amd import SurrogateModel
    from alabi_amd.benchmarks import rosenbrock
    from alabi_amd.moves import GaussianMove
    sm = SurrogateModel(lnlike_fn=rosenbrock["fn"], bounds=rosenbrock["bounds"], savedir=str(tmp_path), verbose=False, random_state=0)
    sm.init_samples(ntrain=50, ntest=20, sampler="uniform")
    sm.init_gp(kernel="ExpSquaredKernel", fit_amp=True, fit_mean=True, white_noise=-12, hyperopt_method="ml", gp_nopt=1)
    b = np.asarray(rosenbrock["bounds"], dtype=float)
    cov = (0.1 * (b[:, 1] - b[:, 0])) ** 2
    sm.run_emcee(nwalkers=16, nsteps=400, min_ess=0, sampler_kwargs={"moves": GaussianMove(cov)})
    assert sm.emcee_samples.ndim == 2 and sm.emcee_samples.shape[1] == 2 and sm.emcee_samples.shape[0] > 0
    assert sm.emcee_samples_full.shape == (400, 16, 2)
    assert 0.0 < sm.acc_frac < 1.0
    assert np.all(sm.emcee_samples > b[:, 0]) and np.all(sm.emcee_samples < b[:, 1])
    assert sm.emcee_sampler.last_path == "metropolis" and sm.emcee_sampler.last_stream_kernel == "ens_mh_kernel"


# --------------------------------------------------------------------------------------------------- the library
def test_library_refuses_what_the_header_says():
    import torch
    from alabi_amd import _lib
    d = 5
    prob = ms.problem(d, "ExpSquared")
    lib = _lib.lib()

    def set_moves(s, p0, p1):
        return lib.alabi_ens_set_moves(s._ens, 1, (C.c_int * 1)(5), _lib.host_doubles([1.0]), _lib.host_doubles([p0]), _lib.host_doubles([p1]))
    s = ms.sampler(prob, 6, 1); s._ensure_ens()
    scale = lambda k, M, diag: lib.alabi_ens_set_move_scale(s._ens, k, _lib.host_doubles(M.ravel()), diag)   # noqa: E731
    eye = np.eye(d)
    full = np.linalg.cholesky(gc.cov_of("matrix", d, "vector"))
    upper = eye.copy(); upper[0, 1] = 0.1
    neg = eye.copy(); neg[2, 2] = -1.0
    assert set_moves(s, 0.0, 0.0) == _lib.BAD_ARG             # a Gaussian move whose slot has been given no scale factor
    assert scale(0, upper, 0) == _lib.BAD_ARG and scale(0, neg, 1) == _lib.BAD_ARG
    assert scale(0, full, 1) == _lib.BAD_ARG                  # not diagonal
    assert scale(8, eye, 1) == _lib.BAD_ARG and scale(-1, eye, 1) == _lib.BAD_ARG   # no such slot
    assert set_moves(s, 0.0, 0.0) == _lib.BAD_ARG             # none of those left a factor
    assert scale(0, full, 0) == _lib.OK
    for p0, p1 in ((-0.1, 0.0), (np.nan, 0.0), (0.0, 3.0), (0.0, 0.5), (np.inf, 1.0)):
        assert set_moves(s, p0, p1) == _lib.BAD_ARG, (p0, p1)
    assert set_moves(s, 0.0, 1.0) == _lib.BAD_ARG             # mode 1 wants a diagonal factor
    assert set_moves(s, 0.0, 0.0) == _lib.OK
    c = torch.as_tensor(gc.start(prob, 6, 2), device="cuda")
    lp = s.compute_log_prob(c)
    run = lambda: lib.alabi_ens_run(s._ens, _lib.ptr(c), _lib.ptr(lp), 0, 4, 1, 2.0, None, None, None, _lib.current_stream())   # noqa: E731
    assert run() == _lib.OK
    assert set_moves(s, 0.0, 0.0) == _lib.BAD_ARG             # the factor belonged to the table it was handed over for
    assert run() == _lib.OK                                   # a refused table leaves the one before it in place
    assert scale(0, eye, 1) == _lib.OK and set_moves(s, np.log(2.0), 1.0) == _lib.OK and run() == _lib.OK
    assert scale(0, full, 0) == _lib.BAD_ARG                  # the move in slot 0 moves one coordinate
    assert scale(0, 2.0 * eye, 1) == _lib.OK and run() == _lib.OK   # a new factor for the move in place
    torch.cuda.synchronize()
    # alabi_ens_set_stream belongs to the handle, not to the table that is set when it is called
    t = ms.sampler(prob, 6, 1); t._ensure_ens()                # a red-blue handle
    path = C.c_int(-1)
    run_t = lambda: lib.alabi_ens_run(t._ens, _lib.ptr(c), _lib.ptr(lp), 0, 4, 1, 2.0, None, None, None, _lib.current_stream())   # noqa: E731
    assert lib.alabi_ens_set_stream(t._ens, 0) == _lib.OK
    assert lib.alabi_ens_set_move_scale(t._ens, 0, _lib.host_doubles(eye.ravel()), 1) == _lib.OK
    assert lib.alabi_ens_set_moves(t._ens, 1, (C.c_int * 1)(5), _lib.host_doubles([1.0]), _lib.host_doubles([0.0]), _lib.host_doubles([0.0])) == _lib.OK
    assert run_t() == _lib.OK and lib.alabi_ens_last_path(t._ens, C.byref(path)) == _lib.OK and path.value == 0
    assert lib.alabi_ens_set_stream(t._ens, 1) == _lib.OK
    assert run_t() == _lib.OK and lib.alabi_ens_last_path(t._ens, C.byref(path)) == _lib.OK and path.value == 4
    torch.cuda.synchronize()
    # one walker: a Gaussian table runs, a red-blue one is refused
    one = ms.sampler(prob, 1, 1, moves=__import__("alabi_amd").moves.GaussianMove(0.1)); one._ensure_ens()
    assert lib.alabi_ens_set_moves(one._ens, 1, (C.c_int * 1)(0), _lib.host_doubles([1.0]), _lib.host_doubles([2.0]),
                                   _lib.host_doubles([0.0])) == _lib.BAD_ARG
