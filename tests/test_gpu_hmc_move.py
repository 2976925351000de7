"""GPU parity of the HMC move (alabi_amd.moves.HMCMove: ens_hmc_kernel, alabi_ens_log_prob_grad) against tests/hmc_numpy.py on
the problems of tests/moves_shapes_common.py (N = 65 / 130 on [-3, 3]^d, one case whose training set needs a second tile).
Tolerances: log-probabilities 1e-8 (1 + max|lp|), gradients 1e-9 max|grad| (the project's predict_grad tolerance), positions of
single steps and chains 1e-7, their log-probabilities 1e-7 (1 + max|lp|), accept masks and acceptance counts identical; call
splitting bit for bit.  tests/test_hmc_move_host.py asserts on the CPU that every model run used here is no near tie and holds an
accept, an in-box reject and an out-of-box end point."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import hmc_cases as hc
import hmc_numpy as hm
import moves_shapes_common as ms

pytestmark = pytest.mark.gpu


def _dev(torch, *arrays):
    return [torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in arrays]


def _last_path(s):
    from alabi_amd import _lib
    path = C.c_int(-1)
    _lib.check(_lib.lib().alabi_ens_last_path(s._ens, C.byref(path)), "alabi_ens_last_path")
    return path.value


def _hmc_plan(s):
    from alabi_amd import _lib
    plan = (C.c_int * 4)()
    _lib.check(_lib.lib().alabi_ens_hmc_plan(s._ens, plan), "alabi_ens_hmc_plan")
    return dict(zip(("threads", "chunk", "lds_bytes", "tiled"), (int(v) for v in plan)))


# -------------------------------------------------------------------------------------------- 1. value and gradient
@pytest.mark.parametrize("name", list(hc.GRID) + list(hc.LPG_EXTRAS), ids=str)
def test_log_prob_grad_against_the_model(name):
    """alabi_ens_log_prob_grad at 32 points (one on a training point, two outside the box, one on its wall): value within
    1e-8 (1 + max|lp|), gradient within 1e-9 max|grad|, -inf and a zero gradient outside."""
    import torch
    prob, ex = hc.lpg_problem(name)
    tgt = hc.target_of(prob, ex)
    pts = hc.lpg_points(prob)
    lp_o, g_o = tgt.gated_value_grad(pts)
    s = ms.sampler(prob, 4, 1, **hc.sampler_kw(ex))
    lp, g = s.log_prob_grad(torch.as_tensor(pts, device="cuda"))
    torch.cuda.synchronize()
    lp, g = lp.cpu().numpy(), g.cpu().numpy()
    out = ~tgt.inside(pts)
    assert out.sum() == 3 and not out[0]
    assert np.all(np.isneginf(lp[out])) and np.all(g[out] == 0.0)
    fin = ~out
    err_lp, err_g = np.max(np.abs(lp[fin] - lp_o[fin])), np.max(np.abs(g[fin] - g_o[fin]))
    print(f"log_prob_grad {name}: value error {err_lp:.3e} (scale {1 + np.max(np.abs(lp_o[fin])):.3g}), gradient error "
          f"{err_g:.3e} (max|grad| {np.max(np.abs(g_o[fin])):.3g})")
    assert err_lp < 1e-8 * (1 + np.max(np.abs(lp_o[fin])))
    assert err_g < 1e-9 * np.max(np.abs(g_o[fin]))
    # the value agrees with the kernels that evaluate the log-probability alone
    sel = [0, 4, 5, 6]
    lp4 = s.compute_log_prob(torch.as_tensor(pts[sel], device="cuda")).cpu().numpy()
    assert np.max(np.abs(lp4 - lp[sel])) < 1e-8 * (1 + np.max(np.abs(lp[sel])))


# ------------------------------------------------------------------------------------------------ 2. injected draws
@pytest.mark.parametrize("d,kernel,L", hc.STEP_CASES)
def test_step_with_injected_randoms(d, kernel, L):
    """Same draws -> identical accept mask, positions within 1e-7 and log-probabilities within 1e-7 (1 + max|lp|), over 20
    steps from the model's state."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.moves import HMCMove
    p0, lp0, cov, ex, steps, st = hc.model_steps(d, kernel, L)
    ms.assert_honest(st, (d, kernel, L))
    prob = ms.problem(d, kernel)
    W = hc.W_STEP
    s = ms.sampler(prob, W, 1, moves=HMCMove(cov, step_size=hc.step_size(d, L), n_leapfrog=L), **hc.sampler_kw(ex))
    c_dev = torch.as_tensor(p0, device="cuda").clone()
    lp_dev = s.compute_log_prob(c_dev)
    assert np.max(np.abs(lp_dev.cpu().numpy() - lp0)) < 1e-8 * (1 + np.max(np.abs(lp0)))
    nacc = torch.zeros(W, dtype=torch.int64, device="cuda")
    lib, stream = _lib.lib(), _lib.current_stream()
    coords, worst_c, worst_lp = p0, 0.0, 0.0
    for it, (dr, c_o, l_o, a_o) in enumerate(steps):
        z, u = _dev(torch, dr.z, dr.u_acc)
        _lib.check(lib.alabi_ens_step_with_randoms_hmc(s._ens, _lib.ptr(c_dev), _lib.ptr(lp_dev), 0, float(dr.e), _lib.ptr(z),
                                                       _lib.ptr(u), _lib.ptr(nacc), stream), "alabi_ens_step_with_randoms_hmc")
        torch.cuda.synchronize()
        c_g, l_g = c_dev.cpu().numpy(), lp_dev.cpu().numpy()
        a_g = np.any(c_g != coords, axis=1)
        scale = 1 + np.max(np.abs(l_o[np.isfinite(l_o)]))
        assert np.array_equal(a_g, a_o), f"accept mask differs at iteration {it}"
        worst_c, worst_lp = max(worst_c, np.max(np.abs(c_g - c_o))), max(worst_lp, np.max(np.abs(l_g - l_o)) / scale)
        assert np.max(np.abs(c_g - c_o)) < 1e-7, f"positions differ at iteration {it}"
        assert np.max(np.abs(l_g - l_o)) < 1e-7 * scale
        coords = c_o
        c_dev.copy_(torch.as_tensor(c_o, device="cuda"))
        lp_dev.copy_(torch.as_tensor(l_o, device="cuda"))
    print(f"step {d} {kernel} L={L}: max position error {worst_c:.3e}, max relative lp error {worst_lp:.3e}")
    assert int(nacc.sum()) == sum(int(a.sum()) for _, _, _, a in steps) > 0
    assert _hmc_plan(s)["threads"] in (256, 512) and _hmc_plan(s)["chunk"] == 1


# ------------------------------------------------------------------------------------------------- 3. exported draws
def test_exported_draws_are_the_models():
    """alabi_ens_export_hmc_draws returns the model's move, its e to 4 ulp and its normals to 1e-13; with n_ensembles = 3 and
    jitter e differs per ensemble."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.moves import HMCMove
    d, W, E, seed, step = 5, 6, 3, 77, (1 << 33) + 12
    prob = ms.problem(d, "ExpSquared")
    spec = [(np.full(d, 0.3), 0.4, 2, 1.5, 0.5), (0.7, None, 1, 2.0, 0.5)]
    s = ms.sampler(prob, W, seed, n_ensembles=E, moves=hc.moves_objects(spec))
    s._ensure_ens()
    n = W * E
    move = torch.empty(E, dtype=torch.int32, device="cuda")
    e = torch.empty(E, dtype=torch.float64, device="cuda")
    z = torch.empty((n, d), dtype=torch.float64, device="cuda")
    u = torch.empty(n, dtype=torch.float64, device="cuda")
    _, cum, p0, p1, _ = hm.move_table(spec, d)
    es, moves_seen = [], set()
    for st in (step, step + 1, step + 2, step + 3):
        _lib.check(_lib.lib().alabi_ens_export_hmc_draws(s._ens, st, _lib.ptr(move), _lib.ptr(e), _lib.ptr(z), _lib.ptr(u),
                                                         _lib.current_stream()), "alabi_ens_export_hmc_draws")
        torch.cuda.synchronize()
        for k in range(E):
            mi_o, e_o, z_o, u_o = hm.draw_hmc_randoms(seed, st, np.arange(W) + k * W, k * W, cum, p0, p1, d)
            assert int(move[k]) == mi_o
            assert abs(e[k].item() - e_o) <= 4 * np.spacing(e_o)
            assert np.max(np.abs(z[k * W:(k + 1) * W].cpu().numpy() - z_o)) < 1e-13
            assert np.array_equal(u[k * W:(k + 1) * W].cpu().numpy(), u_o)
            moves_seen.add(mi_o)
        es.append(e.cpu().numpy().copy())
    assert len(set(es[0])) == E                 # one jitter draw per step and ENSEMBLE
    assert moves_seen == {0, 1}
    assert p0[1] == d ** -0.25                  # step_size=None resolved


# ------------------------------------------------------------------------------------------------ 4. production chains
@lru_cache(maxsize=None)
def _device_chain(name):
    import torch  # noqa: F401
    run = hc.model_chain(name)

    def make():
        return ms.sampler(run.prob, run.W, run.seed, n_ensembles=run.E, moves=hc.moves_objects(run.spec), **hc.sampler_kw(run.ex))
    s = make()
    s.run_mcmc(run.p0, hc.CHAIN_STEPS, skip_initial_state_check=True)
    out = dict(chain=s.get_chain_device().clone(), logp=s.get_chain_device(log_prob=True).clone(), nacc=s._naccept.clone(),
               path=_last_path(s), plan=_hmc_plan(s), last_path=s.last_path, kernel=s.last_stream_kernel)
    s.run_mcmc(None, hc.CONT_STEPS)
    out["cont"] = s.get_chain_device()[hc.CHAIN_STEPS:].clone()
    out["nacc_cont"] = s._naccept.clone()
    t = make()
    t.run_mcmc(run.p0, hc.CHAIN_STEPS, thin_by=hc.THIN, skip_initial_state_check=True)
    out["thin"] = t.get_chain_device().clone()
    out["thin_logp"] = t.get_chain_device(log_prob=True).clone()
    return out


@pytest.mark.parametrize("name", list(hc.CHAIN_CASES))
def test_production_chain(name):
    """60 steps, a 10-step continuation (step0) and a run with thin_by = 3 on ens_hmc_kernel against the model: chains within
    1e-7, identical acceptance counts, last_path "hmc".  With n_ensembles = 3 the jitter and the move choice are per ensemble,
    drawn at its walker 0: three single-ensemble model runs with id0 = e W."""
    run = hc.model_chain(name)
    for st in run.stats:
        ms.assert_honest(st, name)
    g = _device_chain(name)
    assert g["path"] == 5 and g["last_path"] == "hmc" and g["kernel"] == "ens_hmc_kernel"
    assert g["plan"]["tiled"] == (1 if name == "tiled" else 0), g["plan"]
    scale = 1 + np.max(np.abs(run.logp))
    print(f"chain {name}: max position error {np.max(np.abs(g['chain'].cpu().numpy() - run.chain)):.3e}")
    assert np.max(np.abs(g["chain"].cpu().numpy() - run.chain)) < 1e-7
    assert np.max(np.abs(g["logp"].cpu().numpy() - run.logp)) < 1e-7 * scale
    assert np.array_equal(g["nacc"].cpu().numpy(), run.nacc)
    assert np.max(np.abs(g["cont"].cpu().numpy() - run.cont)) < 1e-7
    assert np.array_equal(g["nacc_cont"].cpu().numpy(), run.nacc + run.nacc_cont)
    assert np.max(np.abs(g["thin"].cpu().numpy() - run.chain[hc.THIN - 1::hc.THIN])) < 1e-7
    assert np.max(np.abs(g["thin_logp"].cpu().numpy() - run.logp[hc.THIN - 1::hc.THIN])) < 1e-7 * scale
    if len(run.spec) > 1:
        for counts in run.counts:
            assert set(counts) == set(range(len(run.spec))), counts


# --------------------------------------------------------------------------------------------------- 5. call splitting
def test_call_splitting_changes_no_bit(monkeypatch):
    """One 60-step call, 25 + 35 steps and ALABI_ENS_HMC_CHUNK=7 give identical bits; the plan reports chunk 7."""
    import torch
    name = "two"
    run = hc.model_chain(name)

    def make():
        return ms.sampler(run.prob, run.W, run.seed, moves=hc.moves_objects(run.spec), **hc.sampler_kw(run.ex))
    one = _device_chain(name)
    s = make()
    s.run_mcmc(run.p0, 25, skip_initial_state_check=True)
    s.run_mcmc(None, 35)
    assert torch.equal(s.get_chain_device(), one["chain"]) and torch.equal(s.get_chain_device(log_prob=True), one["logp"])
    assert torch.equal(s._naccept, one["nacc"])
    assert one["plan"]["chunk"] >= hc.CHAIN_STEPS
    monkeypatch.setenv("ALABI_ENS_HMC_CHUNK", "7")
    t = make()
    t.run_mcmc(run.p0, hc.CHAIN_STEPS, skip_initial_state_check=True)
    assert _hmc_plan(t)["chunk"] == 7
    assert torch.equal(t.get_chain_device(), one["chain"]) and torch.equal(t.get_chain_device(log_prob=True), one["logp"])
    assert torch.equal(t._naccept, one["nacc"])


# ------------------------------------------------------------------------------------------------------- 6. refusals
def test_library_refusals():
    """alabi_ens_set_moves refuses a kind-6 row without a factor, with a step size that is not positive and finite, with
    n_leapfrog outside 1 ... 64 and mixed with another kind; alabi_ens_set_stream(ens, 0) does not move an HMC table;
    alabi_ens_draw refuses one."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.moves import HMCMove
    d, W = 3, 6
    prob = ms.problem(d, "ExpSquared")
    s = ms.sampler(prob, W, 5, moves=HMCMove(0.5, step_size=0.4, n_leapfrog=2))
    s._ensure_ens()
    lib = _lib.lib()
    eye = _lib.host_doubles(np.eye(d).ravel())

    def set_moves(kinds, p0, p1, stage=()):
        for k in stage:
            _lib.check(lib.alabi_ens_set_move_scale(s._ens, k, eye, 1), "alabi_ens_set_move_scale")
        n = len(kinds)
        cum = np.cumsum(np.full(n, 1.0 / n))
        return lib.alabi_ens_set_moves(s._ens, n, (C.c_int * n)(*kinds), _lib.host_doubles(cum), _lib.host_doubles(p0), _lib.host_doubles(p1))
    assert set_moves([6], [0.4], [2.0]) == _lib.BAD_ARG                          # no factor since the last table
    assert set_moves([6], [0.0], [2.0], stage=(0,)) == _lib.BAD_ARG              # step size
    assert set_moves([6], [-0.1], [2.0], stage=(0,)) == _lib.BAD_ARG
    assert set_moves([6], [np.inf], [2.0], stage=(0,)) == _lib.BAD_ARG
    assert set_moves([6], [np.nan], [2.0], stage=(0,)) == _lib.BAD_ARG
    assert set_moves([6], [0.4], [0.5], stage=(0,)) == _lib.BAD_ARG              # n_leapfrog 0
    assert set_moves([6], [0.4], [65.0], stage=(0,)) == _lib.BAD_ARG             # n_leapfrog 65
    assert set_moves([6, 0], [0.4, 2.0], [2.0, 0.0], stage=(0,)) == _lib.BAD_ARG   # mixed with a stretch move
    assert set_moves([6, 6], [0.4, 0.2], [64.0, 1.0], stage=(0,)) == _lib.BAD_ARG   # the second slot has no factor
    assert set_moves([6, 5], [0.4, 0.0], [2.0, 0.0], stage=(0, 1)) == _lib.BAD_ARG  # mixed with a Gaussian move
    assert set_moves([6, 6], [0.4, 0.2], [64.0, 1.0], stage=(0, 1)) == _lib.OK
    # the table the sampler set is replaced by the two-move one; it still runs on ens_hmc_kernel after set_stream(0)
    _lib.check(lib.alabi_ens_set_stream(s._ens, 0), "alabi_ens_set_stream")
    assert lib.alabi_ens_draw(s._ens, 0, 1, 2.0, _lib.current_stream()) == _lib.BAD_ARG
    s.run_mcmc(hc.start(prob, W, 3), 5, skip_initial_state_check=True)
    assert s.last_path == "hmc"
    z = torch.zeros((W, d), dtype=torch.float64, device="cuda"); u = torch.full((W,), 0.5, dtype=torch.float64, device="cuda")
    args = (_lib.ptr(z), _lib.ptr(u), None, _lib.current_stream())
    assert lib.alabi_ens_step_with_randoms_hmc(s._ens, _lib.ptr(s._coords), _lib.ptr(s._logp), 2, 0.3, *args) == _lib.BAD_ARG
    assert lib.alabi_ens_step_with_randoms_hmc(s._ens, _lib.ptr(s._coords), _lib.ptr(s._logp), 0, 0.0, *args) == _lib.BAD_ARG


def test_a_table_beyond_the_lds_is_refused_by_the_run():
    """Five full factors at d = 64 need 5 x 64 x 65 x 8 bytes = 162 KB of LDS: alabi_ens_set_moves takes the table, alabi_ens_run
    is ALABI_BAD_ARGUMENT (there is no other kernel for it)."""
    from alabi_amd import _lib
    from alabi_amd.moves import HMCMove
    d = 64
    prob = ms.problem(d, "ExpSquared")
    s = ms.sampler(prob, 2, 5, moves=[HMCMove(1.0, step_size=0.1, n_leapfrog=1)] * 5)
    with pytest.raises(_lib.AlabiHipError):
        s.run_mcmc(hc.start(prob, 2, 3), 2, skip_initial_state_check=True)


# ------------------------------------------------------------------------------------------------------ 7. run_emcee
def test_run_emcee_with_an_hmc_move(tmp_path):
    """SurrogateModel.run_emcee(sampler_kwargs={"moves": HMCMove(cov)}) end to end on the 2-D Rosenbrock model of
    tests/test_gpu_gaussian_move.py (50 training points), cov from the box widths."""
    from alabi_amd import SurrogateModel
    from alabi_amd.benchmarks import rosenbrock
    from alabi_amd.moves import HMCMove
    sm = SurrogateModel(lnlike_fn=rosenbrock["fn"], bounds=rosenbrock["bounds"], savedir=str(tmp_path), verbose=False, random_state=0)
    sm.init_samples(ntrain=50, ntest=20, sampler="uniform")
    sm.init_gp(kernel="ExpSquaredKernel", fit_amp=True, fit_mean=True, white_noise=-12, hyperopt_method="ml", gp_nopt=1)
    b = np.asarray(rosenbrock["bounds"], dtype=float)
    cov = (0.1 * (b[:, 1] - b[:, 0])) ** 2
    # A box-width cov is no posterior covariance, so the default step size (ndim ** -0.25, which assumes one) does not apply:
    # -rosen / 100 has curvature of about 300 in the corners of [-5, 5]^2, where walkers start, and the leapfrog map is stable
    # for step_size * 1.0 * sqrt(300) < 2 only.  step_size = 0.05 is well inside that.
    sm.run_emcee(nwalkers=16, nsteps=200, min_ess=0, sampler_kwargs={"moves": HMCMove(cov, step_size=0.05, n_leapfrog=8)})
    assert sm.emcee_samples.ndim == 2 and sm.emcee_samples.shape[1] == 2 and sm.emcee_samples.shape[0] > 0
    assert sm.emcee_samples_full.shape == (200, 16, 2)
    assert 0.0 < sm.acc_frac < 1.0
    assert np.all(sm.emcee_samples > b[:, 0]) and np.all(sm.emcee_samples < b[:, 1])
    assert sm.emcee_sampler.last_path == "hmc" and sm.emcee_sampler.last_stream_kernel == "ens_hmc_kernel"
