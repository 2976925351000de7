"""GPU parity of the HMC warm-up (alabi_ens_hmc_adapt: ens_hmc_adapt_kernel; EnsembleSampler.tune_hmc) against
tests/hmc_adapt_numpy.py on the cases of tests/hmc_adapt_cases.py.  Tolerances: the project's HMC tolerances for the same arithmetic
(positions 1e-7, log-probabilities 1e-7 (1 + max|lp|), accept masks and counts identical), the acceptance statistic 1e-7 (1 +
max|lp|) since |d a / d dh| <= 1, H-bar and ln e of a single step 20 sqrt(m) / (m + t0) times that (the update's own amplification
at gamma = 0.05), m exact; over a free run ln e, ln e-bar and the sums of the acceptance statistic within FREE_TOL, ten times the
largest error measured over all cases (NOTES.md "HMC warm-up"); splitting and chunking bit for bit.  tests/test_hmc_adapt_host.py
asserts on the CPU that every model run used here is honest."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import hmc_adapt_cases as hac
import hmc_adapt_numpy as han
import hmc_cases as hc
import moves_shapes_common as ms

pytestmark = pytest.mark.gpu

# Largest |device - model| over the 40-step free runs of all cases, measured on an MI355X: ln e 8.52e-9, ln e-bar 2.49e-9, the
# accept_stat sums 3.37e-9 (all three in case ens3; NOTES.md "HMC warm-up" has the table); ten times the largest for the differing
# summation order.  The cap is 1e-6: beyond it MIN_MARGIN's argument no longer covers the accept tests.
FREE_TOL = 8.6e-8
assert FREE_TOL <= 1e-6


def _sampler(r, **kw):
    from alabi_amd.moves import HMCMove
    cov, eps, L, jitter, _ = r.move
    return ms.sampler(r.prob, r.W, r.seed, n_ensembles=r.E, moves=HMCMove(cov, step_size=eps, n_leapfrog=L, jitter=jitter),
                      **hc.sampler_kw(r.ex), **kw)


def _adapt(s, coords, logp, state, step0, nsteps, par=hac.PAR, chain=None, chain_logp=None, nacc=None, stat=None, thin_by=1):
    """alabi_ens_hmc_adapt on device tensors; returns the status."""
    import torch
    from alabi_amd import _lib
    s._ensure_ens()
    st = _lib.lib().alabi_ens_hmc_adapt(s._ens, _lib.ptr(coords), _lib.ptr(logp), int(step0), int(nsteps), int(thin_by), _lib.ptr(state),
                                        _lib.host_doubles(par), _lib.ptr(chain), _lib.ptr(chain_logp), _lib.ptr(nacc), _lib.ptr(stat),
                                        _lib.current_stream())
    torch.cuda.synchronize()
    return st


def _hmc_plan(s):
    from alabi_amd import _lib
    plan = (C.c_int * 4)()
    _lib.check(_lib.lib().alabi_ens_hmc_plan(s._ens, plan), "alabi_ens_hmc_plan")
    return dict(zip(("threads", "chunk", "lds_bytes", "tiled"), (int(v) for v in plan)))


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype).clone()


# --------------------------------------------------------------------------------------------- 1. stepwise, state injected
@pytest.mark.parametrize("name", list(hac.CASES))
def test_single_steps_from_the_models_state(name):
    """Every step from the model's coords, logp and state: identical accept mask, positions, logp, the acceptance statistic and the
    new state within the tolerances of the module's docstring."""
    import torch
    from alabi_amd import _lib
    r = hac.model_run(name)
    ms.assert_honest(r.stats, name)
    s = _sampler(r)
    n = r.W * r.E
    c_dev, lp_dev, st_dev = _dev(r.p0), _dev(r.logp0), _dev(r.state0)
    assert np.max(np.abs(s.compute_log_prob(c_dev).cpu().numpy() - r.logp0)) < 1e-8 * (1 + np.max(np.abs(r.logp0)))
    nacc = torch.zeros(n, dtype=torch.int64, device="cuda")
    stat = torch.zeros(n, dtype=torch.float64, device="cuda")
    t0, worst = hac.PAR[2], dict(c=0.0, lp=0.0, a=0.0, h=0.0, le=0.0)
    for t in range(hac.ADAPT_STEPS):
        c0, l0, s0 = r.trace[t]
        c_o, l_o, a_o = r.run.chain[t], r.run.chain_logp[t], r.run.alpha[t]
        s_o = r.trace[t + 1][2] if t + 1 < hac.ADAPT_STEPS else r.run.state
        c_dev.copy_(_dev(c0)); lp_dev.copy_(_dev(l0)); st_dev.copy_(_dev(s0)); stat.zero_()
        _lib.check(_adapt(s, c_dev, lp_dev, st_dev, t, 1, nacc=nacc, stat=stat), "alabi_ens_hmc_adapt")
        c_g, l_g, s_g, a_g = c_dev.cpu().numpy(), lp_dev.cpu().numpy(), st_dev.cpu().numpy(), stat.cpu().numpy()
        assert np.array_equal(np.any(c_g != c0, axis=1), np.any(c_o != c0, axis=1)), f"accept mask differs at step {t}"
        bound = 1e-7 * (1 + np.max(np.abs(l_o[np.isfinite(l_o)])))
        m = t + 1.0
        amp = 20.0 * np.sqrt(m) / (m + t0)
        errs = dict(c=np.max(np.abs(c_g - c_o)), lp=np.max(np.abs(l_g - l_o)) / bound * 1e-7, a=np.max(np.abs(a_g - a_o)) / bound * 1e-7,
                    h=np.max(np.abs(s_g[:, 1] - s_o[:, 1])) / (amp * bound) * 1e-7, le=np.max(np.abs(s_g[:, 2] - s_o[:, 2])) / (amp * bound) * 1e-7)
        for k, v in errs.items():
            worst[k] = max(worst[k], float(v))
        assert errs["c"] < 1e-7, f"positions differ at step {t}"
        assert np.max(np.abs(l_g - l_o)) < bound
        assert np.max(np.abs(a_g - a_o)) < bound, f"acceptance statistic differs at step {t}"
        assert np.max(np.abs(s_g[:, 1] - s_o[:, 1])) < amp * bound and np.max(np.abs(s_g[:, 2] - s_o[:, 2])) < amp * bound
        assert np.max(np.abs(s_g[:, 3] - s_o[:, 3])) < amp * bound
        assert np.array_equal(s_g[:, 0], s_o[:, 0]) and np.array_equal(s_g[:, 4], s_o[:, 4])
    print(f"adapt step {name}: worst errors in units of 1e-7 bounds {worst}")
    assert int(nacc.sum()) == int(r.run.nacc.sum()) > 0
    assert _hmc_plan(s)["tiled"] == (1 if name == "tiled" else 0)


# ------------------------------------------------------------------------------------------------------------ 2. free run
@lru_cache(maxsize=None)
def _device_run(name, split=None, chunk_env=None):
    """The 40 warm-up steps of a case on the device from the initial state, in one call or split at ``split``."""
    import torch
    from alabi_amd import _lib
    r = hac.model_run(name)
    s = _sampler(r)
    n = r.W * r.E
    c, st = _dev(r.p0), _dev(r.state0)
    lp = s.compute_log_prob(c)
    nacc = torch.zeros(n, dtype=torch.int64, device="cuda")
    stat = torch.zeros(n, dtype=torch.float64, device="cuda")
    chain = torch.empty((hac.ADAPT_STEPS, n, r.d), dtype=torch.float64, device="cuda")
    chain_lp = torch.empty((hac.ADAPT_STEPS, n), dtype=torch.float64, device="cuda")
    parts = [(0, hac.ADAPT_STEPS)] if split is None else [(0, split), (split, hac.ADAPT_STEPS)]
    for a, b in parts:
        _lib.check(_adapt(s, c, lp, st, a, b - a, chain=chain[a:], chain_logp=chain_lp[a:], nacc=nacc, stat=stat), "alabi_ens_hmc_adapt")
    return dict(coords=c, logp=lp, state=st, nacc=nacc, stat=stat, chain=chain, chain_logp=chain_lp, plan=_hmc_plan(s))


@pytest.mark.parametrize("name", list(hac.CASES))
def test_free_run_against_the_model(name):
    """40 steps in one call: identical acceptance counts, positions within 1e-7, ln e, ln e-bar and the accept_stat sums within
    FREE_TOL."""
    r = hac.model_run(name)
    g = _device_run(name)
    assert np.array_equal(g["nacc"].cpu().numpy(), r.run.nacc)
    scale = 1 + np.max(np.abs(r.run.chain_logp))
    st = g["state"].cpu().numpy()
    err = dict(chain=np.max(np.abs(g["chain"].cpu().numpy() - r.run.chain)), logp=np.max(np.abs(g["chain_logp"].cpu().numpy() - r.run.chain_logp)) / scale,
               ln_e=np.max(np.abs(st[:, 2] - r.run.state[:, 2])), ln_ebar=np.max(np.abs(st[:, 3] - r.run.state[:, 3])),
               hbar=np.max(np.abs(st[:, 1] - r.run.state[:, 1])), stat=np.max(np.abs(g["stat"].cpu().numpy() - r.run.alpha.sum(axis=0))))
    print(f"adapt free run {name}: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    assert err["chain"] < 1e-7 and err["logp"] < 1e-7
    assert np.array_equal(st[:, 0], r.run.state[:, 0]) and np.array_equal(st[:, 4], r.run.state[:, 4])
    assert err["ln_e"] < FREE_TOL and err["ln_ebar"] < FREE_TOL and err["stat"] < FREE_TOL
    assert g["plan"]["chunk"] >= hac.ADAPT_STEPS and g["plan"]["tiled"] == (1 if name == "tiled" else 0)


# ---------------------------------------------------------------------------------------------------------------- 3. bits
def test_splitting_and_chunking_change_no_bit(monkeypatch):
    """One 40-step call, 15 + 25 steps and ALABI_ENS_HMC_CHUNK=7: identical coords, logp, state, chain, counts and sums."""
    import torch
    name = "d5jitter"
    one = _device_run(name)
    two = _device_run(name, split=15)
    monkeypatch.setenv("ALABI_ENS_HMC_CHUNK", "7")
    seven = _device_run(name, chunk_env=7)
    assert seven["plan"]["chunk"] == 7
    for other in (two, seven):
        for key in ("coords", "logp", "state", "chain", "chain_logp", "nacc", "stat"):
            assert torch.equal(one[key], other[key]), key


def test_a_frozen_step_size_is_ens_hmc_kernel():
    """gamma = inf, mu = 0 and HMCMove(step_size=1.0): the adapt entry's chain, logp and n_accept are run_mcmc's on ens_hmc_kernel
    for 20 steps, bit for bit -- the two kernels share the body."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.moves import HMCMove
    r = hac.model_run("d5jitter")
    cov, _, L, jitter, _ = r.move

    def make():
        return ms.sampler(r.prob, r.W, r.seed, moves=HMCMove(cov, step_size=1.0, n_leapfrog=L, jitter=jitter), **hc.sampler_kw(r.ex))
    a = make()
    a.run_mcmc(r.p0, 20, skip_initial_state_check=True)
    assert a.last_stream_kernel == "ens_hmc_kernel"
    b = make()
    c = _dev(r.p0)
    lp = b.compute_log_prob(c)
    state = torch.zeros((r.W, 5), dtype=torch.float64, device="cuda")
    nacc = torch.zeros(r.W, dtype=torch.int64, device="cuda")
    chain = torch.empty((20, r.W, r.d), dtype=torch.float64, device="cuda")
    chain_lp = torch.empty((20, r.W), dtype=torch.float64, device="cuda")
    _lib.check(_adapt(b, c, lp, state, 0, 20, par=(0.8, float("inf"), 10.0, 0.75), chain=chain, chain_logp=chain_lp, nacc=nacc),
               "alabi_ens_hmc_adapt")
    assert torch.equal(chain, a.get_chain_device()) and torch.equal(chain_lp, a.get_chain_device(log_prob=True))
    assert torch.equal(nacc, a._naccept) and 0 < int(nacc.sum()) < 20 * r.W
    st = state.cpu().numpy()
    assert np.all(st[:, 0] == 20) and np.all(st[:, 2] == 0.0) and np.all(st[:, 4] == 0.0)


def test_a_run_after_tune_hmc_continues_the_counter():
    """tune_hmc(nwarmup=60) then run_mcmc(None, 15) equals a fresh sampler built with the tuned move that starts at the same step
    and state."""
    import torch
    r = hac.model_run("matrix")
    s = _sampler(r)
    state = s.tune_hmc(r.p0, nwarmup=60, metric="dense")
    tun = s.hmc_tuning
    assert tun["window_ends"] == [54] and len(tun["step_sizes"]) == 1 and tun["last_path"] == "hmc-adapt" == s.last_path
    assert s._rng_step == 60 and s.iteration == 0 and int(s._naccept.sum()) == 0
    assert tun["cov"].shape == (r.d, r.d) and np.array_equal(s.moves[0][0].cov, tun["cov"]) and s.moves[0][0].step_size == tun["step_size"]
    assert np.array_equal(state.coords, s._coords.cpu().numpy())
    c0, l0 = s._coords.clone(), s._logp.clone()
    s.run_mcmc(None, 15)
    assert s.last_path == "hmc" and s._rng_step == 75
    t = ms.sampler(r.prob, r.W, r.seed, moves=s.moves[0][0], **hc.sampler_kw(r.ex))
    t._coords, t._logp, t._rng_step = c0, l0, 60
    t.run_mcmc(None, 15)
    assert torch.equal(t.get_chain_device(), s.get_chain_device()) and torch.equal(t._naccept, s._naccept)
    assert torch.equal(t.get_chain_device(log_prob=True), s.get_chain_device(log_prob=True))


# ---------------------------------------------------------------------------------------------------------- 4. end to end
def test_tune_hmc_end_to_end():
    """tune_hmc(nwarmup=300) on ms.problem(5, "ExpSquared") under ms.AFFINE, 16 walkers, from identity mass and the default step
    size: the terminal buffer's mean acceptance statistic within 0.1 of 0.8 (twice the model's spread over its seeds), the
    acceptance fraction of the next 200 steps within 0.15 of the model's, the installed covariance the shrunk covariance of the
    last window's positions recomputed in NumPy to 1e-12 relative."""
    from alabi_amd.moves import HMCMove
    E = hac.E2E
    prob, ex = hac.e2e_problem()
    model = hac.e2e_model(E.seed)
    cov, eps, L, jitter, _ = hac.e2e_move()
    s = ms.sampler(prob, E.W, E.seed, moves=HMCMove(cov, step_size=eps, n_leapfrog=L, jitter=jitter), **hc.sampler_kw(ex))
    st = s.tune_hmc(hac.e2e_start(prob, E.seed), nwarmup=E.nwarmup)
    tun = s.hmc_tuning
    print(f"tune_hmc: mean accept stat {tun['mean_accept_stat']:.3f} (model {model.warm.mean_accept_stat:.3f}), step size "
          f"{tun['step_size']:.4f} (model {model.warm.step_size:.4f}), {tun['seconds']:.3f} s")
    assert tun["window_ends"] == [100, 150, 250] == model.warm.window_ends and len(tun["step_sizes"]) == 3
    assert abs(tun["mean_accept_stat"] - 0.8) < 0.1
    want = han.shrunk_covariance(s._last_window_chain.cpu().numpy().reshape(-1, prob.d), "diag")
    assert s._last_window_chain.shape == (100, E.W, prob.d)
    assert np.max(np.abs(tun["cov"] - want) / want) < 1e-12
    assert np.array_equal(s.moves[0][0].cov, tun["cov"]) and s.moves[0][0].n_leapfrog == L
    s.run_mcmc(st, E.nrun, skip_initial_state_check=True)
    acc = float(np.mean(s.acceptance_fraction))
    print(f"tune_hmc: acceptance fraction of the next {E.nrun} steps {acc:.3f} (model {model.acc_frac:.3f})")
    assert s.last_path == "hmc" and abs(acc - model.acc_frac) < 0.15


def test_run_emcee_with_hmc_warmup(tmp_path):
    """run_emcee(sampler_kwargs={"moves": HMCMove(...), "hmc_warmup": 100}) on the 2-D Rosenbrock model of
    tests/test_gpu_hmc_move.py sets sm.hmc_tuning; the run itself is on ens_hmc_kernel."""
    from alabi_amd import SurrogateModel
    from alabi_amd.benchmarks import rosenbrock
    from alabi_amd.moves import HMCMove
    sm = SurrogateModel(lnlike_fn=rosenbrock["fn"], bounds=rosenbrock["bounds"], savedir=str(tmp_path), verbose=False, random_state=0)
    sm.init_samples(ntrain=50, ntest=20, sampler="uniform")
    sm.init_gp(kernel="ExpSquaredKernel", fit_amp=True, fit_mean=True, white_noise=-12, hyperopt_method="ml", gp_nopt=1)
    b = np.asarray(rosenbrock["bounds"], dtype=float)
    cov = (0.1 * (b[:, 1] - b[:, 0])) ** 2
    sm.run_emcee(nwalkers=16, nsteps=200, min_ess=0,
                 sampler_kwargs={"moves": HMCMove(cov, step_size=0.05, n_leapfrog=8), "hmc_warmup": 100, "hmc_target_accept": 0.75})
    tun = sm.hmc_tuning
    assert tun["last_path"] == "hmc-adapt" and tun["window_ends"] == [90] and tun["nwarmup"] == 100 and tun["metric"] == "diag"
    assert tun["step_size"] > 0 and np.all(tun["cov"] > 0) and 0.0 < tun["mean_accept_stat"] <= 1.0
    assert sm.emcee_sampler.last_path == "hmc" and sm.emcee_sampler.moves[0][0].step_size == tun["step_size"]
    assert sm.emcee_samples_full.shape == (200, 16, 2) and 0.0 < sm.acc_frac < 1.0
    assert np.all(sm.emcee_samples > b[:, 0]) and np.all(sm.emcee_samples < b[:, 1])


# ------------------------------------------------------------------------------------------------------------ 5. refusals
def test_library_refusals():
    """ALABI_BAD_ARGUMENT for a two-move table, delta = 1, gamma = 0 (and the other ranges); the same call with Stan's defaults runs."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.moves import HMCMove
    r = hac.model_run("d5jitter")
    s = _sampler(r)
    c, st = _dev(r.p0), _dev(r.state0)
    lp = s.compute_log_prob(c)
    for par in ((1.0, 0.05, 10.0, 0.75), (0.0, 0.05, 10.0, 0.75), (0.8, 0.0, 10.0, 0.75), (0.8, -1.0, 10.0, 0.75), (0.8, 0.05, -1.0, 0.75),
                (0.8, 0.05, 10.0, 0.5), (0.8, 0.05, 10.0, 1.5), (float("nan"), 0.05, 10.0, 0.75)):
        assert _adapt(s, c, lp, st, 0, 2, par=par) == _lib.BAD_ARG, par
    assert _adapt(s, c, lp, None, 0, 2) == _lib.BAD_ARG
    assert torch.equal(c, _dev(r.p0)) and torch.equal(st, _dev(r.state0))
    assert _adapt(s, c, lp, st, 0, 2) == _lib.OK
    two = ms.sampler(r.prob, r.W, r.seed, moves=[HMCMove(0.5, step_size=0.3, n_leapfrog=2), HMCMove(0.7, step_size=0.2, n_leapfrog=1)],
                     **hc.sampler_kw(r.ex))
    assert _adapt(two, _dev(r.p0), lp.clone(), _dev(r.state0), 0, 2) == _lib.BAD_ARG
    stretch = ms.sampler(r.prob, r.W, r.seed, **hc.sampler_kw(r.ex))
    assert _adapt(stretch, _dev(r.p0), lp.clone(), _dev(r.state0), 0, 2) == _lib.BAD_ARG


def test_a_table_beyond_the_lds_is_refused():
    """One full factor at d = 64 takes 64 x 65 x 8 = 33 KB; with 12300 training points the gradient weights take the LDS past
    128 KB: alabi_ens_hmc_adapt is ALABI_BAD_ARGUMENT (there is no other kernel for it)."""
    import torch
    from alabi_amd import EnsembleSampler, HipGP, _lib
    from alabi_amd.moves import HMCMove
    from conftest import make_problem
    d, N, W = 64, 12300, 2
    X, y, h = make_problem(N, d, 7, log_wn=-4.0, ell2=4.0 * d)
    gp = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"])
    gp.compute(X)
    s = EnsembleSampler(W, d, gp, y, np.stack([np.full(d, -3.0), np.full(d, 3.0)], axis=1), seed=3, live_dangerously=True,
                        moves=HMCMove(np.eye(d), step_size=0.1, n_leapfrog=1))
    c = torch.zeros((W, d), dtype=torch.float64, device="cuda")
    lp = s.compute_log_prob(c)
    state = _dev(han.initial_state(W, 0.1))
    assert (d * (d | 1) + N) * 8 > 128 * 1024
    assert _adapt(s, c, lp, state, 0, 2) == _lib.BAD_ARG
    assert torch.equal(state, _dev(han.initial_state(W, 0.1)))
    # the same table on 130 training points runs: it was the LDS
    small = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"])
    small.compute(X[:130])
    t = EnsembleSampler(W, d, small, y[:130], np.stack([np.full(d, -3.0), np.full(d, 3.0)], axis=1), seed=3, live_dangerously=True,
                        moves=HMCMove(np.eye(d), step_size=0.1, n_leapfrog=1))
    assert _adapt(t, c, t.compute_log_prob(c), state, 0, 2) == _lib.OK
