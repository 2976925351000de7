"""GPU parity of the NUTS warm-up (alabi_ens_nuts_adapt: ens_nuts_adapt_kernel; alabi_ens_find_step_size: ens_step_search_kernel;
EnsembleSampler.tune_nuts / find_step_size) against tests/nuts_adapt_numpy.py on the cases of tests/nuts_adapt_cases.py.
Tolerances: those of tests/test_gpu_hmc_adapt.py for the same arithmetic -- leaves, depths and divergence counts identical,
positions 1e-7, log-probabilities and a_t 1e-7 (1 + max|lp|) (a_t is a mean of statistics with |d a / d delta| <= 1), H-bar, ln e
and ln e-bar of a single transition 20 sqrt(m) / (m + t0) times that, m and mu exact; over a free run ln e, ln e-bar and the sum
of a_t within FREE_TOL; splitting, chunking and the frozen step size bit for bit; the search's step counts exact.
tests/test_nuts_adapt_host.py asserts on the CPU that every model run used here is honest.

Case "rq" (rational quadratic) stands where the issue's table names an "Exponential" family: the project has no such kernel; its
non-squared-exponential families are Matern 3/2, Matern 5/2 and the rational quadratic, all on the GENERIC instantiations."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import hmc_cases as hc
import moves_shapes_common as ms
import nuts_adapt_cases as nac
import nuts_adapt_numpy as nan_
import nuts_numpy as nn

pytestmark = pytest.mark.gpu

# Largest |device - model| over the 40-transition free runs of the cases that stay under the cap, measured on an MI355X: ln e
# 9.74e-9 (d1), ln e-bar 1.92e-9 (tiled), the sum of a_t 3.85e-9 (d1) (NOTES.md "NUTS warm-up" has the table); ten times the
# largest for the differing summation order.  The cap is 1e-6: beyond it MIN_MARGIN's argument no longer covers the tree's
# decisions.
FREE_TOL = 9.8e-8
assert FREE_TOL <= 1e-6
LN2 = float(np.log(2.0))


def _move_object(move):
    from alabi_amd.moves import NUTSMove
    cov, eps, depth, jitter, _ = move
    return NUTSMove(cov, step_size=eps, max_depth=depth, jitter=jitter)


def _sampler(r, **kw):
    return ms.sampler(r.prob, r.W, r.seed, n_ensembles=r.E, moves=_move_object(r.move), **hc.sampler_kw(r.ex), **kw)


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype).clone()


def _adapt(s, coords, logp, state, step0, nsteps, par=nac.PAR, chain=None, chain_logp=None, nacc=None, counts=None, leaf_sum=None, stat=None,
           thin_by=1):
    """alabi_ens_nuts_adapt on device tensors; returns the status."""
    import torch
    from alabi_amd import _lib
    s._ensure_ens()
    st = _lib.lib().alabi_ens_nuts_adapt(s._ens, _lib.ptr(coords), _lib.ptr(logp), int(step0), int(nsteps), int(thin_by), _lib.ptr(state),
                                         _lib.host_doubles(par), _lib.ptr(chain), _lib.ptr(chain_logp), _lib.ptr(nacc), _lib.ptr(counts),
                                         _lib.ptr(leaf_sum), _lib.ptr(stat), _lib.current_stream())
    torch.cuda.synchronize()
    return st


def _search(s, coords, logp, step, k_move, ln_e, iters):
    import torch
    from alabi_amd import _lib
    s._ensure_ens()
    st = _lib.lib().alabi_ens_find_step_size(s._ens, _lib.ptr(coords), _lib.ptr(logp), int(step), int(k_move), _lib.ptr(ln_e), _lib.ptr(iters),
                                             _lib.current_stream())
    torch.cuda.synchronize()
    return st


def _nuts_plan(s):
    from alabi_amd import _lib
    plan = (C.c_int * 4)()
    _lib.check(_lib.lib().alabi_ens_nuts_plan(s._ens, plan), "alabi_ens_nuts_plan")
    return dict(zip(("threads", "chunk", "lds_bytes", "tiled"), (int(v) for v in plan)))


def _buffers(n):
    import torch
    return dict(nacc=torch.zeros(n, dtype=torch.int64, device="cuda"), counts=torch.zeros((n, 3), dtype=torch.int64, device="cuda"),
                leaf_sum=torch.zeros(n, dtype=torch.float64, device="cuda"), stat=torch.zeros(n, dtype=torch.float64, device="cuda"))


# --------------------------------------------------------------------------------------------- 1. stepwise, state injected
@pytest.mark.parametrize("name", list(nac.CASES))
def test_single_transitions_from_the_models_state(name):
    """Every transition from the model's coords, logp and state: identical leaves, depths and divergence counts, positions, logp,
    a_t and the new state within the tolerances of the module's docstring."""
    from alabi_amd import _lib
    r = nac.model_run(name)
    assert nan_.honesty(r.rec, ms.MIN_MARGIN)["ok"]
    s = _sampler(r)
    n = r.W * r.E
    c_dev, lp_dev, st_dev = _dev(r.p0), _dev(r.logp0), _dev(r.state0)
    assert np.max(np.abs(s.compute_log_prob(c_dev).cpu().numpy() - r.logp0)) < 1e-8 * (1 + np.max(np.abs(r.logp0)))
    b = _buffers(n)
    t0, worst = nac.PAR[2], dict(c=0.0, lp=0.0, a=0.0, h=0.0, le=0.0)
    model_counts = np.zeros((n, 3), dtype=np.int64)
    for t in range(nac.ADAPT_STEPS):
        c0, l0, s0 = r.trace[t]
        c_o, l_o, a_o = r.run.chain[t], r.run.chain_logp[t], r.run.alpha[t]
        s_o = r.trace[t + 1][2] if t + 1 < nac.ADAPT_STEPS else r.run.state
        c_dev.copy_(_dev(c0)); lp_dev.copy_(_dev(l0)); st_dev.copy_(_dev(s0)); b["stat"].zero_(); b["counts"].zero_()
        _lib.check(_adapt(s, c_dev, lp_dev, st_dev, t, 1, **b), "alabi_ens_nuts_adapt")
        c_g, l_g, s_g, a_g = c_dev.cpu().numpy(), lp_dev.cpu().numpy(), st_dev.cpu().numpy(), b["stat"].cpu().numpy()
        model_counts += b["counts"].cpu().numpy()
        bound = 1e-7 * (1 + np.max(np.abs(l_o[np.isfinite(l_o)])))
        m = t + 1.0
        amp = 20.0 * np.sqrt(m) / (m + t0)
        errs = dict(c=np.max(np.abs(c_g - c_o)), lp=np.max(np.abs(l_g - l_o)) / bound * 1e-7, a=np.max(np.abs(a_g - a_o)) / bound * 1e-7,
                    h=np.max(np.abs(s_g[:, 1] - s_o[:, 1])) / (amp * bound) * 1e-7, le=np.max(np.abs(s_g[:, 2] - s_o[:, 2])) / (amp * bound) * 1e-7)
        for k, v in errs.items():
            worst[k] = max(worst[k], float(v))
        assert errs["c"] < 1e-7, f"positions differ at transition {t}"
        assert np.max(np.abs(l_g - l_o)) < bound
        assert np.max(np.abs(a_g - a_o)) < bound, f"a_t differs at transition {t}"
        assert np.max(np.abs(s_g[:, 1] - s_o[:, 1])) < amp * bound and np.max(np.abs(s_g[:, 2] - s_o[:, 2])) < amp * bound
        assert np.max(np.abs(s_g[:, 3] - s_o[:, 3])) < amp * bound
        assert np.array_equal(s_g[:, 0], s_o[:, 0]) and np.array_equal(s_g[:, 4], s_o[:, 4])
    print(f"nuts adapt transition {name}: worst errors in units of 1e-7 bounds {worst}")
    assert np.array_equal(model_counts, r.run.counts), "leaves, depths or divergences differ"
    assert np.array_equal(b["nacc"].cpu().numpy(), r.run.nacc) and int(r.run.nacc.sum()) > 0
    assert _nuts_plan(s)["tiled"] == (1 if name == "tiled" else 0)
    if name == "divergent":
        assert r.run.counts[:, 2].sum() > 0


# ------------------------------------------------------------------------------------------------------------ 2. free run
@lru_cache(maxsize=None)
def _device_run(name, split=None, chunk_env=None):
    """The 40 warm-up transitions of a case on the device from the initial state, in one call or split at ``split``."""
    import torch
    from alabi_amd import _lib
    r = nac.model_run(name)
    s = _sampler(r)
    n = r.W * r.E
    c, st = _dev(r.p0), _dev(r.state0)
    lp = s.compute_log_prob(c)
    b = _buffers(n)
    chain = torch.empty((nac.ADAPT_STEPS, n, r.d), dtype=torch.float64, device="cuda")
    chain_lp = torch.empty((nac.ADAPT_STEPS, n), dtype=torch.float64, device="cuda")
    parts = [(0, nac.ADAPT_STEPS)] if split is None else [(0, split), (split, nac.ADAPT_STEPS)]
    for a, e in parts:
        _lib.check(_adapt(s, c, lp, st, a, e - a, chain=chain[a:], chain_logp=chain_lp[a:], **b), "alabi_ens_nuts_adapt")
    handle_counts, handle_acc = s.nuts_counts()
    assert not handle_counts.any() and not handle_acc.any()       # warm-up is no part of alabi_ens_nuts_stats
    return dict(coords=c, logp=lp, state=st, chain=chain, chain_logp=chain_lp, plan=_nuts_plan(s), **b)


@pytest.mark.parametrize("name", list(nac.CASES))
def test_free_run_against_the_model(name):
    """40 transitions in one call: identical counts, positions within 1e-7, ln e, ln e-bar and the sum of a_t within FREE_TOL."""
    r = nac.model_run(name)
    g = _device_run(name)
    assert np.array_equal(g["nacc"].cpu().numpy(), r.run.nacc)
    assert np.array_equal(g["counts"].cpu().numpy(), r.run.counts)
    scale = 1 + np.max(np.abs(r.run.chain_logp))
    st = g["state"].cpu().numpy()
    err = dict(chain=np.max(np.abs(g["chain"].cpu().numpy() - r.run.chain)), logp=np.max(np.abs(g["chain_logp"].cpu().numpy() - r.run.chain_logp)) / scale,
               ln_e=np.max(np.abs(st[:, 2] - r.run.state[:, 2])), ln_ebar=np.max(np.abs(st[:, 3] - r.run.state[:, 3])),
               hbar=np.max(np.abs(st[:, 1] - r.run.state[:, 1])), stat=np.max(np.abs(g["stat"].cpu().numpy() - r.run.alpha.sum(axis=0))),
               leaf_sum=np.max(np.abs(g["leaf_sum"].cpu().numpy() - r.run.a_sum)))
    print(f"nuts adapt free run {name}: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    assert err["chain"] < 1e-7 and err["logp"] < 1e-7
    assert np.array_equal(st[:, 0], r.run.state[:, 0]) and np.array_equal(st[:, 4], r.run.state[:, 4])
    assert err["ln_e"] < FREE_TOL and err["ln_ebar"] < FREE_TOL and err["stat"] < FREE_TOL
    assert g["plan"]["chunk"] >= nac.ADAPT_STEPS and g["plan"]["tiled"] == (1 if name == "tiled" else 0)


# ---------------------------------------------------------------------------------------------------------------- 3. bits
def test_splitting_and_chunking_change_no_bit(monkeypatch):
    """One 40-transition call, 15 + 25 and ALABI_ENS_NUTS_CHUNK=7: identical coords, logp, state, chain, counts and sums."""
    import torch
    name = "ens3"
    one = _device_run(name)
    two = _device_run(name, split=15)
    monkeypatch.setenv("ALABI_ENS_NUTS_CHUNK", "7")
    seven = _device_run(name, chunk_env=7)
    assert seven["plan"]["chunk"] == 7
    for other in (two, seven):
        for key in ("coords", "logp", "state", "chain", "chain_logp", "nacc", "counts", "leaf_sum", "stat"):
            assert torch.equal(one[key], other[key]), key


def test_a_frozen_step_size_is_ens_nuts_kernel():
    """gamma = inf, mu = 0 and NUTSMove(step_size=1.0): the adapt entry's chain, logp, n_accept, counts and sum of a are run_mcmc's
    on ens_nuts_kernel for 20 transitions, bit for bit -- the two kernels share the body."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.moves import NUTSMove
    r = nac.model_run("ens3")
    cov, _, depth, jitter, _ = r.move
    n = r.W * r.E

    def make():
        return ms.sampler(r.prob, r.W, r.seed, n_ensembles=r.E, moves=NUTSMove(cov, step_size=1.0, max_depth=depth, jitter=jitter),
                          **hc.sampler_kw(r.ex))
    a = make()
    a.run_mcmc(r.p0, 20, skip_initial_state_check=True)
    assert a.last_stream_kernel == "ens_nuts_kernel"
    b = make()
    c = _dev(r.p0)
    lp = b.compute_log_prob(c)
    state = torch.zeros((n, 5), dtype=torch.float64, device="cuda")
    buf = _buffers(n)
    chain = torch.empty((20, n, r.d), dtype=torch.float64, device="cuda")
    chain_lp = torch.empty((20, n), dtype=torch.float64, device="cuda")
    _lib.check(_adapt(b, c, lp, state, 0, 20, par=(0.8, float("inf"), 10.0, 0.75), chain=chain, chain_logp=chain_lp, **buf),
               "alabi_ens_nuts_adapt")
    assert torch.equal(chain, a.get_chain_device()) and torch.equal(chain_lp, a.get_chain_device(log_prob=True))
    assert torch.equal(buf["nacc"], a._naccept) and 0 < int(buf["nacc"].sum()) <= 20 * n
    counts, acc = a.nuts_counts()
    assert np.array_equal(buf["counts"].cpu().numpy(), counts) and np.array_equal(buf["leaf_sum"].cpu().numpy(), acc) and counts[:, 0].sum() > 20 * n
    st = state.cpu().numpy()
    assert np.all(st[:, 0] == 20) and np.all(st[:, 2] == 0.0) and np.all(st[:, 4] == 0.0)


# -------------------------------------------------------------------------------------------------------------- 4. search
@pytest.mark.parametrize("name", list(nac.SEARCH_CASES))
def test_search_against_the_model(name):
    """ln e moves by the model's whole number of ln 2 steps, iters is the model's, and coords and logp keep every bit."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.moves import HMCMove
    m = nac.model_search(name)
    c = m.case
    if c.table == "nuts":
        moves = _move_object(c.moves[0])
    else:
        moves = [(HMCMove(mv[0], step_size=mv[1], n_leapfrog=mv[2], jitter=mv[3]), mv[4]) for mv in c.moves]
    s = ms.sampler(c.prob, c.W, c.seed, n_ensembles=c.E, moves=moves, **hc.sampler_kw(c.ex))
    n = c.W * c.E
    coords = _dev(c.p0)
    logp = s.compute_log_prob(coords)
    c_before, lp_before = coords.clone(), logp.clone()
    ln_e = torch.full((n,), c.ln_e, dtype=torch.float64, device="cuda")
    iters = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    _lib.check(_search(s, coords, logp, nac.SEARCH_STEP, c.k_move, ln_e, iters), "alabi_ens_find_step_size")
    got = np.round((ln_e.cpu().numpy() - c.ln_e) / LN2).astype(np.int64)
    want = np.round((m.ln_e - c.ln_e) / LN2).astype(np.int64)
    print(f"search {name}: steps {got.tolist()}, iters {iters.cpu().numpy().tolist()}")
    assert np.array_equal(got, want) and np.array_equal(iters.cpu().numpy(), m.iters)
    assert np.max(np.abs(ln_e.cpu().numpy() - m.ln_e)) < 1e-12
    assert torch.equal(coords, c_before) and torch.equal(logp, lp_before)
    if name == "cap":
        assert np.all(m.iters == nan_.SEARCH_CAP)
    # iters may be null, and the result does not depend on it
    again = torch.full((n,), c.ln_e, dtype=torch.float64, device="cuda")
    _lib.check(_search(s, coords, logp, nac.SEARCH_STEP, c.k_move, again, None), "alabi_ens_find_step_size")
    assert torch.equal(again, ln_e)


def test_find_step_size_method():
    """EnsembleSampler.find_step_size starts at the move's resolved step size and reads the sampler's draw counter; nothing moves."""
    m = nac.model_search("d24")
    c = m.case
    s = ms.sampler(c.prob, c.W, c.seed, moves=_move_object(c.moves[0]), **hc.sampler_kw(c.ex))
    s._rng_step = nac.SEARCH_STEP
    out = s.find_step_size(c.p0)
    assert np.array_equal(out["iters"], m.iters) and np.max(np.abs(np.log(out["step_sizes"]) - m.ln_e)) < 1e-12
    assert abs(out["step_size"] - np.exp(np.mean(m.ln_e))) < 1e-12 and s._rng_step == nac.SEARCH_STEP and s.iteration == 0
    assert np.array_equal(s._coords.cpu().numpy(), c.p0)


# ---------------------------------------------------------------------------------------------------------- 5. end to end
def test_tune_nuts_end_to_end():
    """tune_nuts(nwarmup=300) on the problem of test_tune_hmc_end_to_end (ms.problem(5, "ExpSquared") under ms.AFFINE, 16 walkers,
    identity mass, the default step size, max_depth 6) with the search: the terminal buffer's mean acceptance statistic inside the
    band of the NumPy model over five seeds (tests/test_nuts_adapt_host.py, NOTES.md "NUTS warm-up"); the move afterwards is a
    NUTSMove with what was found; run_mcmc(None, n) continues the counter and nuts_stats counts the sampling transitions alone."""
    import torch
    from alabi_amd.moves import NUTSMove
    E = nac.E2E
    prob, ex = nac.e2e_problem()
    cov, eps, depth, jitter, _ = nac.e2e_move()
    s = ms.sampler(prob, E.W, E.seed, moves=NUTSMove(cov, step_size=eps, max_depth=depth, jitter=jitter), **hc.sampler_kw(ex))
    st = s.tune_nuts(nac.e2e_start(prob, E.seed), nwarmup=E.nwarmup)
    tun = s.nuts_tuning
    print(f"tune_nuts: mean accept stat {tun['mean_accept_stat']:.4f}, step size {tun['step_size']:.4f}, mean depth {tun['mean_depth']:.2f}, "
          f"divergences {tun['divergences']}, search iters {[(int(i.min()), int(i.max())) for i in tun['search_iters']]}, {tun['seconds']:.3f} s")
    assert tun["window_ends"] == [100, 150, 250] and len(tun["step_sizes"]) == 3 and len(tun["search_iters"]) == 4
    assert tun["last_path"] == "nuts-adapt" == s.last_path and tun["nwarmup"] == E.nwarmup and tun["metric"] == "diag"
    lo, hi = nac.E2E_BAND
    assert lo < tun["mean_accept_stat"] < hi
    mv = s.moves[0][0]
    assert isinstance(mv, NUTSMove) and mv.step_size == tun["step_size"] and np.array_equal(mv.cov, tun["cov"]) and mv.max_depth == depth
    want = nan_.han.shrunk_covariance(s._last_window_chain.cpu().numpy().reshape(-1, prob.d), "diag")
    assert np.max(np.abs(tun["cov"] - want) / want) < 1e-12
    assert s._rng_step == E.nwarmup and s.iteration == 0 and int(s._naccept.sum()) == 0
    assert s.nuts_stats["transitions"] == 0 and s.nuts_stats["divergences"] == 0 and not s.nuts_counts()[0].any()
    assert np.array_equal(st.coords, s._coords.cpu().numpy())
    c0, l0 = s._coords.clone(), s._logp.clone()
    s.run_mcmc(None, E.nrun)
    assert s.last_path == "nuts" and s._rng_step == E.nwarmup + E.nrun and s.iteration == E.nrun
    assert s.nuts_stats["transitions"] == E.nrun * E.W
    t = ms.sampler(prob, E.W, E.seed, moves=mv, **hc.sampler_kw(ex))
    t._coords, t._logp, t._rng_step = c0, l0, E.nwarmup
    t.run_mcmc(None, E.nrun)
    assert torch.equal(t.get_chain_device(), s.get_chain_device()) and torch.equal(t._naccept, s._naccept)
    print(f"tune_nuts: the next {E.nrun} transitions: {s.nuts_stats}")


def _direct(r, nsteps, search):
    """What tune_nuts(nwarmup=nsteps, metric=None) must do, by the library's entries: the search at step 0 (or the initial state),
    then ONE adapt call; returns the state and the search's iteration counts."""
    import torch
    from alabi_amd import _lib
    s = _sampler(r)
    n = r.W * r.E
    c = _dev(r.p0)
    lp = s.compute_log_prob(c)
    iters = None
    if search:
        ln_e = torch.full((n,), float(np.log(r.move[1])), dtype=torch.float64, device="cuda")
        iters = torch.zeros(n, dtype=torch.int32, device="cuda")
        _lib.check(_search(s, c, lp, 0, 0, ln_e, iters), "alabi_ens_find_step_size")
        state = _dev(nan_.searched_state(ln_e.cpu().numpy()))
    else:
        state = _dev(nan_.han.initial_state(n, r.move[1]))
    _lib.check(_adapt(s, c, lp, state, 0, nsteps), "alabi_ens_nuts_adapt")
    return state.cpu().numpy(), c, iters


@pytest.mark.parametrize("search", [True, False])
def test_tune_nuts_is_the_search_and_one_adapt_call(search):
    """metric=None, 15 transitions: tune_nuts' walkers and pooled step size are those of the search (init_step_size="search") or of
    the move's own step size (None) followed by one alabi_ens_nuts_adapt call, bit for bit."""
    import torch
    r = nac.model_run("ens3")
    s = _sampler(r)
    s.tune_nuts(r.p0, nwarmup=15, metric=None, init_step_size="search" if search else None)
    state, c, iters = _direct(r, 15, search)
    tun = s.nuts_tuning
    assert tun["step_size"] == float(np.exp(np.mean(state[:, 3]))) and tun["cov"] is None and tun["window_ends"] == []
    assert torch.equal(s._coords, c) and s._rng_step == 15
    if search:
        assert len(tun["search_iters"]) == 1 and np.array_equal(tun["search_iters"][0], iters.cpu().numpy())
    else:
        assert tun["search_iters"] == []
    assert s.moves[0][0].jitter == r.move[3] and s.moves[0][0].max_depth == r.move[2]


def test_run_emcee_with_nuts_warmup(tmp_path):
    """run_emcee(sampler_kwargs={"moves": NUTSMove(...), "nuts_warmup": 100}) on the 2-D Rosenbrock model of
    tests/test_gpu_hmc_adapt.py sets sm.nuts_tuning; the run itself is on ens_nuts_kernel."""
    from alabi_amd import SurrogateModel
    from alabi_amd.benchmarks import rosenbrock
    from alabi_amd.moves import NUTSMove
    sm = SurrogateModel(lnlike_fn=rosenbrock["fn"], bounds=rosenbrock["bounds"], savedir=str(tmp_path), verbose=False, random_state=0)
    sm.init_samples(ntrain=50, ntest=20, sampler="uniform")
    sm.init_gp(kernel="ExpSquaredKernel", fit_amp=True, fit_mean=True, white_noise=-12, hyperopt_method="ml", gp_nopt=1)
    b = np.asarray(rosenbrock["bounds"], dtype=float)
    cov = (0.1 * (b[:, 1] - b[:, 0])) ** 2
    sm.run_emcee(nwalkers=16, nsteps=100, min_ess=0,
                 sampler_kwargs={"moves": NUTSMove(cov, step_size=0.05, max_depth=5), "nuts_warmup": 100, "nuts_target_accept": 0.75})
    tun = sm.nuts_tuning
    assert tun["last_path"] == "nuts-adapt" and tun["window_ends"] == [90] and tun["nwarmup"] == 100 and tun["metric"] == "diag"
    assert tun["step_size"] > 0 and np.all(tun["cov"] > 0) and 0.0 < tun["mean_accept_stat"] <= 1.0 and len(tun["search_iters"]) == 2
    assert sm.emcee_sampler.last_path == "nuts" and sm.emcee_sampler.moves[0][0].step_size == tun["step_size"]
    assert sm.nuts_stats["transitions"] == 100 * 16
    assert sm.emcee_samples_full.shape == (100, 16, 2)
    assert np.all(sm.emcee_samples > b[:, 0]) and np.all(sm.emcee_samples < b[:, 1])


# ------------------------------------------------------------------------------------------------------------ 6. refusals
def test_library_refusals():
    """ALABI_BAD_ARGUMENT for a two-move table, a kind-6 table, da_par out of range; the same call with Stan's defaults runs.
    alabi_ens_hmc_adapt still refuses the NUTS table, and the search refuses a table without a gradient move."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.moves import HMCMove, NUTSMove
    r = nac.model_run("d5m52")
    s = _sampler(r)
    c, st = _dev(r.p0), _dev(r.state0)
    lp = s.compute_log_prob(c)
    for par in ((1.0, 0.05, 10.0, 0.75), (0.0, 0.05, 10.0, 0.75), (0.8, 0.0, 10.0, 0.75), (0.8, -1.0, 10.0, 0.75), (0.8, 0.05, -1.0, 0.75),
                (0.8, 0.05, 10.0, 0.5), (0.8, 0.05, 10.0, 1.5), (float("nan"), 0.05, 10.0, 0.75)):
        assert _adapt(s, c, lp, st, 0, 2, par=par) == _lib.BAD_ARG, par
    assert _adapt(s, c, lp, None, 0, 2) == _lib.BAD_ARG
    assert torch.equal(c, _dev(r.p0)) and torch.equal(st, _dev(r.state0))
    assert _lib.lib().alabi_ens_hmc_adapt(s._ens, _lib.ptr(c), _lib.ptr(lp), 0, 2, 1, _lib.ptr(st), _lib.host_doubles(nac.PAR), None, None, None,
                                          None, _lib.current_stream()) == _lib.BAD_ARG
    assert _adapt(s, c, lp, st, 0, 2) == _lib.OK                      # counts, sums and accept_stat may all be null
    two = ms.sampler(r.prob, r.W, r.seed, moves=[NUTSMove(0.5, step_size=0.3, max_depth=2), NUTSMove(0.7, step_size=0.2, max_depth=1)],
                     **hc.sampler_kw(r.ex))
    assert _adapt(two, _dev(r.p0), lp.clone(), _dev(r.state0), 0, 2) == _lib.BAD_ARG
    ln_e = torch.zeros(r.W, dtype=torch.float64, device="cuda")
    assert _search(two, _dev(r.p0), lp.clone(), 0, 2, ln_e, None) == _lib.BAD_ARG       # k_move beyond the table
    assert _search(two, _dev(r.p0), lp.clone(), 0, 1, ln_e, None) == _lib.OK
    hmc = ms.sampler(r.prob, r.W, r.seed, moves=HMCMove(0.5, step_size=0.3, n_leapfrog=2), **hc.sampler_kw(r.ex))
    assert _adapt(hmc, _dev(r.p0), lp.clone(), _dev(r.state0), 0, 2) == _lib.BAD_ARG
    stretch = ms.sampler(r.prob, r.W, r.seed, **hc.sampler_kw(r.ex))
    assert _adapt(stretch, _dev(r.p0), lp.clone(), _dev(r.state0), 0, 2) == _lib.BAD_ARG
    assert _search(stretch, _dev(r.p0), lp.clone(), 0, 0, ln_e, None) == _lib.BAD_ARG


def test_a_table_beyond_the_lds_is_refused():
    """One full factor at d = 64 takes 64 x 65 x 8 = 33 KB; with 12300 training points the gradient weights take the LDS past 128 KB
    for both kernels: alabi_ens_nuts_adapt and alabi_ens_find_step_size are ALABI_BAD_ARGUMENT and write nothing."""
    import torch
    from alabi_amd import EnsembleSampler, HipGP, _lib
    from alabi_amd.moves import NUTSMove
    from conftest import make_problem
    d, N, W = 64, 12300, 2
    X, y, h = make_problem(N, d, 7, log_wn=-4.0, ell2=4.0 * d)
    box = np.stack([np.full(d, -3.0), np.full(d, 3.0)], axis=1)
    c = torch.zeros((W, d), dtype=torch.float64, device="cuda")
    state0 = nan_.han.initial_state(W, 0.1)

    def make(n):
        gp = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"])
        gp.compute(X[:n])
        return EnsembleSampler(W, d, gp, y[:n], box, seed=3, live_dangerously=True, moves=NUTSMove(np.eye(d), step_size=0.1, max_depth=1))
    s = make(N)
    lp = s.compute_log_prob(c)
    state = _dev(state0)
    ln_e = torch.zeros(W, dtype=torch.float64, device="cuda")
    assert (d * (d | 1) + N) * 8 > 128 * 1024
    assert _adapt(s, c, lp, state, 0, 2) == _lib.BAD_ARG and _search(s, c, lp, 0, 0, ln_e, None) == _lib.BAD_ARG
    assert torch.equal(state, _dev(state0)) and not ln_e.any()
    # the same table on 130 training points runs: it was the LDS
    t = make(130)
    assert _adapt(t, c, t.compute_log_prob(c), state, 0, 2) == _lib.OK
    assert _search(t, c, t.compute_log_prob(c), 0, 0, ln_e, None) == _lib.OK
