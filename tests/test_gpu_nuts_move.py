"""GPU parity of the NUTS move (alabi_amd.moves.NUTSMove: ens_nuts_kernel) against tests/nuts_numpy.py on the problems of
tests/moves_shapes_common.py (N = 65 / 130 on [-3, 3]^d, one case whose training set needs a second tile).  Tolerances: positions of
single transitions and chains 1e-7, their log-probabilities 1e-7 (1 + max|lp|); traces, acceptance counts and the integer sums of
alabi_ens_nuts_stats identical; the sum of the acceptance statistic 1e-6 relative; call splitting bit for bit.
tests/test_nuts_move_host.py asserts on the CPU that no decision of a model run used here is a near tie."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import hmc_cases as hc
import moves_shapes_common as ms
import nuts_cases as nc
import nuts_numpy as nn

pytestmark = pytest.mark.gpu


def _dev(torch, *arrays):
    return [torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in arrays]


def _last_path(s):
    from alabi_amd import _lib
    path = C.c_int(-1)
    _lib.check(_lib.lib().alabi_ens_last_path(s._ens, C.byref(path)), "alabi_ens_last_path")
    return path.value


def _nuts_plan(s):
    from alabi_amd import _lib
    plan = (C.c_int * 4)()
    _lib.check(_lib.lib().alabi_ens_nuts_plan(s._ens, plan), "alabi_ens_nuts_plan")
    return dict(zip(("threads", "chunk", "lds_bytes", "tiled"), (int(v) for v in plan)))


# ------------------------------------------------------------------------------------------- 1., 2. injected transitions
@pytest.mark.parametrize("name", nc.STEP_NAMES, ids=str)
def test_transition_with_injected_randoms(name):
    """Same draws -> identical trace [W, 4] (depth reached, leaves, stop reason, taken), positions within 1e-7 and
    log-probabilities within 1e-7 (1 + max|lp|), over 6 transitions of 8 walkers from the model's state: the grid at max_depth 3, a
    matrix cov, max_depth 1, the divergent case (max_depth 4) and a max_depth 5 case."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.moves import NUTSMove
    run = nc.model_steps(name)
    assert nn.honesty(run.rec, ms.MIN_MARGIN)["ok"]
    W, prob = nc.W_STEP, run.prob
    s = ms.sampler(prob, W, 1, moves=NUTSMove(run.cov, step_size=run.e, max_depth=run.depth), **hc.sampler_kw(run.ex))
    c_dev = torch.as_tensor(run.p0, device="cuda").clone()
    lp_dev = s.compute_log_prob(c_dev)
    assert np.max(np.abs(lp_dev.cpu().numpy() - run.lp0)) < 1e-8 * (1 + np.max(np.abs(run.lp0)))
    nacc = torch.zeros(W, dtype=torch.int64, device="cuda")
    trace = torch.full((W, 4), -1, dtype=torch.int32, device="cuda")
    lib, stream = _lib.lib(), _lib.current_stream()
    worst_c, worst_lp, a_model = 0.0, 0.0, np.zeros(W)
    counts_model = np.zeros((W, 3), dtype=np.int64)
    for it, (dr, c_o, l_o, tr_o, a_o) in enumerate(run.steps):
        z, dirw, ul, ut = _dev(torch, dr.z, dr.dirw.view(np.int32), dr.u_leaf, dr.u_tree)
        _lib.check(lib.alabi_ens_step_with_randoms_nuts(s._ens, _lib.ptr(c_dev), _lib.ptr(lp_dev), 0, float(dr.e), _lib.ptr(z), _lib.ptr(dirw),
                                                        _lib.ptr(ul), _lib.ptr(ut), _lib.ptr(trace), _lib.ptr(nacc), stream),
                   "alabi_ens_step_with_randoms_nuts")
        torch.cuda.synchronize()
        c_g, l_g, tr_g = c_dev.cpu().numpy(), lp_dev.cpu().numpy(), trace.cpu().numpy()
        scale = 1 + np.max(np.abs(l_o))
        err_c, err_lp = np.max(np.abs(c_g - c_o)), np.max(np.abs(l_g - l_o)) / scale
        print(f"nuts step {name} it {it}: position error {err_c:.3e}, relative lp error {err_lp:.3e}")
        assert np.array_equal(tr_g, tr_o), f"trace differs at iteration {it}:\n{tr_g}\n{tr_o}"
        worst_c, worst_lp = max(worst_c, err_c), max(worst_lp, err_lp)
        assert err_c < 1e-7, f"positions differ at iteration {it}"
        assert err_lp < 1e-7
        counts_model[:, 0] += tr_o[:, 1]; counts_model[:, 1] += tr_o[:, 0]; counts_model[:, 2] += tr_o[:, 2] == nn.STOP_DIVERGENT
        a_model += a_o
        c_dev.copy_(torch.as_tensor(c_o, device="cuda"))
        lp_dev.copy_(torch.as_tensor(l_o, device="cuda"))
    print(f"nuts step {name}: max position error {worst_c:.3e}, max relative lp error {worst_lp:.3e}")
    assert np.array_equal(nacc.cpu().numpy(), sum(tr[:, 3] for _, _, _, tr, _ in run.steps))
    counts, a_sum = s.nuts_counts()
    assert np.array_equal(counts, counts_model)
    assert np.all(np.abs(a_sum - a_model) <= 1e-6 * np.abs(a_model))
    plan = _nuts_plan(s)
    assert plan["threads"] in (256, 512) and plan["chunk"] == 1 and plan["tiled"] == 0
    if name == "divergent":
        assert counts[:, 2].sum() >= 5


# ------------------------------------------------------------------------------------------------- 3. exported draws
def test_exported_draws_are_the_models():
    """alabi_ens_export_nuts_draws returns the model's move, direction words and uniforms bit for bit, its e to 4 ulp and its
    normals to 1e-13; with n_ensembles = 3 and jitter e differs per ensemble."""
    import torch
    from alabi_amd import _lib
    d, W, E, seed, step, depth = 5, 6, 3, 77, (1 << 33) + 12, 4
    prob = ms.problem(d, "ExpSquared")
    spec = [(np.full(d, 0.3), 0.4, 4, 1.5, 0.5), (0.7, None, 2, 2.0, 0.5)]
    s = ms.sampler(prob, W, seed, n_ensembles=E, moves=nc.moves_objects(spec))
    s._ensure_ens()
    n, nl = W * E, (1 << depth) - 1
    move = torch.empty(E, dtype=torch.int32, device="cuda")
    e = torch.empty(E, dtype=torch.float64, device="cuda")
    z = torch.empty((n, d), dtype=torch.float64, device="cuda")
    dirw = torch.empty(n, dtype=torch.int32, device="cuda")
    ul = torch.empty((n, nl), dtype=torch.float64, device="cuda")
    ut = torch.empty((n, depth), dtype=torch.float64, device="cuda")
    _, cum, p0, p1, _ = nn.move_table(spec, d)
    es, moves_seen = [], set()
    for st in (step, step + 1, step + 2, step + 3):
        _lib.check(_lib.lib().alabi_ens_export_nuts_draws(s._ens, st, depth, _lib.ptr(move), _lib.ptr(e), _lib.ptr(z), _lib.ptr(dirw),
                                                          _lib.ptr(ul), _lib.ptr(ut), _lib.current_stream()), "alabi_ens_export_nuts_draws")
        torch.cuda.synchronize()
        for k in range(E):
            mi_o, e_o, z_o, dir_o, ul_o, ut_o = nn.draw_nuts_randoms(seed, st, np.arange(W) + k * W, k * W, cum, p0, p1, d, max_depth=depth)
            sl = slice(k * W, (k + 1) * W)
            assert int(move[k]) == mi_o
            assert abs(e[k].item() - e_o) <= 4 * np.spacing(e_o)
            assert np.max(np.abs(z[sl].cpu().numpy() - z_o)) < 1e-13
            assert np.array_equal(dirw[sl].cpu().numpy().view(np.uint32), dir_o)
            assert np.array_equal(ul[sl].cpu().numpy(), ul_o) and np.array_equal(ut[sl].cpu().numpy(), ut_o)
            moves_seen.add(mi_o)
        es.append(e.cpu().numpy().copy())
    assert len(set(es[0])) == E                 # one jitter draw per step and ENSEMBLE
    assert moves_seen == {0, 1}
    assert p0[1] == d ** -0.25                  # step_size=None resolved
    assert _lib.lib().alabi_ens_export_nuts_draws(s._ens, step, 11, _lib.ptr(move), _lib.ptr(e), _lib.ptr(z), _lib.ptr(dirw), _lib.ptr(ul),
                                                  _lib.ptr(ut), _lib.current_stream()) == _lib.BAD_ARG


# ------------------------------------------------------------------------------------------------ 4. production chains
@lru_cache(maxsize=None)
def _device_chain(name):
    import torch  # noqa: F401
    run = nc.model_chain(name)

    def make():
        return ms.sampler(run.prob, run.W, run.seed, n_ensembles=run.E, moves=nc.moves_objects(run.spec), **hc.sampler_kw(run.ex))
    s = make()
    s.run_mcmc(run.p0, nc.CHAIN_STEPS, skip_initial_state_check=True)
    counts, a_sum = s.nuts_counts()
    out = dict(chain=s.get_chain_device().clone(), logp=s.get_chain_device(log_prob=True).clone(), nacc=s._naccept.clone(),
               path=_last_path(s), plan=_nuts_plan(s), last_path=s.last_path, kernel=s.last_stream_kernel, counts=counts, a_sum=a_sum,
               stats=s.nuts_stats)
    s.run_mcmc(None, nc.CONT_STEPS)
    out["cont"] = s.get_chain_device()[nc.CHAIN_STEPS:].clone()
    out["nacc_cont"] = s._naccept.clone()
    out["counts_cont"], out["a_sum_cont"] = s.nuts_counts(reset=True)
    out["counts_reset"], out["a_sum_reset"] = s.nuts_counts()
    t = make()
    t.run_mcmc(run.p0, nc.CHAIN_STEPS, thin_by=nc.THIN, skip_initial_state_check=True)
    out["thin"] = t.get_chain_device().clone()
    out["thin_logp"] = t.get_chain_device(log_prob=True).clone()
    return out


@pytest.mark.parametrize("name", list(nc.CHAIN_CASES))
def test_production_chain(name):
    """40 transitions, a 10-step continuation (step0) and a run with thin_by = 3 on ens_nuts_kernel against the model: chains
    within 1e-7, identical acceptance counts and integer sums of alabi_ens_nuts_stats, the sum of a within 1e-6 relative, path 6.
    With n_ensembles = 3 the jitter and the move choice are per ensemble, drawn at its walker 0."""
    run = nc.model_chain(name)
    for rec in run.recs:
        assert nn.honesty(rec, ms.MIN_MARGIN)["ok"]
    g = _device_chain(name)
    assert g["path"] == 6 and g["last_path"] == "nuts" and g["kernel"] == "ens_nuts_kernel"
    assert g["plan"]["tiled"] == (1 if name == "tiled" else 0), g["plan"]
    scale = 1 + np.max(np.abs(run.logp))
    err = np.max(np.abs(g["chain"].cpu().numpy() - run.chain), axis=(1, 2))
    print(f"nuts chain {name}: max position error {err.max():.3e} (after 10 / 20 / 40 transitions {err[9]:.3e} / {err[19]:.3e} / {err[-1]:.3e})")
    assert err.max() < 1e-7
    assert np.max(np.abs(g["logp"].cpu().numpy() - run.logp)) < 1e-7 * scale
    assert np.array_equal(g["nacc"].cpu().numpy(), run.nacc)
    assert np.array_equal(g["counts"], run.counts)
    assert np.all(np.abs(g["a_sum"] - run.a_sum) <= 1e-6 * np.abs(run.a_sum))
    assert np.max(np.abs(g["cont"].cpu().numpy() - run.cont)) < 1e-7
    assert np.array_equal(g["nacc_cont"].cpu().numpy(), run.nacc + run.nacc_cont)
    assert np.array_equal(g["counts_cont"], run.counts + run.counts_cont)            # the sums cover the calls since the last reset
    assert np.all(np.abs(g["a_sum_cont"] - (run.a_sum + run.a_sum_cont)) <= 1e-6 * np.abs(run.a_sum + run.a_sum_cont))
    assert not g["counts_reset"].any() and not g["a_sum_reset"].any()
    assert np.max(np.abs(g["thin"].cpu().numpy() - run.chain[nc.THIN - 1::nc.THIN])) < 1e-7
    assert np.max(np.abs(g["thin_logp"].cpu().numpy() - run.logp[nc.THIN - 1::nc.THIN])) < 1e-7 * scale
    n = nc.CHAIN_STEPS * run.W * run.E
    st = g["stats"]
    assert st["transitions"] == n and st["divergences"] == int(run.counts[:, 2].sum())
    assert st["mean_depth"] == run.counts[:, 1].sum() / n and st["leaves_per_transition"] == run.counts[:, 0].sum() / n
    assert abs(st["mean_accept_stat"] - run.a_sum.sum() / run.counts[:, 0].sum()) < 1e-6
    if len(run.spec) > 1:
        for counts in run.move_counts:
            assert set(counts) == set(range(len(run.spec))), counts


# --------------------------------------------------------------------------------------------------- 5. call splitting
def test_call_splitting_changes_no_bit(monkeypatch):
    """One 40-transition call, 25 + 15 transitions and ALABI_ENS_NUTS_CHUNK=3 give identical bits, stats included; the plan
    reports chunk 3."""
    import torch
    name = "two"
    run = nc.model_chain(name)

    def make():
        return ms.sampler(run.prob, run.W, run.seed, n_ensembles=run.E, moves=nc.moves_objects(run.spec), **hc.sampler_kw(run.ex))
    one = _device_chain(name)
    s = make()
    s.run_mcmc(run.p0, 25, skip_initial_state_check=True)
    s.run_mcmc(None, 15)
    assert torch.equal(s.get_chain_device(), one["chain"]) and torch.equal(s.get_chain_device(log_prob=True), one["logp"])
    assert torch.equal(s._naccept, one["nacc"])
    counts, a_sum = s.nuts_counts()
    assert np.array_equal(counts, one["counts"]) and np.array_equal(a_sum, one["a_sum"])
    assert one["plan"]["chunk"] >= 4
    monkeypatch.setenv("ALABI_ENS_NUTS_CHUNK", "3")
    t = make()
    t.run_mcmc(run.p0, nc.CHAIN_STEPS, skip_initial_state_check=True)
    assert _nuts_plan(t)["chunk"] == 3
    assert torch.equal(t.get_chain_device(), one["chain"]) and torch.equal(t.get_chain_device(log_prob=True), one["logp"])
    assert torch.equal(t._naccept, one["nacc"])
    counts, a_sum = t.nuts_counts()
    assert np.array_equal(counts, one["counts"]) and np.array_equal(a_sum, one["a_sum"])


# ------------------------------------------------------------------------------------------------------- 6. refusals
def test_library_refusals():
    """alabi_ens_set_moves refuses a kind-7 row without a factor, with a step size that is not positive and finite, with max_depth
    outside 1 ... 10 and mixed with kind 6 or kind 0; alabi_ens_set_stream(ens, 0) does not move a NUTS table; alabi_ens_draw,
    alabi_ens_hmc_adapt and the HMC test entry refuse one."""
    import torch
    from alabi_amd import _lib
    from alabi_amd.moves import NUTSMove
    d, W = 3, 6
    prob = ms.problem(d, "ExpSquared")
    s = ms.sampler(prob, W, 5, moves=NUTSMove(0.5, step_size=0.4, max_depth=2))
    s._ensure_ens()
    lib = _lib.lib()
    eye = _lib.host_doubles(np.eye(d).ravel())

    def set_moves(kinds, p0, p1, stage=()):
        for k in stage:
            _lib.check(lib.alabi_ens_set_move_scale(s._ens, k, eye, 1), "alabi_ens_set_move_scale")
        n = len(kinds)
        cum = np.cumsum(np.full(n, 1.0 / n))
        return lib.alabi_ens_set_moves(s._ens, n, (C.c_int * n)(*kinds), _lib.host_doubles(cum), _lib.host_doubles(p0), _lib.host_doubles(p1))
    assert set_moves([7], [0.4], [2.0]) == _lib.BAD_ARG                          # a slot without a factor
    for bad in (0.0, -0.1, np.inf, np.nan):
        assert set_moves([7], [bad], [2.0], stage=(0,)) == _lib.BAD_ARG          # step size
    assert set_moves([7], [0.4], [0.5], stage=(0,)) == _lib.BAD_ARG              # max_depth 0
    assert set_moves([7], [0.4], [11.0], stage=(0,)) == _lib.BAD_ARG             # max_depth 11
    assert set_moves([7, 0], [0.4, 2.0], [2.0, 0.0], stage=(0,)) == _lib.BAD_ARG     # mixed with a stretch move
    assert set_moves([7, 7], [0.4, 0.2], [10.0, 1.0], stage=(0,)) == _lib.BAD_ARG    # the second slot has no factor
    assert set_moves([7, 6], [0.4, 0.4], [2.0, 2.0], stage=(0, 1)) == _lib.BAD_ARG   # mixed with an HMC move (a refusal keeps the factors)
    assert set_moves([7, 7], [0.4, 0.2], [3.0, 1.0], stage=(0, 1)) == _lib.OK
    _lib.check(lib.alabi_ens_set_stream(s._ens, 0), "alabi_ens_set_stream")
    assert lib.alabi_ens_draw(s._ens, 0, 1, 2.0, _lib.current_stream()) == _lib.BAD_ARG
    s.run_mcmc(hc.start(prob, W, 3), 5, skip_initial_state_check=True)
    assert s.last_path == "nuts"
    z = torch.zeros((W, d), dtype=torch.float64, device="cuda"); u = torch.full((W,), 0.5, dtype=torch.float64, device="cuda")
    assert lib.alabi_ens_step_with_randoms_hmc(s._ens, _lib.ptr(s._coords), _lib.ptr(s._logp), 0, 0.3, _lib.ptr(z), _lib.ptr(u), None,
                                               _lib.current_stream()) == _lib.BAD_ARG
    state = torch.zeros((W, 5), dtype=torch.float64, device="cuda")
    assert lib.alabi_ens_hmc_adapt(s._ens, _lib.ptr(s._coords), _lib.ptr(s._logp), 0, 4, 1, _lib.ptr(state),
                                   _lib.host_doubles(np.array([0.8, 0.05, 10.0, 0.75])), None, None, None, None,
                                   _lib.current_stream()) == _lib.BAD_ARG
    dirw = torch.zeros(W, dtype=torch.int32, device="cuda")
    ul = torch.full((W, 7), 0.5, dtype=torch.float64, device="cuda"); ut = torch.full((W, 3), 0.5, dtype=torch.float64, device="cuda")
    args = (_lib.ptr(z), _lib.ptr(dirw), _lib.ptr(ul), _lib.ptr(ut), None, None, _lib.current_stream())
    assert lib.alabi_ens_step_with_randoms_nuts(s._ens, _lib.ptr(s._coords), _lib.ptr(s._logp), 2, 0.3, *args) == _lib.BAD_ARG
    assert lib.alabi_ens_step_with_randoms_nuts(s._ens, _lib.ptr(s._coords), _lib.ptr(s._logp), 0, 0.0, *args) == _lib.BAD_ARG


def test_a_table_beyond_the_lds_is_refused_by_the_run():
    """Five full factors at d = 64 need 5 x 64 x 65 x 8 bytes = 162 KB of LDS: alabi_ens_set_moves takes the table, alabi_ens_run
    is ALABI_BAD_ARGUMENT (there is no other kernel for it).  Three fit with the weights and the checkpoints."""
    from alabi_amd import _lib
    from alabi_amd.moves import NUTSMove
    d = 64
    prob = ms.problem(d, "ExpSquared")
    s = ms.sampler(prob, 2, 5, moves=[NUTSMove(1.0, step_size=0.1, max_depth=1)] * 5)
    with pytest.raises(_lib.AlabiHipError):
        s.run_mcmc(hc.start(prob, 2, 3), 2, skip_initial_state_check=True)
    t = ms.sampler(prob, 2, 5, moves=[NUTSMove(1.0, step_size=0.1, max_depth=1)] * 3)
    t.run_mcmc(hc.start(prob, 2, 3), 2, skip_initial_state_check=True)
    npad = _nuts_plan(t)["lds_bytes"] // 8 - 3 * 64 * 65 - 2 * 10 * 64          # what is left for the weights: the padded N = 130
    assert 130 <= npad <= 256 and npad % 16 == 0 and t.last_path == "nuts"


def test_python_refusals():
    """tune_hmc with a NUTSMove and shard=True raise ValueError; the former names the route."""
    from alabi_amd.moves import NUTSMove
    prob = ms.problem(3, "ExpSquared")
    s = ms.sampler(prob, 4, 5, moves=NUTSMove(0.5, step_size=0.4, max_depth=2))
    with pytest.raises(ValueError, match="tune an HMCMove"):
        s.tune_hmc(hc.start(prob, 4, 3), nwarmup=10)
    with pytest.raises(ValueError, match="shard=True cannot run a NUTSMove"):
        ms.sampler(prob, 4, 5, moves=NUTSMove(0.5), shard=True)


# ------------------------------------------------------------------------------------------------------ 7. run_emcee
def test_run_emcee_with_a_nuts_move(tmp_path):
    """SurrogateModel.run_emcee(sampler_kwargs={"moves": NUTSMove(cov)}) end to end on the 2-D Rosenbrock model of
    tests/test_gpu_hmc_move.py (50 training points), cov from the box widths, 16 walkers, 100 transitions."""
    from alabi_amd import SurrogateModel
    from alabi_amd.benchmarks import rosenbrock
    from alabi_amd.moves import NUTSMove
    sm = SurrogateModel(lnlike_fn=rosenbrock["fn"], bounds=rosenbrock["bounds"], savedir=str(tmp_path), verbose=False, random_state=0)
    sm.init_samples(ntrain=50, ntest=20, sampler="uniform")
    sm.init_gp(kernel="ExpSquaredKernel", fit_amp=True, fit_mean=True, white_noise=-12, hyperopt_method="ml", gp_nopt=1)
    b = np.asarray(rosenbrock["bounds"], dtype=float)
    cov = (0.1 * (b[:, 1] - b[:, 0])) ** 2
    sm.run_emcee(nwalkers=16, nsteps=100, min_ess=0, sampler_kwargs={"moves": NUTSMove(cov, step_size=0.05, max_depth=6)})
    assert sm.emcee_samples.ndim == 2 and sm.emcee_samples.shape[1] == 2 and sm.emcee_samples.shape[0] > 0
    assert sm.emcee_samples_full.shape == (100, 16, 2)
    assert np.all(sm.emcee_samples > b[:, 0]) and np.all(sm.emcee_samples < b[:, 1])
    assert sm.emcee_sampler.last_path == "nuts" and sm.emcee_sampler.last_stream_kernel == "ens_nuts_kernel"
    assert set(sm.nuts_stats) == {"transitions", "mean_depth", "leaves_per_transition", "divergences", "mean_accept_stat"}
    assert sm.nuts_stats["transitions"] == 1600 and 1.0 <= sm.nuts_stats["leaves_per_transition"] <= 63.0
    assert 0.0 < sm.nuts_stats["mean_accept_stat"] <= 1.0 and 0.0 < sm.acc_frac <= 1.0
    with pytest.raises(ValueError, match="tune an HMCMove"):
        sm.run_emcee(nwalkers=16, nsteps=10, min_ess=0, sampler_kwargs={"moves": NUTSMove(cov, step_size=0.05), "hmc_warmup": 20})
