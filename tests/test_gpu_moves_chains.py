"""Production runs of the launch-per-half-step ensemble kernels at the dimension buckets and kernel families no other sampler test
reaches (d up to 64; Matern and rational-quadratic surrogates), step for step against tests/snooker_numpy.py and
oracle/stretch_oracle.py: the stretch + DE + snooker mixture, the stretch move alone above d = 30, the moves under the fused extras
(normal prior, affine and non-affine log-probability maps, inputs far from the origin), the host-callback path against the fused
one, and the multi-proposal kernels at the buckets where NP changes.  Single steps and the degenerate snooker geometries are in
tests/test_gpu_moves_shapes.py; problems, model runs and what makes a comparison honest in tests/moves_shapes_common.py.

Tolerances are those of the tests these shapes extend (tests/test_gpu_snooker.py, tests/test_gpu_ensemble.py,
tests/test_gpu_generic_lnprob.py): chains and log-probabilities to 1e-7, acceptance counts identical."""
import numpy as np
import pytest

import moves_shapes_common as mc

pytestmark = pytest.mark.gpu

FUSED, HOST = "launch-per-half-step", "host-callback"


@pytest.fixture(autouse=True)
def half_step_path(monkeypatch):
    monkeypatch.setenv("ALABI_ENS_STREAM", "0")
    monkeypatch.setenv("ALABI_ENS_GROUP", "0")
    monkeypatch.delenv("ALABI_ENS_MULTI", raising=False)


def _honest(run, what, nmoves=None):
    print(what, run.stats, run.counts)
    mc.assert_honest(run.stats, what)
    if nmoves:
        assert len(run.counts) == nmoves and min(run.counts.values()) >= 1          # every move of the set was taken


def _run(run, spec, path=FUSED, **kw):
    """The model run's start, seed and length on the device."""
    W, d = run.p0.shape
    s = mc.sampler(run.prob, W, run.seed, moves=None if spec is None else mc.moves_objects(spec), **kw)
    s.run_mcmc(run.p0, len(run.chain), skip_initial_state_check=W <= d)
    assert s.last_path == path
    return s


@pytest.mark.parametrize("thin", [1, 3])
@pytest.mark.parametrize("W", [12, 13])
@pytest.mark.parametrize("d,kernel", mc.CHAIN_CASES, ids=[f"d{d}-{k}" for d, k in mc.CHAIN_CASES])
def test_three_move_production_chain(d, kernel, W, thin):
    """Counter-based draws + kernel sequence == snooker_numpy.run_ensemble_moves, 60 steps and a continuation of 10."""
    run = mc.model_chain(d, kernel, W)
    _honest(run, f"chain d={d} {kernel} W={W}", 3)
    s = mc.sampler(run.prob, W, run.seed, moves=mc.moves_objects(mc.ALL_THREE))
    s.run_mcmc(run.p0, mc.CHAIN_STEPS, thin_by=thin, skip_initial_state_check=W <= d)
    assert s.last_path == FUSED
    chain_o, lp_o = run.chain[thin - 1::thin], run.logp[thin - 1::thin]
    chain = s.get_chain()
    assert chain.shape == chain_o.shape
    print("max chain diff", np.max(np.abs(chain - chain_o)), "max logp diff", np.max(np.abs(s.get_log_prob() - lp_o)))
    assert np.max(np.abs(chain - chain_o)) < 1e-7
    assert np.max(np.abs(s.get_log_prob() - lp_o)) < 1e-7
    assert np.array_equal(s._naccept.cpu().numpy(), run.nacc)
    s.run_mcmc(None, mc.CONT_STEPS, thin_by=thin)                                    # continues the counter
    cont = run.cont[thin - 1::thin]
    assert s.last_path == FUSED and np.max(np.abs(s.get_chain()[-len(cont):] - cont)) < 1e-7


@pytest.mark.parametrize("d", [33, 48, 64])
def test_stretch_alone_above_thirty_dimensions(d):
    """moves=None beyond the persistent kernels' buckets: ens_half_kernel<48> and <64> against stretch_oracle.run_ensemble."""
    run = mc.model_chain(d, "ExpSquared", 12, mc.STRETCH, "stretch")
    _honest(run, f"stretch d={d}")
    chain_o, lp_o, nacc_o, _, _ = mc.stretch_reference(run)
    assert np.array_equal(chain_o, run.chain)
    s = _run(run, None)
    assert np.max(np.abs(s.get_chain() - chain_o)) < 1e-7
    assert np.max(np.abs(s.get_log_prob() - lp_o)) < 1e-7
    assert np.array_equal(s._naccept.cpu().numpy(), nacc_o)
    s.run_mcmc(None, mc.CONT_STEPS)
    assert s.last_path == FUSED and np.max(np.abs(s.get_chain()[-mc.CONT_STEPS:] - run.cont)) < 1e-7


# ---- the fused extras under the three-move set
@pytest.mark.parametrize("d", [4, 17])
def test_moves_under_normal_prior_and_logp_affine(d):
    """normal_prior_sum (lanes 0, 2 and, at d = 17, lane 16) and logp_affine, as tests/test_gpu_ensemble.py has them for the stretch move."""
    run = mc.model_extras(d, "prior")
    _honest(run, f"prior d={d}", 3)
    s = _run(run, mc.ALL_THREE, logp_affine=mc.AFFINE, normal_prior=mc.normal_prior(d))
    assert np.max(np.abs(s.get_chain() - run.chain)) < 1e-7
    assert np.max(np.abs(s.get_log_prob() - run.logp)) < 1e-7 * (np.max(np.abs(run.logp)) + 1)
    assert np.array_equal(s._naccept.cpu().numpy(), run.nacc)


@pytest.mark.parametrize("kind", ["nlog", "log"])
@pytest.mark.parametrize("d", [4, 17])
def test_moves_under_nonaffine_y_map(d, kind):
    """apply_ymap inside the half-step kernels, as tests/test_gpu_generic_lnprob.py::test_nonaffine_y_scaler_fused."""
    run = mc.model_extras(d, kind)
    _honest(run, f"{kind} d={d}", 3)
    s = _run(run, mc.ALL_THREE, logp_map=kind)
    assert np.max(np.abs(s.get_chain() - run.chain)) <= 1e-7
    assert np.max(np.abs(s.get_log_prob() - run.logp) / (np.abs(run.logp) + 1)) <= 1e-9
    assert np.array_equal(s._naccept.cpu().numpy(), run.nacc)


@pytest.mark.parametrize("d", [4, 17])
def test_moves_with_inputs_far_from_origin(d):
    """Inputs thousands of length scales from the origin (se_pair_terms' centring, the snooker sums of differences): the chain
    tolerance scales with the offset as in tests/test_gpu_ensemble.py::test_half_step_kernels_inputs_far_from_origin."""
    run = mc.model_extras(d, "offset")
    _honest(run, f"offset d={d}", 3)
    s = _run(run, mc.ALL_THREE)
    assert np.max(np.abs(s.get_chain() - run.chain)) <= 1e-7 * np.max(np.abs(run.prob.off))
    assert np.max(np.abs(s.get_log_prob() - run.logp) / (np.abs(run.logp) + 1)) <= 1e-8
    assert np.array_equal(s._naccept.cpu().numpy(), run.nacc)


@pytest.mark.parametrize("d,kernel", [(1, "ExpSquared"), (17, "ExpSquared"), (64, "ExpSquared"), (17, "Matern52")])
def test_host_callback_equals_fused(d, kernel):
    """A host prior_fn equal to the box, gate_box=False: the propose kernels (all three instantiations) -> host -> accept kernel give
    the chain of the fused kernels."""
    from oracle.stretch_oracle import box_lnprior_batch
    run = mc.model_chain(d, kernel, 12, mc.ALL_THREE, "host", mc.CHAIN_STEPS, 0)
    _honest(run, f"host d={d} {kernel}", 3)
    bounds = run.prob.bounds
    fused = _run(run, mc.ALL_THREE)
    host = _run(run, mc.ALL_THREE, HOST, prior_fn=lambda q: box_lnprior_batch(q, bounds), gate_box=False)
    assert np.max(np.abs(host.get_chain() - fused.get_chain())) < 1e-7
    assert np.array_equal(host._naccept.cpu().numpy(), fused._naccept.cpu().numpy())
    assert np.array_equal(fused._naccept.cpu().numpy(), run.nacc)


# ---- the multi-proposal kernels where NP changes: 4 up to bucket 16, 2 up to bucket 24, 1 beyond
MULTI_CASES = [(d, "ExpSquared") for d in (1, 8, 16, 17, 24, 25)] + [(8, "Matern52"), (24, "Matern52")]


@pytest.mark.parametrize("spec", [mc.STRETCH, mc.DE_STRETCH], ids=["stretch", "de+stretch"])
@pytest.mark.parametrize("d,kernel", MULTI_CASES, ids=[f"d{d}-{k}" for d, k in MULTI_CASES])
def test_multi_proposal_kernels_bit_identical(d, kernel, spec, monkeypatch):
    """ALABI_ENS_MULTI = 2 and 4 against 1: W = 14, E = 3, so a half step has 7 proposals per ensemble and the last workgroup of
    ens_half_multi_kernel / ens_half_multi_de_kernel is ragged for NP = 2 and 4.  Where the bucket has no such instantiation (4 above
    bucket 16, 2 above bucket 24) the library falls back; the bits are the same either way."""
    W, E, nsteps = 14, 3, 30
    p0, seed, run = mc.model_multi(d, kernel, spec)
    _honest(run, f"multi d={d} {kernel}", len(spec))
    moves = None if spec is mc.STRETCH else mc.moves_objects(spec)
    out = {}
    for multi in ("1", "2", "4"):
        monkeypatch.setenv("ALABI_ENS_MULTI", multi)
        s = mc.sampler(run.prob, W, seed, n_ensembles=E, moves=moves)
        s.run_mcmc(p0, nsteps, skip_initial_state_check=W <= d)
        assert s.last_path == FUSED
        out[multi] = (s.get_chain(), s.get_log_prob(), s._naccept.cpu().numpy().copy())
    for multi in ("2", "4"):
        for a, b in zip(out["1"], out[multi]):
            np.testing.assert_array_equal(a, b)
    # ensemble 0 is the model's run
    assert np.max(np.abs(out["1"][0][:, :W] - run.chain)) < 1e-7
    assert np.array_equal(out["1"][2][:W], run.nacc)
