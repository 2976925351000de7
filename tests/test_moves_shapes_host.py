"""Host side of tests/test_gpu_moves_shapes.py and tests/test_gpu_moves_chains.py: the optional ``margin_out`` of the NumPy move
models, and the model runs the GPU tests compare against -- none has an accept test within 1e-6 of a tie, each accepts, rejects
inside the box and proposes outside it, and the surrogate varies over its proposals."""
import numpy as np
import pytest

import de_move_numpy as dm
import moves_shapes_common as mc
import snooker_numpy as sn
from oracle import stretch_oracle as so


def _target(q):
    out = -0.5 * np.sum(q ** 2, axis=1)
    out[np.any(np.abs(q) > 2.0, axis=1)] = -np.inf
    return out


@pytest.mark.parametrize("move", ["stretch", "de", "snooker"])
def test_margin_output_is_the_accept_test_and_changes_nothing(move):
    W, d = 12, 3
    dr = mc.injected_draws(W, d, 9, 0)
    coords = np.random.RandomState(1).uniform(-1.5, 1.5, (W, d))
    logp = _target(coords)
    call = {"stretch": lambda **kw: so.stretch_step_arrays(coords, logp, dr.order, dr.n0, dr.u_z, dr.j1, dr.u_acc, _target, 2.0, **kw),
            "de": lambda **kw: dm.de_step_arrays(coords, logp, dr.order, dr.n0, dr.j1, dr.j2, 3.0 * dr.gamma_de, dr.u_acc, _target, **kw),
            "snooker": lambda **kw: sn.snooker_step_arrays(coords, logp, dr.order, dr.n0, dr.j1, dr.j2, dr.j3, 1.7, dr.u_acc, _target, **kw)}[move]
    plain, margins = call(), []
    with_margins = call(margin_out=margins)
    for a, b in zip(plain, with_margins):
        assert np.array_equal(a, b)
    assert [len(m) for m in margins] == [dr.n0, W - dr.n0]
    m = np.empty(W)
    m[dr.order[:dr.n0]], m[dr.order[dr.n0:]] = margins
    assert np.array_equal(m > 0, plain[2])                               # the sign of the margin is the decision
    assert np.any(m == -np.inf) and np.any(m > 0) and np.any((m < 0) & np.isfinite(m))
    # the first half step's margins from their definition
    S = dr.order[:dr.n0]
    lnfac = {"stretch": (d - 1.0) * np.log(((2.0 - 1.0) * dr.u_z[S] + 1.0) ** 2.0 / 2.0), "de": np.zeros(dr.n0)}.get(move)
    if lnfac is None:
        lnfac = plain[3][S]
    moved = plain[2][S]
    assert np.allclose(margins[0][moved], (lnfac + plain[1][S] - logp[S] - np.log(dr.u_acc[S]))[moved], rtol=0, atol=1e-12)


def test_runs_pass_the_margins_through():
    p0 = np.random.RandomState(2).uniform(-1.5, 1.5, (8, 2))
    for run in (lambda **kw: so.run_ensemble(p0, 7, _target, seed=3, **kw),
                lambda **kw: dm.run_ensemble_moves(p0, 7, _target, seed=3, moves=list(mc.DE_STRETCH), **kw),
                lambda **kw: sn.run_ensemble_moves(p0, 7, _target, seed=3, moves=list(mc.ALL_THREE), **kw)):
        margins = []
        a, b = run(), run(margin_out=margins)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert len(margins) == 14 and sum(len(m) for m in margins) == 7 * 8
        assert int(np.sum(np.concatenate(margins) > 0)) == int(a[2].sum())


def test_a_stretch_only_move_set_is_the_stretch_oracle():
    run = mc.model_chain(33, "ExpSquared", 12, mc.STRETCH, "stretch")
    ref = mc.stretch_reference(run)
    assert np.array_equal(ref[0], run.chain) and np.array_equal(ref[1], run.logp) and np.array_equal(ref[2], run.nacc)


def test_every_single_step_model_is_honest():
    assert {d for d, _ in mc.STEP_CASES} == {1, 2, 3, 7, 16, 17, 24, 25, 33, 48, 63, 64} and len(mc.STEP_CASES) == 30
    for d, kernel in mc.STEP_CASES:
        for move in ("stretch", "de", "snooker"):
            mc.assert_honest(mc.model_steps(d, kernel, move)[3], (d, kernel, move))


def test_every_production_model_is_honest():
    runs = [mc.model_chain(d, k, W) for d, k in mc.CHAIN_CASES for W in (12, 13)]
    runs += [mc.model_extras(d, which) for d in (4, 17) for which in ("prior", "nlog", "log", "offset")]
    runs += [mc.model_chain(d, k, 12, mc.ALL_THREE, "host", mc.CHAIN_STEPS, 0) for d, k in ((1, "ExpSquared"), (17, "ExpSquared"), (64, "ExpSquared"), (17, "Matern52"))]
    for run in runs:
        mc.assert_honest(run.stats, (run.p0.shape, run.prob.kernel_name))
        assert len(run.counts) == 3
    for d in (33, 48, 64):
        mc.assert_honest(mc.model_chain(d, "ExpSquared", 12, mc.STRETCH, "stretch").stats, d)
