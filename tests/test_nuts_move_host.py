"""Host tests of the NUTS move: the two statements of the rule in tests/nuts_numpy.py against each other, the sampled
distribution on a Gaussian cut by its box, ``parse_moves`` / ``MoveSet`` / the sampler's refusals for ``NUTSMove``, and the honesty
of every model run the GPU tests compare against.  No GPU, no library."""
import numpy as np
import pytest

import hmc_numpy as hm
import moves_shapes_common as ms
import nuts_cases as nc
import nuts_numpy as nn
from oracle.autocorr_oracle import integrated_time


# ------------------------------------------------------------------------------------- 1. the two forms of the U-turn test
def test_checkpoint_form_equals_aligned_block_form():
    """2000 transitions (max_depth 6, three step sizes) on a 3-D Gaussian in a box that cuts it: the checkpoint form makes the
    same U-turn checks in the same order as the aligned-block form -- every product within 1e-12 of its scale --, and trace,
    next state and acceptance statistic are identical."""
    sd = np.array([1.0, 1.5, 0.7])
    tgt = hm.GaussianTarget(np.zeros(3), np.diag(sd ** 2), np.array([[-1.0, 1.0], [-0.75, 2.25], [-40.0, 40.0]]))
    C = np.diag(sd * 0.9)
    rs = np.random.RandomState(11)
    x = np.array([0.2, 0.3, -0.1])
    lp, g, _ = tgt.value_grad(x[None])
    lp, g = float(lp[0]), g[0]
    depth, reasons, nchecks = 6, set(), 0
    for t in range(2000):
        e = (0.12, 0.35, 0.8)[t % 3]
        z0, dirw = rs.randn(3), int(rs.randint(0, 1 << 30))
        u_leaf, u_tree = rs.rand((1 << depth) - 1), rs.rand(depth)
        ra, rb = {}, {}
        a = nn.transition(tgt, x, lp, g, C, e, z0, dirw, u_leaf, u_tree, depth, form="blocks", rec=ra)
        b = nn.transition(tgt, x, lp, g, C, e, z0, dirw, u_leaf, u_tree, depth, form="checkpoints", rec=rb)
        assert a[3] == b[3] and a[4] == b[4] and np.array_equal(a[0], b[0]) and a[1] == b[1], t
        ua, ub = np.asarray(ra["uturn"]), np.asarray(rb["uturn"])
        assert ua.shape == ub.shape, t
        assert np.all(np.abs(ua[:, 0] - ub[:, 0]) <= 1e-12 * (1.0 + ua[:, 1] / nn.UTURN_EPS)), t
        assert np.array_equal(ua[:, 0] <= 0.0, ub[:, 0] <= 0.0), t
        assert ra["events"] == rb["events"], t
        nchecks += len(ua)
        reasons.add(a[3][2])
        x, lp, g = a[0], a[1], a[2]
    assert reasons >= {nn.STOP_TREE, nn.STOP_SUBTREE} and nchecks > 20000


# ------------------------------------------------------------------------------------------------------- 2. invariance
def _assert_mean_var(chain, mean, var):
    """tests/test_hmc_move_host.py's tolerance: within 5 standard errors, the standard error from the run's own effective sample
    size (sd sqrt(tau / n), tau the integrated autocorrelation time of that very series)."""
    nsteps, W, d = chain.shape
    n = nsteps * W
    flat = chain.reshape(-1, d)
    se = flat.std(axis=0) * np.sqrt(np.maximum(integrated_time(chain), 1.0) / n)
    assert np.all(np.abs(flat.mean(axis=0) - mean) < 5 * se), (flat.mean(axis=0) - mean, se)
    sq = (chain - mean) ** 2
    se2 = sq.reshape(n, d).std(axis=0) * np.sqrt(np.maximum(integrated_time(sq), 1.0) / n)
    assert np.all(np.abs(sq.reshape(n, d).mean(axis=0) - var) < 5 * se2), (sq.reshape(n, d).mean(axis=0) - var, se2)
    return se, se2


def test_the_weights_leave_the_truncated_gaussian_invariant():
    """A 3-D Gaussian cut at -1 / +1 sigma in coordinate 0 and at -0.5 / +1.5 sigma in coordinate 1 (coordinate 2 free), diagonal
    C, e = 0.35, max_depth 6, 8 walkers x 1200 transitions: the orbit ignores the box, a leaf outside it has weight 0, and the
    chain has the truncated moments -- which differ from the untruncated ones by far more than the bound."""
    from scipy.stats import truncnorm
    sd = np.array([1.0, 1.5, 0.7])
    cuts = np.array([[-1.0, 1.0], [-0.5, 1.5], [-50.0, 50.0]])
    tgt = hm.GaussianTarget(np.zeros(3), np.diag(sd ** 2), cuts * sd[:, None])
    t_mean = np.array([truncnorm.mean(a, b) for a, b in cuts]) * sd
    t_var = np.array([truncnorm.var(a, b) for a, b in cuts]) * sd ** 2
    rs = np.random.RandomState(5)
    W, nsteps, depth = 8, 1200, 6
    x = np.stack([truncnorm.rvs(a, b, size=W, random_state=rs) for a, b in cuts], axis=1) * sd
    lp, g, _ = tgt.value_grad(x)
    C = np.diag(sd)
    chain = np.empty((nsteps, W, 3))
    taken = leaves = 0
    for t in range(nsteps):
        x, lp, g, trace, _ = nn.nuts_step_arrays(tgt, x, lp, g, C, 0.35, rs.randn(W, 3), rs.randint(0, 1 << 30, size=W),
                                                 rs.rand(W, (1 << depth) - 1), rs.rand(W, depth), depth)
        chain[t] = x
        taken += trace[:, 3].sum(); leaves += trace[:, 1].sum()
    assert np.all(tgt.inside(chain.reshape(-1, 3)))
    assert taken > 0.8 * nsteps * W and leaves > 4 * nsteps * W
    se, se2 = _assert_mean_var(chain, t_mean, t_var)
    assert abs(sd[0] ** 2 - t_var[0]) > 20 * se2[0] and abs(sd[1] ** 2 - t_var[1]) > 20 * se2[1]   # the test can tell the two apart


# ----------------------------------------------------------------------------------- 3. the model runs the GPU tests use
_RUNS = list(nc.all_model_runs())


@pytest.mark.parametrize("name,rec", _RUNS, ids=lambda v: "-".join(str(x) for x in v).replace(" ", "") if isinstance(v, tuple) else "")
def test_every_model_run_is_honest(name, rec):
    """Conditions on the model alone: every leaf and tree comparison |ln u - threshold| > ms.MIN_MARGIN; every U-turn product
    |rho . z| > 100 x 1e-7 x (|rho|_1 + m |z|_1), m the number of points in rho (each momentum may be off by the project's 1e-7,
    100 is its margin factor); every leaf coordinate farther than 1e-5 from a wall; every delta at least 1 from -1000."""
    h = nn.honesty(rec, ms.MIN_MARGIN)
    assert h["ok"], (name, h)


def test_the_case_set_covers_every_outcome():
    """Over the case set: each stop reason, a kept subtree with an out-of-box leaf, a transition that stays at its start, a depth
    of at least 3, both directions."""
    events = set()
    for _, rec in _RUNS:
        events.update(rec["events"])
    assert {("stop", r) for r in (nn.STOP_DEPTH, nn.STOP_TREE, nn.STOP_SUBTREE, nn.STOP_DIVERGENT)} <= events
    assert {"kept_subtree_with_out_of_box_leaf", "stays", "forward", "backward"} <= events
    assert max(ev[1] for ev in events if isinstance(ev, tuple) and ev[0] == "depth") >= 3
    # every case alone goes both ways and compares at least one leaf and one tree uniform
    for name, rec in _RUNS:
        assert {"forward", "backward"} <= set(rec["events"]) and len(rec["cmp"]) > 10, name


def test_the_divergent_case_diverges():
    """A normal prior of standard deviation 0.02 on coordinate 0 and e = 0.06 with C = I: e sqrt(1 / 0.02^2) = 3 > 2, the leapfrog
    map is unstable there, and delta falls below -1001 within a few leaves."""
    run = nc.model_steps("divergent")
    assert nc.DIVERGENT_STEP * np.sqrt(1.0 / 0.02 ** 2) > 2.0 and run.e == nc.DIVERGENT_STEP
    assert np.all(np.diag(hm.gm.scale_factor(run.cov, 3)[0]) == 1.0)
    traces = np.concatenate([tr for _, _, _, tr, _ in run.steps])
    div = traces[:, 2] == nn.STOP_DIVERGENT
    assert div.sum() >= 5 and (~div).sum() >= 5
    assert np.all(traces[div, 1] <= 8)                             # within a few leaves
    delta = np.asarray(run.rec["delta"])
    low = delta[~(delta > nn.DIVERGENT_BELOW)]
    assert len(low) == div.sum() and np.all(low < -1001.0)
    assert nn.STOP_DIVERGENT not in {tr[2] for name in nc.GRID for _, _, _, trs, _ in nc.model_steps(name).steps for tr in trs}


def test_the_mixture_chooses_both_moves_and_the_ensembles_differ():
    two = nc.model_chain("two")
    assert all(set(c) == {0, 1} for c in two.move_counts)
    assert len({tuple(np.round(r, 12)) for r in two.chain[-1].reshape(3, -1)}) == 3


# --------------------------------------------------------------------------------------------- 4. NUTSMove and parse_moves
def test_nuts_move_validation():
    from alabi_amd.moves import NUTS_MAX_DEPTH, NUTSMove
    m = NUTSMove([0.5, 2.0], step_size=0.3, max_depth=5, jitter=1.5)
    assert m.max_depth == 5 and m.diagonal and m.resolved_step_size(2) == 0.3 and m.ln_jitter == hm.ln_jitter(1.5)
    assert np.array_equal(m.scale_matrix(2), np.diag(np.sqrt([0.5, 2.0])))
    assert NUTSMove(0.5).max_depth == 8 and NUTSMove(0.5).resolved_step_size(16) == 0.5 and NUTS_MAX_DEPTH == 10
    assert not NUTSMove(np.array([[1.0, 0.2], [0.2, 1.0]])).diagonal
    for bad in (0, 11, 2.5, True):
        with pytest.raises(ValueError, match="max_depth"):
            NUTSMove(0.5, max_depth=bad)
    for kw in (dict(step_size=0.0), dict(step_size=np.inf), dict(jitter=1.0), dict(jitter=np.nan)):
        with pytest.raises(ValueError, match="NUTSMove"):
            NUTSMove(0.5, **kw)
    for cov in (-1.0, [1.0, 0.0], np.array([[1.0, 2.0], [2.0, 1.0]]), np.zeros((2, 3)), np.nan):
        with pytest.raises(ValueError):
            NUTSMove(cov)
    assert "max_depth=5" in repr(m)


def test_parse_moves_nuts_rows_and_mixtures():
    from alabi_amd.moves import KIND_NUTS, GaussianMove, HMCMove, NUTSMove, StretchMove, parse_moves
    s = parse_moves([(NUTSMove(0.5, step_size=0.4, max_depth=3, jitter=1.5), 1.0), (NUTSMove([1.0, 2.0, 3.0]), 3.0)], 3)
    assert s.all_nuts and s.has_nuts and not s.has_hmc and not s.all_hmc and not s.all_metropolis
    assert list(s.kind) == [KIND_NUTS, KIND_NUTS] and np.allclose(s.cum, [0.25, 1.0])
    assert s.p0[0] == 0.4 and s.p0[1] == 3.0 ** -0.25
    assert s.p1[0] == 3.0 + hm.ln_jitter(1.5) / 512.0 and s.p1[1] == 8.0
    assert [k for k, _, _ in s.scales()] == [0, 1]
    _, cum, p0, p1, _ = nn.move_table([(0.5, 0.4, 3, 1.5, 1.0), (np.array([1.0, 2.0, 3.0]), None, 8, None, 3.0)], 3)
    assert np.array_equal(cum, s.cum) and np.array_equal(p0, s.p0) and np.array_equal(p1, s.p1)
    for other in (StretchMove(), GaussianMove(0.1), HMCMove(0.5)):
        with pytest.raises(ValueError):
            parse_moves([(other, 0.5), (NUTSMove(0.5), 0.5)], 3)
    with pytest.raises(ValueError, match="a move set that holds a NUTSMove must consist of NUTSMove objects only"):
        parse_moves([StretchMove(), NUTSMove(0.5)], 3)
    with pytest.raises(ValueError, match="Dimension mismatch"):
        parse_moves(NUTSMove([1.0, 2.0]), 3)
    assert not parse_moves(HMCMove(0.5), 3).has_nuts


class _FakeGP:
    ndim = 4


def test_sampler_refusals(monkeypatch):
    """Host callables, shard=True and tune_hmc are refused with a ValueError; tune_hmc's names the route; any nwalkers >= 1."""
    import alabi_amd.sampler as sa
    from alabi_amd.moves import NUTSMove
    monkeypatch.setattr(sa, "HipGP", _FakeGP)
    monkeypatch.setattr(sa.torch, "zeros", lambda *a, **k: None)
    monkeypatch.setattr(sa.torch.cuda, "Stream", lambda *a, **k: None)
    monkeypatch.setattr(sa, "_dev", lambda: "cpu")
    monkeypatch.setattr(sa.EnsembleSampler, "__del__", lambda self: None)
    b = np.array([[-1.0, 1.0]] * 4)
    with pytest.raises(ValueError, match="gradient"):
        sa.EnsembleSampler(8, 4, _FakeGP(), None, b, moves=NUTSMove(0.5), prior_fn=lambda q: np.zeros(len(q)))
    with pytest.raises(ValueError, match="shard=True cannot run a NUTSMove"):
        sa.EnsembleSampler(8, 4, _FakeGP(), None, b, moves=NUTSMove(0.5), shard=True)
    for W in (1, 3, 40):
        s = sa.EnsembleSampler(W, 4, _FakeGP(), None, b, moves=[(NUTSMove(0.5), 1.0), (NUTSMove(0.2, max_depth=2), 2.0)], seed=1)
        assert s._move_set.all_nuts and s.__getstate__()["_move_set"].all_nuts
        with pytest.raises(ValueError, match=r'tune an HMCMove.*NUTSMove\(sm.hmc_tuning\["cov"\], step_size=sm.hmc_tuning\["step_size"\]\)'):
            s.tune_hmc(np.zeros((W, 4)))
