"""Host tests of the Gaussian Metropolis move and the MHMove (no GPU): parsing and the move table, the sampler's checks, the NumPy
model tests/gaussian_move_numpy.py itself -- its fma, that it samples what it should, no-accept and thinned runs --, the MHMove host
loop against a plain NumPy Metropolis loop, and the honesty of every model run tests/test_gpu_gaussian_move.py compares with."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import gaussian_move_cases as gc
import gaussian_move_numpy as gm
import moves_shapes_common as ms


# --------------------------------------------------------------------------------------------------------------- parsing
def test_cov_forms_modes_and_factor():
    from alabi_amd.moves import KIND_GAUSS, GaussianMove, parse_moves
    d = 3
    full = np.array([[2.0, 0.3, 0.1], [0.3, 1.0, 0.2], [0.1, 0.2, 0.5]])
    m = parse_moves(GaussianMove(0.25), d)
    assert m.kind.tolist() == [KIND_GAUSS] and m.p0.tolist() == [0.0] and m.p1.tolist() == [0.0]
    assert m.has_gauss and m.all_metropolis and not m.multi_partner and not m.all_mh
    (k, C, diag), = m.scales()
    assert k == 0 and diag and np.array_equal(C, 0.5 * np.eye(d))
    for mode, num in (("vector", 0.0), ("random", 1.0), ("sequential", 2.0)):
        m = parse_moves(GaussianMove([1.0, 4.0, 9.0], mode=mode, factor=2.0), d)
        assert m.p0[0] == np.log(2.0) and m.p1[0] == num
        assert np.array_equal(m.scales()[0][1], np.diag([1.0, 2.0, 3.0])) and m.scales()[0][2]
    m = parse_moves(GaussianMove(full), d)
    (_, C, diag), = m.scales()
    assert not diag and np.array_equal(C, np.linalg.cholesky(full)) and np.all(np.triu(C, 1) == 0.0)
    assert np.allclose(C @ C.T, full, rtol=1e-14)
    # the model states the same table
    kinds, cum, p0, p1, scales = gm.move_table([("gauss", full, "vector", None, 1.0), ("gauss", 0.25, "random", 3.0, 3.0)], d, 8)
    mm = parse_moves([(GaussianMove(full), 1.0), (GaussianMove(0.25, mode="random", factor=3.0), 3.0)], d)
    assert np.array_equal(kinds, mm.kind) and np.array_equal(cum, mm.cum) and np.array_equal(p0, mm.p0) and np.array_equal(p1, mm.p1)
    for (C_o, diag_o), (_, C_h, diag_h) in zip(scales, mm.scales()):
        assert np.array_equal(C_o, C_h) and diag_o == diag_h


@pytest.mark.parametrize("cov,kw,match", [
    (0.0, {}, "positive"), (-1.0, {}, "positive"), ([1.0, 0.0, 2.0], {}, "positive"), (np.nan, {}, "finite"),
    ([1.0, np.inf, 1.0], {}, "finite"), (np.ones((2, 3)), {}, "Invalid proposal scale"), (np.ones((2, 2, 2)), {}, "Invalid proposal scale"),
    (np.array([[1.0, 2.0], [2.0, 1.0]]), {}, "not positive definite"), (np.eye(3), {"mode": "random"}, "vector"),
    (np.eye(3), {"mode": "sequential"}, "vector"), (1.0, {"mode": "all"}, "mode"), (1.0, {"factor": 1.0}, "factor"),
    (1.0, {"factor": 0.5}, "factor"), (1.0, {"factor": np.inf}, "factor"), ("abc", {}, "Invalid proposal scale")])
def test_every_value_error_of_the_constructor(cov, kw, match):
    from alabi_amd.moves import GaussianMove
    with pytest.raises(ValueError, match=match):
        GaussianMove(cov, **kw)


def test_dimension_mismatch_is_emcees_error():
    from alabi_amd.moves import GaussianMove, MHMove, parse_moves
    for mv in (GaussianMove([1.0, 2.0]), GaussianMove(np.eye(4)), MHMove(lambda c, r: (c, np.zeros(len(c))), ndim=2)):
        with pytest.raises(ValueError, match="Dimension mismatch in proposal"):
            parse_moves(mv, 3)
    assert parse_moves(GaussianMove(2.0), 7).all_metropolis          # a scalar fits every dimension


def test_foreign_objects_by_their_attributes():
    from alabi_amd.moves import GaussianMove, MHMove, parse_moves
    G = type("GaussianMove", (), {})
    g = G(); g.cov, g.mode, g.factor = [1.0, 4.0], "random", 1.5
    m = parse_moves(g, 2)
    assert isinstance(m.moves[0], GaussianMove) and m.all_metropolis and m.p1[0] == 1.0 and m.p0[0] == np.log(1.5)
    for name in ("GaussianMove", "MHMove"):
        bare = type(name, (), {})()
        with pytest.raises(NotImplementedError, match=name) as ei:
            parse_moves(bare, 2)
        assert "alabi_amd.moves.GaussianMove" in str(ei.value)
    half = G(); half.cov = 1.0                                       # not all three attributes: still refused by name
    with pytest.raises(NotImplementedError, match="GaussianMove"):
        parse_moves(half, 2)
    fn = lambda c, r: (c, np.zeros(len(c)))  # noqa: E731
    for name in ("MHMove", "GaussianMove", "Whatever"):
        obj = type(name, (), {})(); obj.get_proposal = fn
        m = parse_moves(obj, 2)
        assert m.all_mh and isinstance(m.moves[0], MHMove) and m.moves[0].get_proposal is fn and not m.all_metropolis
    notcallable = type("Whatever", (), {})(); notcallable.get_proposal = 3
    with pytest.raises(NotImplementedError, match="Whatever"):
        parse_moves(notcallable, 2)


def test_mixtures_and_the_all_mhmove_rule():
    from alabi_amd.moves import DEMove, GaussianMove, MHMove, StretchMove, parse_moves
    m = parse_moves([(GaussianMove(0.1), 0.5), (StretchMove(), 0.3), (DEMove(), 0.2)], 4)
    assert m.kind.tolist() == [5, 0, 1] and m.has_gauss and not m.all_metropolis and m.multi_partner
    assert [k for k, _, _ in m.scales()] == [0]
    m = parse_moves([GaussianMove(0.1), GaussianMove(np.eye(4))], 4)
    assert m.all_metropolis and not m.multi_partner and [k for k, _, _ in m.scales()] == [0, 1]
    assert not parse_moves(StretchMove(), 4).all_metropolis
    fn = lambda c, r: (c, np.zeros(len(c)))  # noqa: E731
    assert parse_moves([(MHMove(fn), 1.0), (MHMove(fn), 2.0)], 4).all_mh
    for other in (GaussianMove(0.1), StretchMove()):
        with pytest.raises(ValueError, match="MHMove objects only"):
            parse_moves([MHMove(fn), other], 4)
    with pytest.raises(ValueError, match="callable"):
        MHMove(3)


def test_sampler_checks(monkeypatch):
    """EnsembleSampler's argument checks with a stand-in for the GP: one walker is accepted for Metropolis sets only, shard=True
    is refused."""
    import alabi_amd.sampler as smp
    from alabi_amd.moves import GaussianMove, MHMove, StretchMove

    class FakeGP:
        ndim = 5
    monkeypatch.setattr(smp, "HipGP", FakeGP)
    monkeypatch.setattr(smp, "_dev", lambda: "cpu")
    monkeypatch.setattr(smp.torch.cuda, "Stream", lambda *a, **k: None)
    made = []

    def mk(W, moves, **kw):
        s = smp.EnsembleSampler(W, 5, FakeGP(), None, [[-1, 1]] * 5, seed=1, moves=moves, **kw)
        made.append(s)
        return s
    fn = lambda c, r: (c, np.zeros(len(c)))  # noqa: E731
    for mv in (GaussianMove(0.1), [GaussianMove(0.1), GaussianMove(np.eye(5))], MHMove(fn)):
        assert mk(1, mv).nwalkers == 1                                # no "fewer walkers than twice the dimension" for these
        assert mk(3, mv).nwalkers == 3
        with pytest.raises(ValueError, match="shard=True"):
            mk(16, mv, shard=True)
    with pytest.raises(RuntimeError, match="red-blue"):
        mk(4, [GaussianMove(0.1), StretchMove()])                     # a mixture keeps the red-blue rule
    with pytest.raises(RuntimeError, match="red-blue"):
        mk(4, None)
    with pytest.raises(ValueError, match="two walkers"):
        mk(1, None, live_dangerously=True)
    with pytest.raises(ValueError, match="shard=True"):
        mk(16, [GaussianMove(0.1), StretchMove()], shard=True)
    with pytest.raises(ValueError, match="n_ensembles == 1"):
        mk(4, MHMove(fn), n_ensembles=2)
    assert mk(4, GaussianMove(0.1), n_ensembles=3).total_walkers == 12
    with pytest.raises(ValueError, match="Dimension mismatch in proposal"):
        mk(4, GaussianMove(np.eye(4)))
    for s in made:
        s.__dict__["_ens"] = None


# --------------------------------------------------------------------------------------------------------------- the model
def test_fma_is_exact():
    """The emulated fma against exact rational arithmetic, cancellation included."""
    rs = np.random.RandomState(0)
    n = 4000
    a = rs.randn(n) * 10.0 ** rs.uniform(-3, 3, n)
    b = rs.randn(n) * 10.0 ** rs.uniform(-3, 3, n)
    c = -a * b * (1.0 + rs.randn(n) * 10.0 ** rs.uniform(-17, 0, n))
    c[::3] = rs.randn(len(c[::3]))
    c[1::7] = 0.0
    got = gm.fma(a, b, c)
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got, want)
    assert np.any(got != a * b + c)                                  # the cases do tell one rounding from two


def test_proposal_order_and_copied_coordinates():
    rs = np.random.RandomState(3)
    n, d = 6, 4
    x, z = rs.randn(n, d), rs.randn(n, d)
    C = np.tril(rs.randn(d, d)) + 3 * np.eye(d)
    q = gm.gaussian_proposal(x, C, 1.3, np.full(n, -1), z)
    for w in range(n):
        for k in range(d):
            s = Fraction(0)
            sf = 0.0
            for i in range(k + 1):
                sf = float(Fraction(C[k, i]) * Fraction(z[w, i]) + Fraction(sf))
            assert q[w, k] == float(Fraction(1.3) * Fraction(sf) + Fraction(x[w, k]))
            del s
    coord = np.array([0, 3, 1, 2, 2, 0])
    Dg = np.diag(np.diag(C))
    q1 = gm.gaussian_proposal(x, Dg, 1.0, coord, z)
    for w in range(n):
        for k in range(d):
            assert q1[w, k] == (x[w, k] + Dg[k, k] * z[w, k] if k == coord[w] else x[w, k])
    assert np.array_equal(gm.gaussian_proposal(x, Dg, 1.0, coord, z, diagonal=True), q1)


def test_draws_layout():
    """f is one value per (step, ensemble), the coordinate of mode 2 is the absolute step, streams differ, normals are normal."""
    seed, d, W = 5, 7, 400
    gids = np.arange(W) + 1000
    f1, c1, z1 = gm.draw_gauss_randoms(seed, 12, gids, 1000, np.log(2.0), 1, d)
    f2, c2, z2 = gm.draw_gauss_randoms(seed, 12, gids[:5], 1000, np.log(2.0), 1, d)
    assert f1 == f2 and np.array_equal(c1[:5], c2) and np.array_equal(z1[:5], z2)       # keyed by the walker, f by the ensemble
    assert gm.draw_gauss_randoms(seed, 12, gids, 1001, np.log(2.0), 1, d)[0] != f1
    assert 0.5 <= f1 <= 2.0 and gm.draw_gauss_randoms(seed, 12, gids, 1000, 0.0, 0, d)[0] == 1.0
    assert set(np.unique(c1)) == set(range(d))
    assert np.all(gm.draw_gauss_randoms(seed, 7 * 5 + 3, gids, 1000, 0.0, 2, d)[1] == 3)
    assert np.all(gm.draw_gauss_randoms(seed, 12, gids, 1000, 0.0, 0, d)[1] == -1)
    assert abs(z1.mean()) < 5 / np.sqrt(z1.size) and abs(z1.var() - 1.0) < 5 * np.sqrt(2.0 / z1.size)
    assert abs(np.corrcoef(z1[:, 0], z1[:, 1])[0, 1]) < 5 / np.sqrt(W)


TARGET_COV = np.array([[1.0, 0.6, -0.3], [0.6, 2.0, 0.5], [-0.3, 0.5, 0.8]])
TARGET_MEAN = np.array([0.5, -1.0, 2.0])


@pytest.mark.parametrize("moves", [
    (("gauss", 0.5 * TARGET_COV, "vector", None, 1.0),),
    (("gauss", np.array([0.5, 1.0, 0.4]), "vector", 2.0, 1.0),),
    (("gauss", np.array([1.0, 2.0, 0.8]), "random", None, 1.0),),
    (("gauss", np.array([1.0, 2.0, 0.8]), "sequential", None, 1.0),),
], ids=["matrix", "diagonal-factor", "random", "sequential"])
def test_the_statement_samples_the_target(moves):
    """Walkers start as exact draws from a correlated 3-D Gaussian; the move leaves it invariant.  After T steps the W walkers are
    still W INDEPENDENT draws from the target (the chains never interact), so the pooled mean of the final states has standard
    error sqrt(cov_kk / W) and the pooled covariance entry (j, k) has standard error sqrt((cov_jj cov_kk + cov_jk^2) / (W - 1))
    (Wishart); both are asked to agree within 5 standard errors.  A move that did not leave the target invariant -- a missing
    factor, a wrong coordinate rule -- drifts away over the 40 steps: the negative control below shows the test has teeth."""
    W, T, seed = 4000, 40, 21
    Pinv = np.linalg.inv(TARGET_COV)
    lnp = lambda q: -0.5 * np.einsum("ni,ij,nj->n", q - TARGET_MEAN, Pinv, q - TARGET_MEAN)  # noqa: E731
    p0 = np.random.RandomState(seed).multivariate_normal(TARGET_MEAN, TARGET_COV, W)
    chain, lp, nacc, coords, _ = gm.run_ensemble_moves(p0, T, lnp, seed=seed, moves=list(moves), thin_by=T)
    assert 0.15 < nacc.mean() / T < 0.9 and np.array_equal(chain[0], coords)
    assert np.mean(np.any(coords != p0, axis=1)) > 0.99                # the final states are not the start
    se_mean = np.sqrt(np.diag(TARGET_COV) / W)
    assert np.all(np.abs(coords.mean(axis=0) - TARGET_MEAN) < 5 * se_mean)
    se_cov = np.sqrt((np.outer(np.diag(TARGET_COV), np.diag(TARGET_COV)) + TARGET_COV ** 2) / (W - 1))
    assert np.all(np.abs(np.cov(coords, rowvar=False) - TARGET_COV) < 5 * se_cov)


def test_the_sampling_test_has_teeth():
    """The same check fails for a rule that is not a Metropolis rule for the target: accepting against a target twice as wide."""
    W, T, seed = 4000, 40, 21
    Pinv = np.linalg.inv(2.0 * TARGET_COV)
    lnp = lambda q: -0.5 * np.einsum("ni,ij,nj->n", q - TARGET_MEAN, Pinv, q - TARGET_MEAN)  # noqa: E731
    p0 = np.random.RandomState(seed).multivariate_normal(TARGET_MEAN, TARGET_COV, W)
    coords = gm.run_ensemble_moves(p0, T, lnp, seed=seed, moves=[("gauss", 0.5 * TARGET_COV, "vector", None, 1.0)], thin_by=T)[3]
    se_cov = np.sqrt((np.outer(np.diag(TARGET_COV), np.diag(TARGET_COV)) + TARGET_COV ** 2) / (W - 1))
    assert np.any(np.abs(np.cov(coords, rowvar=False) - TARGET_COV) > 5 * se_cov)


def test_no_accept_and_thinned_runs():
    prob = ms.problem(5, "ExpSquared")
    model = ms.BoxModel(prob)
    p0 = gc.start(prob, 7, 3)
    spec = gc.spec_of(5, ("matrix", "vector", 2.0, 0.5), ("vector", "random", None, 0.5))
    never = lambda q: np.full(len(q), -np.inf)  # noqa: E731
    lp0 = model(p0)
    chain, lp, nacc, coords, logp = gm.run_ensemble_moves(p0, 12, never, seed=4, moves=list(spec), logp0=lp0)
    assert np.array_equal(coords, p0) and np.array_equal(logp, lp0) and not nacc.any()
    assert all(np.array_equal(c, p0) for c in chain)
    full = gm.run_ensemble_moves(p0, 30, model, seed=4, moves=list(spec), logp0=lp0)
    thin = gm.run_ensemble_moves(p0, 30, model, seed=4, moves=list(spec), logp0=lp0, thin_by=4)
    assert thin[0].shape[0] == 7 and np.array_equal(thin[0], full[0][3::4]) and np.array_equal(thin[1], full[1][3::4])
    assert np.array_equal(thin[2], full[2]) and full[2].sum() > 0
    # a call split in two with step0 is the one call
    a = gm.run_ensemble_moves(p0, 13, model, seed=4, moves=list(spec), logp0=lp0)
    b = gm.run_ensemble_moves(a[3], 17, model, seed=4, moves=list(spec), logp0=a[4], step0=13)
    assert np.array_equal(np.concatenate([a[0], b[0]]), full[0]) and np.array_equal(a[2] + b[2], full[2])
    # ensembles are told apart by id0 alone
    c = gm.run_ensemble_moves(p0, 30, model, seed=4, moves=list(spec), logp0=lp0, id0=7)
    assert not np.array_equal(c[0], full[0])


def test_a_mixture_calls_every_move():
    run = gc.model_mixture(5)
    assert set(run.counts) == {0, 1, 2} and sum(run.counts.values()) == gc.CHAIN_STEPS


# ---------------------------------------------------------------------------------------------------------- MHMove host loop
def test_mhmove_host_loop_is_a_plain_metropolis_loop(monkeypatch):
    """EnsembleSampler._run_mh with the log-probability replaced by a NumPy function: the chain of a NumPy Metropolis loop driven
    by the same RandomState, for one move and for a weighted pair (the move choice comes from the same generator)."""
    import torch
    import alabi_amd.sampler as smp
    from alabi_amd.moves import MHMove, parse_moves
    d, W, nsteps, seed, thin = 3, 5, 25, 1234, 2
    C1 = np.linalg.cholesky(0.3 * TARGET_COV)
    sig2 = np.array([0.4, 0.2, 0.6])

    def prop_full(coords, rng):
        z = rng.standard_normal(coords.shape)
        return gm.gaussian_proposal(coords, C1, 1.0, np.full(len(coords), -1), z), np.zeros(len(coords))

    def prop_shift(coords, rng):                                       # an asymmetric proposal with its Hastings factor
        step = rng.exponential(sig2, coords.shape)
        return coords + step, -np.sum(step / sig2, axis=1)
    Pinv = np.linalg.inv(TARGET_COV)
    lnp = lambda q: -0.5 * np.einsum("ni,ij,nj->n", q - TARGET_MEAN, Pinv, q - TARGET_MEAN)  # noqa: E731
    p0 = np.random.RandomState(1).multivariate_normal(TARGET_MEAN, TARGET_COV, W)
    for moves in ([MHMove(prop_full, ndim=d)], [(MHMove(prop_full), 0.7), (MHMove(prop_shift), 0.3)]):
        ms_ = parse_moves(moves, d)
        s = SimpleNamespace(_move_set=ms_, nwalkers=W, ndim=d, seed=seed, _mh_rng=None, _coords=torch.as_tensor(p0.copy()),
                            _logp=torch.as_tensor(lnp(p0)), _naccept=torch.zeros(W, dtype=torch.int64),
                            compute_log_prob=lambda c: torch.as_tensor(lnp(c.numpy())))
        monkeypatch.setattr(smp.torch.cuda, "current_stream", lambda: SimpleNamespace(synchronize=lambda: None))
        chain = torch.empty((nsteps // thin, W, d), dtype=torch.float64)
        chain_lp = torch.empty((nsteps // thin, W), dtype=torch.float64)
        smp.EnsembleSampler._run_mh(s, nsteps, thin, chain, chain_lp)
        # the plain loop
        rng = np.random.RandomState(seed)
        x, lp, nacc, rows = p0.copy(), lnp(p0), np.zeros(W, dtype=np.int64), []
        for t in range(nsteps):
            mv = ms_.moves[rng.choice(len(ms_.moves), p=ms_.weights)] if len(ms_.moves) > 1 else ms_.moves[0]
            q, lf = mv.get_proposal(x, rng)
            lq = lnp(q)
            acc = np.log(rng.rand(W)) < lq - lp + lf
            x[acc], lp[acc] = q[acc], lq[acc]
            nacc += acc
            if (t + 1) % thin == 0:
                rows.append(x.copy())
        assert np.array_equal(chain.numpy(), np.array(rows)) and np.array_equal(s._naccept.numpy(), nacc)
        assert np.array_equal(s._coords.numpy(), x) and np.array_equal(chain_lp.numpy()[-1], lnp(np.array(rows)[-1]))
        assert 0 < nacc.sum() < nsteps * W
    # a proposal function that returns the wrong shapes
    bad = parse_moves(MHMove(lambda c, r: (c[:, :2], np.zeros(len(c)))), d)
    s._move_set = bad
    with pytest.raises(ValueError, match="must return"):
        smp.EnsembleSampler._run_mh(s, 2, 1, None, None)


# ------------------------------------------------------------------------------------------------------------ honesty
@pytest.mark.parametrize("name,st", [pytest.param(n, None, id="-".join(str(x) for x in n)) for n in
                                     [("step",) + c for c in gc.STEP_CASES] + [("chain", n) for n in gc.CHAIN_CASES] +
                                     [("ens", e) for e in range(gc.ENS_CASE[3])] + [("extra",) + e for e in gc.EXTRAS] +
                                     [("mix", d) for d in gc.MIX_DIMS]])
def test_model_runs_are_honest(name, st):
    """Every model run the GPU tests compare against: min |margin| > MIN_MARGIN, at least one accept, one in-box reject and one
    out-of-box proposal, and a surrogate term that varies (mu_spread >= MIN_MU_SPREAD)."""
    if name[0] == "step":
        st = gc.model_steps(*name[1:])[4]
    elif name[0] == "chain":
        st = gc.model_chain(name[1]).stats
    elif name[0] == "ens":
        st = gc.model_ensembles()[2][name[1]].stats
    elif name[0] == "extra":
        st = gc.model_extras(*name[1:]).stats
    else:
        st = gc.model_mixture(name[1]).stats
    ms.assert_honest(st, name)


def test_every_gpu_comparison_is_listed_here():
    assert len(list(gc.all_model_runs())) == len(gc.STEP_CASES) + len(gc.CHAIN_CASES) + gc.ENS_CASE[3] + len(gc.EXTRAS) + len(gc.MIX_DIMS)
