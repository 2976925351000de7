"""Host side of the snooker move (no GPU): alabi_amd.moves.SnookerMove through parse_moves, and the CPU statement
tests/snooker_numpy.py that the GPU tests (tests/test_gpu_snooker.py) compare the kernels with -- its draws, what it samples,
and what it does with coincident walkers."""
import itertools

import numpy as np
import pytest

import de_move_numpy as dm
import snooker_numpy as sn


# ------------------------------------------------------------------------------------------------------------ parsing
def test_parse_snooker_alone_in_lists_and_in_weighted_pairs():
    from alabi_amd.moves import KIND_SNOOKER, DEMove, SnookerMove, StretchMove, parse_moves
    assert KIND_SNOOKER == 2
    one = parse_moves(SnookerMove(), 5)
    assert len(one) == 1 and one.has_snooker and not one.has_de and np.array_equal(one.cum, [1.0])
    assert list(one.kind) == [2] and one.p0[0] == 1.7 and one.p1[0] == 0.0          # default gammas
    lst = parse_moves([StretchMove(), SnookerMove(gammas=1.2), DEMove(gamma0=1.0)], 3)
    assert list(lst.kind) == [0, 2, 1] and list(lst.p0) == [2.0, 1.2, 1.0] and lst.has_snooker and lst.has_de
    assert np.array_equal(lst.weights, [1 / 3, 1 / 3, 1 / 3])
    mix = parse_moves([(DEMove(), 0.8), (SnookerMove(), 0.2)], 4)
    assert list(mix.kind) == [1, 2] and np.array_equal(mix.cum, np.cumsum([0.8, 0.2])) and mix.p0[1] == 1.7
    assert isinstance(mix.moves[1], SnookerMove) and "1.7" in repr(mix.moves[1])
    assert not parse_moves([(DEMove(), 0.5), (StretchMove(), 0.5)], 4).has_snooker
    assert np.array_equal(sn.move_table([("de", 1e-5, None, 0.8), ("snooker", 1.7, 0.2)], 4)[0], mix.kind)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_snooker_needs_a_finite_gammas(bad):
    from alabi_amd.moves import SnookerMove
    with pytest.raises(ValueError):
        SnookerMove(gammas=bad)


def test_foreign_desnookermove_is_refused_and_points_to_snookermove():
    from alabi_amd.moves import DEMove, parse_moves
    foreign = type("DESnookerMove", (), {})()
    foreign.gammas = 1.7
    with pytest.raises(NotImplementedError, match="DESnookerMove") as ei:
        parse_moves([(DEMove(), 0.8), (foreign, 0.2)], 3)
    assert "alabi_amd.moves.SnookerMove" in str(ei.value)


# -------------------------------------------------------------------------------------------------------------- draws
@pytest.mark.parametrize("W,id0", [(6, 0), (7, 14), (33, 0)])
def test_three_partners_are_distinct_and_in_range(W, id0):
    seed = 0xDEADBEEFCAFE1234
    cum = np.cumsum([0.8, 0.2])
    for step0 in (0, 12345678900):
        dr = sn.draw_steps_batched(seed, step0, 40, W, cum, id0)
        ref = dm.draw_steps_batched(seed, step0, 40, W, cum, id0)
        for key, val in ref.items():                                     # streams 0-4 are what they were
            assert np.array_equal(dr[key], val), key
        for k in range(40):
            mi, j1, j2, j3 = sn.draw_snooker_randoms(seed, step0 + k, W, cum, id0)
            assert mi == dr["move"][k]
            assert np.array_equal(j1, dr["partner"][k]) and np.array_equal(j2, dr["j2"][k]) and np.array_equal(j3, dr["j3"][k])
            order, n0 = dr["order"][k], dr["n0"]
            nc = np.empty(W, dtype=int); nc[order[:n0]] = W - n0; nc[order[n0:]] = n0
            for j in (j1, j2, j3):
                assert np.all(j >= 0) and np.all(j < nc)
            assert np.all(j1 != j2) and np.all(j1 != j3) and np.all(j2 != j3)


def test_every_ordered_triple_of_four_walkers_occurs():
    """W = 8: both complementary sets hold 4 walkers, 24 ordered triples; 400 steps x 8 walkers = 3200 draws, 133 per triple
    on average (a triple stays empty with probability 24 (23/24)^3200 ~ 1e-58 under uniformity).  Counts within five binomial
    standard deviations of the mean."""
    dr = sn.draw_steps_batched(77, 0, 400, 8, np.array([1.0]))
    trip = np.stack([dr["partner"], dr["j2"], dr["j3"]], axis=-1).reshape(-1, 3)
    keys, counts = np.unique(trip, axis=0, return_counts=True)
    assert {tuple(int(v) for v in k) for k in keys} == set(itertools.permutations(range(4), 3))
    mean = len(trip) / 24.0
    assert np.all(np.abs(counts - mean) < 5 * np.sqrt(mean * (1 - 1 / 24.0)))


# --------------------------------------------------------------------------------------------- what the statement samples
def _pooled_variance(jac):
    lnp = lambda q: -0.5 * np.sum(q * q, axis=1)                          # noqa: E731
    p0 = np.random.RandomState(3).normal(size=(12, 5))
    chain = sn.run_ensemble_moves(p0, 3000, lnp, seed=2024, moves=[("snooker", 1.7, 1.0)], jac=jac)[0]
    return float(chain[600:].reshape(-1, 5).var())


def test_published_log_factor_leaves_a_gaussian_invariant_and_the_others_do_not():
    """The test that defines the move: snooker only, 5-D unit Gaussian, 12 walkers, 3000 steps, 600 dropped, Philox draws.  A
    NumPy-generator prototype gave pooled variances 1.002-1.005 with (d - 1), 0.62-0.63 with 0.5 (d - 1) (the factor recalled
    from emcee 3.1) and 0.30-0.34 with none."""
    v = _pooled_variance(None)
    v_half = _pooled_variance(0.5 * (5 - 1))
    v_none = _pooled_variance(0.0)
    print("pooled variance: published", v, "half", v_half, "none", v_none)
    assert 0.95 <= v <= 1.05
    assert v_half < 0.8 and v_none < 0.8


# ---------------------------------------------------------------------------------------------------- degenerate input
@pytest.mark.parametrize("d", [1, 3])
def test_coincident_walkers_leave_the_walker_in_place(d):
    """s == z: n = 0, e = 0 / 0, q = NaN -- rejected by the comparison itself, nothing NaN is stored."""
    W = 8
    rng = np.random.RandomState(1)
    coords = rng.normal(size=(W, d))
    order = np.arange(W, dtype=np.int32); n0 = 4
    j1 = np.zeros(W, dtype=np.int32); j2 = np.ones(W, dtype=np.int32); j3 = np.full(W, 2, dtype=np.int32)
    coords[0] = coords[4]                                                 # walker 0 (set 0) and its z = C[0] = walker 4 coincide
    lnp = lambda q: -0.5 * np.sum(q * q, axis=1)                          # noqa: E731
    logp = lnp(coords)
    c, lp, acc, lnfac = sn.snooker_step_arrays(coords, logp, order, n0, j1, j2, j3, 1.7, np.full(W, 0.999), lnp)
    assert np.all(np.isfinite(c)) and np.all(np.isfinite(lp))
    assert not acc[0] and np.array_equal(c[0], coords[0]) and lp[0] == logp[0]
    # second half: walker 4's z is C[0] = walker 0, which kept its row, so the two still coincide
    assert not acc[4] and np.array_equal(c[4], coords[4])
    if d == 3:
        assert acc.any()                                                  # the step itself is alive


def test_proposal_on_top_of_z_is_rejected_in_one_dimension():
    """d = 1, s = 0, z = 1.7, z1 = 1, z2 = 0, gamma = 1.7: e = -1, p = -1, q = 1.7 = z exactly, so |q - z| = 0 and the factor is
    0 * (-inf) = NaN: rejected although lnp(q) is finite and u' is tiny."""
    coords = np.array([[0.0], [9.0], [8.0], [1.7], [1.0], [0.0]])
    order = np.arange(6, dtype=np.int32)
    j1 = np.zeros(6, dtype=np.int32); j2 = np.ones(6, dtype=np.int32); j3 = np.full(6, 2, dtype=np.int32)
    lnp = lambda q: -0.5 * np.sum(q * q, axis=1) / 100.0                  # noqa: E731
    logp = lnp(coords)
    c, lp, acc, lnfac = sn.snooker_step_arrays(coords, logp, order, 3, j1, j2, j3, 1.7, np.full(6, 1e-300), lnp)
    assert np.isnan(lnfac[0]) and not acc[0] and c[0, 0] == 0.0 and lp[0] == logp[0]
    assert np.all(np.isfinite(c)) and np.all(np.isfinite(lp))
