"""Host side of the ensemble sampler's moves (no GPU): alabi_amd.moves.parse_moves, and the CPU statement of emcee's DEMove and
of move mixtures (tests/de_move_numpy.py) that the GPU tests (tests/test_gpu_moves.py) compare the kernels with -- its array
step against the literal emcee step, its batched draws against the single-step ones, and what it samples."""
import numpy as np
import pytest

import de_move_numpy as dm
from de_move_numpy import TWO_MODE_MOVES, mode_share_and_crossings, two_mode_lnprob, two_mode_start
from oracle import stretch_oracle as so


# ------------------------------------------------------------------------------------------------ the statement itself
def test_array_de_step_reproduces_emcee_literal_step_bit_for_bit():
    rng = np.random.RandomState(3)
    W, d = 14, 3
    cov = np.array([1.0, 4.0, 0.25])
    lnp_one = lambda x: -0.5 * float(np.sum(x * x / cov))            # noqa: E731
    lnp_batch = lambda q: -0.5 * np.sum(q * q / cov, axis=1)         # noqa: E731
    coords = rng.normal(size=(W, d))
    logp = lnp_batch(coords)
    n_acc = 0
    for it in range(25):
        rec = {}
        sigma, g0 = ((1e-5, None), (0.3, 1.0))[it % 2]
        c_l, l_l, a_l = dm.emcee_literal_de_step(coords, logp, lnp_one, np.random.RandomState(50 + it), sigma, g0, record=rec)
        order, n0, j1, j2, gamma, u_acc = dm.literal_de_draws_to_arrays(rec)
        assert np.all(j1 != j2)
        c_a, l_a, a_a = dm.de_step_arrays(coords, logp, order, n0, j1, j2, gamma, u_acc, lnp_batch)
        assert np.array_equal(c_l, c_a) and np.array_equal(a_l, a_a)
        assert np.max(np.abs(l_l - l_a)) < 1e-13                     # (the batched sum may round differently from the scalar one)
        n_acc += int(a_l.sum())
        coords, logp = c_l, l_a
    assert 0 < n_acc < 25 * W


def test_nondiagonal_pairs_are_all_ordered_pairs():
    for n in (2, 3, 7):
        p = dm._get_nondiagonal_pairs(n)
        assert p.shape == (n * (n - 1), 2) and np.all(p[:, 0] != p[:, 1])
        assert len({(int(a), int(b)) for a, b in p}) == n * (n - 1)


@pytest.mark.parametrize("W,id0", [(4, 0), (10, 0), (33, 66), (257, 0)])
def test_batched_draws_equal_single_step_statements(W, id0):
    seed = 0xDEADBEEFCAFE1234
    cum = np.cumsum([0.8, 0.2])
    for step0 in (0, 12345678900):
        dr = dm.draw_steps_batched(seed, step0, 3, W, cum, id0)
        for k in range(3):
            order, n0, u_z, partner, u_acc = so.draw_step_randoms(seed, step0 + k, W, id0)
            mi, j1, j2, n, gamma = dm.draw_move_randoms(seed, step0 + k, W, cum, g0=0.7, sigma=0.3, id0=id0)
            assert n0 == dr["n0"] and mi == dr["move"][k]
            assert np.array_equal(order, dr["order"][k]) and np.array_equal(u_z, dr["u_z"][k])
            assert np.array_equal(partner, dr["partner"][k]) and np.array_equal(u_acc, dr["u_acc"][k])
            assert np.array_equal(j1, partner) and np.array_equal(j2, dr["j2"][k]) and np.array_equal(n, dr["n"][k])
            assert np.all(j1 != j2) and np.all(j2 >= 0)
            nc = np.empty(W, dtype=int); nc[order[:n0]] = W - n0; nc[order[n0:]] = n0
            assert np.all(j2 < nc) and np.all(j1 < nc)
            assert np.array_equal(gamma, 0.7 * (1.0 + 0.3 * n))


def test_move_choice_follows_the_weights():
    cum = np.cumsum(np.array([0.5, 0.3, 0.2]))
    dr = dm.draw_steps_batched(9, 0, 4000, 4, cum)
    frac = np.bincount(dr["move"], minlength=3) / 4000.0
    assert np.all(np.abs(frac - [0.5, 0.3, 0.2]) < 4 * np.sqrt(0.25 / 4000))      # four binomial standard deviations at most


# ------------------------------------------------------------------------------------------------------------ parsing
def _make(name, attrs):
    obj = type(name, (), {})()
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def test_parse_moves_forms_and_weight_normalisation():
    from alabi_amd.moves import DEMove, StretchMove, parse_moves
    assert parse_moves(None, 5) is None
    one = parse_moves(DEMove(), 5)
    assert len(one) == 1 and one.has_de and np.array_equal(one.cum, [1.0])
    assert one.p0[0] == 2.38 / np.sqrt(2 * 5) and one.p1[0] == 1e-5              # default gamma0 and sigma
    lst = parse_moves([StretchMove(), DEMove(gamma0=1.0)], 3)
    assert np.array_equal(lst.weights, [0.5, 0.5]) and list(lst.kind) == [0, 1] and list(lst.p0) == [2.0, 1.0]
    mix = parse_moves([(DEMove(), 8.0), (StretchMove(a=3.0), 2.0)], 4)
    w = np.array([8.0, 2.0])
    assert np.array_equal(mix.weights, w / w.sum()) and np.array_equal(mix.cum, np.cumsum(w / w.sum()))
    assert list(mix.kind) == [1, 0] and mix.p0[1] == 3.0 and mix.p0[0] == 2.38 / np.sqrt(8.0)
    assert not parse_moves(StretchMove(), 2).has_de


def test_parse_moves_recognises_foreign_objects_by_name_and_attributes():
    from alabi_amd.moves import DEMove, StretchMove, parse_moves
    ms = parse_moves([(_make("DEMove", dict(sigma=0.01, gamma0=None)), 0.8), (_make("StretchMove", dict(a=2.5)), 0.2)], 2)
    assert isinstance(ms.moves[0], DEMove) and isinstance(ms.moves[1], StretchMove)
    assert ms.p1[0] == 0.01 and ms.p0[0] == 2.38 / np.sqrt(4.0) and ms.p0[1] == 2.5


@pytest.mark.parametrize("name", ["DESnookerMove", "KDEMove", "WalkMove", "GaussianMove", "MHMove"])
def test_parse_moves_refuses_other_moves_by_name(name):
    from alabi_amd.moves import DEMove, parse_moves
    with pytest.raises(NotImplementedError, match=name):
        parse_moves([(DEMove(), 0.9), (_make(name, dict(gammas=1.7)), 0.1)], 3)


def test_parse_moves_bad_weights():
    from alabi_amd.moves import DEMove, StretchMove, parse_moves
    with pytest.raises(ValueError):
        parse_moves([(DEMove(), -1.0), (StretchMove(), 2.0)], 3)
    with pytest.raises(ValueError):
        parse_moves([(DEMove(), 0.0), (StretchMove(), 0.0)], 3)
    with pytest.raises(ValueError):
        parse_moves([], 3)
    with pytest.raises(ValueError):
        parse_moves([DEMove()] * 9, 3)


# --------------------------------------------------------------------------------------------- what the statement samples
def test_de_move_samples_a_gaussian():
    """N(0, diag(1, 4, 0.25)), 24 walkers, 4000 DE steps, 500 discarded.  A RandomState prototype of emcee's DE step gave std
    ratios 0.992-1.017, |mean| / sd <= 0.032 and acceptance 0.316-0.322 over four seeds; this statement with its Philox draws gave
    0.988-1.010, <= 0.019 and 0.317-0.321 over four seeds before the seed was fixed.  The thresholds leave room around that."""
    var = np.array([1.0, 4.0, 0.25])
    lnp = lambda q: -0.5 * np.sum(q * q / var, axis=1)               # noqa: E731
    W = 24
    p0 = np.random.RandomState(1).normal(size=(W, 3)) * np.sqrt(var)
    chain, _, nacc, _, _ = dm.run_ensemble_moves(p0, 4000, lnp, seed=2024, moves=[("de", 1e-5, None, 1.0)])
    flat = chain[500:].reshape(-1, 3)
    ratio = flat.std(axis=0) / np.sqrt(var)
    bias = np.abs(flat.mean(axis=0)) / np.sqrt(var)
    acc = nacc.mean() / 4000.0
    print("std ratio", ratio, "|mean|/sd", bias, "acceptance", acc)
    assert np.all(ratio >= 0.95) and np.all(ratio <= 1.05)
    assert np.all(bias < 0.08)
    assert 0.2 < acc < 0.45


def test_mixture_crosses_between_separated_modes_where_the_stretch_move_does_not():
    """32 walkers, 4 of them started in the + mode, 3000 steps, 500 discarded: the DE mixture equalises the modes (share of
    the + mode in [0.4, 0.6], at least 1000 crossings; a RandomState prototype gave 0.50-0.52 and ~6500 crossings in 6000
    steps), the stretch move stays where it started."""
    p0 = two_mode_start()
    counts = {}
    chain, _, _, _, _ = dm.run_ensemble_moves(p0, 3000, two_mode_lnprob, seed=11, moves=TWO_MODE_MOVES, count_moves=counts)
    share, crossings = mode_share_and_crossings(chain[500:])
    print("DE mixture: share of the + mode", share, "crossings", crossings, "steps per move", counts)
    assert 0.4 <= share <= 0.6
    assert crossings >= 1000
    assert counts.get(1, 0) > 150                                     # both moves of the mixture ran
    chain_s, _, _, _, _ = so.run_ensemble(p0, 1000, two_mode_lnprob, seed=11)
    share_s, crossings_s = mode_share_and_crossings(chain_s[200:])
    print("stretch: share", share_s, "crossings", crossings_s)
    assert crossings_s < 100 and share_s < 0.3


def test_two_mode_settings_of_the_gpu_host_callback_test():
    """The settings tests/test_gpu_moves.py runs through a host like_fn (same target, ensemble, start, seed and box; 1500
    steps, share of the + mode after 300 steps in [0.4, 0.6]), checked on the CPU statement first."""
    bounds = np.array([[-15.0, 15.0]] * 5)

    def lnp(q):
        lp = so.box_lnprior_batch(q, bounds)
        inside = np.isfinite(lp)
        out = np.full(len(q), -np.inf)
        if inside.any():
            out[inside] = two_mode_lnprob(q[inside])
        return out
    chain, _, _, _, _ = dm.run_ensemble_moves(two_mode_start(), 1500, lnp, seed=11, moves=TWO_MODE_MOVES)
    share, crossings = mode_share_and_crossings(chain[300:])
    print("share of the + mode", share, "crossings", crossings)
    assert 0.4 <= share <= 0.6
