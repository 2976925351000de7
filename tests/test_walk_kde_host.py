"""Host side of the walk and KDE moves (no GPU): alabi_amd.moves.WalkMove / KDEMove through parse_moves and MoveSet.resolve, and
the CPU statement tests/walk_kde_numpy.py that the GPU tests (tests/test_gpu_walk_kde.py) compare the kernels with -- pinned to
np.cov and scipy.stats.gaussian_kde, its draws, and what it samples.  The library's ALABI_BAD_ARGUMENT cases need a handle and
are in the GPU file."""
import itertools
import warnings

import numpy as np
import pytest
from scipy.stats import gaussian_kde

import snooker_numpy as sn
import walk_kde_numpy as wk


# ------------------------------------------------------------------------------------------------------------ parsing
def test_parse_walk_and_kde_alone_in_lists_and_in_weighted_pairs():
    from alabi_amd.moves import KIND_KDE, KIND_WALK, DEMove, KDEMove, SnookerMove, WalkMove, parse_moves
    assert (KIND_WALK, KIND_KDE) == (3, 4)
    one = parse_moves(WalkMove(), 5)
    assert list(one.kind) == [3] and one.p0[0] == 0.0 and one.p1[0] == 0.0 and one.has_walk and not one.has_kde
    assert one.multi_partner
    sub = parse_moves(WalkMove(s=3), 5)
    assert list(sub.p0) == [3.0] and "3" in repr(sub.moves[0])
    k = parse_moves(KDEMove(), 5)
    assert list(k.kind) == [4] and k.has_kde and k.multi_partner and np.isnan(k.p0[0]) and np.isnan(k.p1[0])   # W not known yet
    mix = parse_moves([(DEMove(), .5), (WalkMove(), .2), (KDEMove(), .2), (SnookerMove(), .1)], 4)
    assert list(mix.kind) == [1, 3, 4, 2] and np.array_equal(mix.cum, np.cumsum(np.array([.5, .2, .2, .1]) / np.sum([.5, .2, .2, .1])))
    mix.resolve(40)
    assert mix.p0[2] == mix.p1[2] == 20.0 ** (-1.0 / 8.0)
    tab = wk.move_table([("de", 1e-5, None, .5), ("walk", None, .2), ("kde", None, .2), ("snooker", 1.7, .1)], 4, 40)
    for a, b in zip(tab, (mix.kind, mix.cum, mix.p0, mix.p1)):
        assert np.array_equal(a, b)


def test_kde_factors_of_an_odd_ensemble_silverman_scalar_and_callable():
    from alabi_amd.moves import KDEMove, MoveSet, parse_moves
    d, W = 3, 33                                                          # Nc = 16 in split 0, 17 in split 1
    ms = parse_moves(KDEMove(), d).resolve(W)
    assert ms.p0[0] == 16.0 ** (-1.0 / 7.0) and ms.p1[0] == 17.0 ** (-1.0 / 7.0) and ms.p0[0] != ms.p1[0]
    data = np.random.RandomState(0).normal(size=(d, 16))
    assert ms.p0[0] == gaussian_kde(data).factor                         # scipy's own scotts_factor at n = 16
    sil = parse_moves(KDEMove("silverman"), d).resolve(W)
    assert sil.p0[0] == gaussian_kde(data, bw_method="silverman").factor
    assert sil.p1[0] == (17.0 * 5.0 / 4.0) ** (-1.0 / 7.0)
    sc = parse_moves(KDEMove(0.3), d).resolve(W)
    assert sc.p0[0] == sc.p1[0] == 0.3
    assert MoveSet([KDEMove("scott")], [1.0], d, nwalkers=W).p0[0] == ms.p0[0]
    with pytest.raises(NotImplementedError, match="callable"):
        KDEMove(bw_method=lambda kde: 0.5)
    for bad in ("nonsense", 0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            KDEMove(bw_method=bad)
    assert wk.kde_factor("silverman", 17, d) == sil.p1[0] and wk.kde_factor(None, 16, d) == ms.p0[0]


def test_value_errors_of_the_moves_and_of_the_sampler_bounds():
    from alabi_amd.moves import KDEMove, WalkMove, parse_moves
    for bad in (1, 0, -2, 2.5):
        with pytest.raises(ValueError):
            WalkMove(s=bad)
    assert WalkMove(s=4.0).s == 4
    with pytest.raises(ValueError, match="nwalkers // 2"):
        parse_moves(WalkMove(s=6), 2).resolve(11)                         # the smaller half has 5
    parse_moves(WalkMove(s=5), 2).resolve(11)
    with pytest.raises(ValueError, match="nwalkers >= 4"):
        parse_moves(WalkMove(), 1).resolve(3)
    with pytest.raises(ValueError, match="at most"):
        parse_moves(WalkMove(), 1).resolve(4098)
    parse_moves(WalkMove(), 1).resolve(4096)
    with pytest.raises(ValueError, match="2 ndim \\+ 2"):
        parse_moves(KDEMove(), 5).resolve(11)                             # min Nc = 5 < d + 1
    parse_moves(KDEMove(), 5).resolve(12)


def test_foreign_objects_by_name_and_attribute():
    from alabi_amd.moves import KDEMove, WalkMove, parse_moves
    fw = type("WalkMove", (), {})(); fw.s = 4
    fk = type("KDEMove", (), {})(); fk.bw_method = "silverman"
    ms = parse_moves([(fw, 1.0), (fk, 3.0)], 3)
    assert isinstance(ms.moves[0], WalkMove) and ms.moves[0].s == 4
    assert isinstance(ms.moves[1], KDEMove) and ms.moves[1].bw_method == "silverman"
    for name in ("WalkMove", "KDEMove", "MHMove", "GaussianMove", "DESnookerMove"):
        with pytest.raises(NotImplementedError, match=name):
            parse_moves(type(name, (), {})(), 3)                          # without the attribute: refused by name


def test_sampler_refuses_sharding_and_warns_about_few_walkers(monkeypatch):
    """EnsembleSampler's checks run before anything touches the GPU; a stand-in passes the HipGP type check."""
    import alabi_amd.sampler as smp
    from alabi_amd.moves import KDEMove, WalkMove

    class FakeGP:
        ndim = 5
    monkeypatch.setattr(smp, "HipGP", FakeGP)
    monkeypatch.setattr(smp, "_dev", lambda: "cpu")
    monkeypatch.setattr(smp.torch.cuda, "Stream", lambda *a, **k: None)
    mk = lambda W, moves, **kw: smp.EnsembleSampler(W, 5, FakeGP(), None, [[-1, 1]] * 5, seed=1, moves=moves, **kw)   # noqa: E731
    for mv in (WalkMove(), KDEMove()):
        with pytest.raises(ValueError, match="shard=True"):
            mk(64, mv, shard=True)
    with pytest.raises(ValueError, match="nwalkers // 2"):
        mk(12, WalkMove(s=7))
    with pytest.raises(ValueError, match="2 ndim \\+ 2"):
        mk(10, KDEMove(), live_dangerously=True)
    with pytest.warns(RuntimeWarning, match="KDEMove with 6 complementary walkers"):
        s = mk(12, KDEMove())
    assert s._move_set.p0[0] == 6.0 ** (-1.0 / 9.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mk(48, KDEMove())                                                 # 24 = 4 (d + 1): no warning
    s.__dict__["_ens"] = None


# ----------------------------------------------------------------------------------------- the rules against NumPy / SciPy
@pytest.mark.parametrize("s0,d", [(2, 5), (3, 5), (6, 5), (40, 3)])
def test_walk_sum_form_has_the_covariance_of_np_cov(s0, d):
    rows = np.random.RandomState(s0).normal(size=(s0, d)) * np.arange(1, d + 1) + 10.0
    mean = np.zeros(d)
    for m in range(s0):
        mean = mean + rows[m]
    mean = mean / s0
    A = (rows - mean).T / np.sqrt(s0 - 1.0)
    ref = np.atleast_2d(np.cov(rows, rowvar=False))
    assert np.max(np.abs(A @ A.T - ref)) <= 8 * np.finfo(float).eps * np.max(np.abs(ref))
    # walk_proposal is x + A z
    z = np.random.RandomState(1).normal(size=(1, s0))
    q = wk.walk_proposal(np.ones((1, d)), rows[None], z)
    assert np.allclose(q[0], 1.0 + A @ z[0], rtol=0, atol=1e-13 * np.max(np.abs(A)) * s0)


@pytest.mark.parametrize("nc,d,bw", [(6, 5, None), (16, 5, "silverman"), (17, 3, 0.4), (40, 1, None)])
def test_kde_statement_against_gaussian_kde(nc, d, bw):
    """mean / covariance / factor against scipy's, the proposal's scatter L L^T against kde.covariance, and the log factor
    against kde.logpdf(x) - kde.logpdf(q).  Tolerance: the log-sum-exp of nc terms of size O(1) and the condition of L (< 1e3
    here) leave well under 1e-10."""
    rng = np.random.RandomState(nc)
    c = rng.normal(size=(nc, d)) * np.arange(1, d + 1) + 3.0
    kde = gaussian_kde(c.T, bw_method=bw)
    f = wk.kde_factor(bw, nc, d)
    assert abs(f - kde.factor) <= 4 * np.finfo(float).eps * f            # scipy forms neff = 1 / sum(w^2) from weights 1 / n
    mean, L, y, singular = wk.kde_prepare(c, f)
    assert not singular
    assert np.allclose(mean, c.mean(axis=0), rtol=1e-14)
    assert np.allclose(L @ L.T, np.atleast_2d(kde.covariance), rtol=1e-12, atol=1e-14)
    assert np.allclose(L, np.linalg.cholesky(np.atleast_2d(kde.covariance)), rtol=1e-11, atol=1e-14)
    assert np.allclose(L @ y.T, (c - mean).T, rtol=1e-11, atol=1e-12)
    x = rng.normal(size=(9, d)) * np.arange(1, d + 1) + 3.0
    row = rng.randint(0, nc, size=9)
    z = rng.normal(size=(9, d))
    q, lnfac = wk.kde_proposal(x, c, mean, L, y, row, z)
    assert np.allclose(q, c[row] + z @ L.T, rtol=1e-13, atol=1e-13)
    ref = kde.logpdf(x.T) - kde.logpdf(q.T)
    assert np.max(np.abs(lnfac - ref)) < 1e-10 * (1 + np.max(np.abs(ref)))


def test_singular_half_is_reported_not_raised():
    c = np.tile(np.array([[0.3, -0.2, 0.1]]), (8, 1))
    assert wk.kde_prepare(c, 0.5)[3]
    W, d = 16, 3
    coords = np.random.RandomState(1).normal(size=(W, d))
    order = np.arange(W, dtype=np.int32)
    coords[8:] = coords[8]                                                # the complementary set of split 0 is one point
    lnp = lambda q: -0.5 * np.sum(q * q, axis=1)                          # noqa: E731
    sing = []
    out = wk.kde_step_arrays(coords, lnp(coords), order, 8, 0.5, np.zeros(W, dtype=np.int32), np.ones((W, d)), np.full(W, 0.5), lnp,
                             singular_out=sing)
    assert sing == [0] and not out[2][:8].any() and np.array_equal(out[0][:8], coords[:8])
    assert np.all(np.isfinite(out[3][8:]))                                # split 1 ran: its complementary set is alive


# -------------------------------------------------------------------------------------------------------------- draws
def test_new_streams_leave_the_old_draws_alone_and_are_in_range():
    seed, W, d = 0xDEADBEEFCAFE1234, 11, 3
    cum = np.array([1.0])
    for step in (0, 12345678900):
        dr = sn.draw_steps_batched(seed, step, 1, W, cum, 0)
        order, n0 = dr["order"][0], dr["n0"]
        for S, nc in ((order[:n0], W - n0), (order[n0:], n0)):
            sub, z = wk.draw_walk_randoms(seed, step, S, nc, 3)
            assert sub.shape == (len(S), 3) and np.all(np.diff(sub, axis=1) > 0) and sub.min() >= 0 and sub.max() < nc
            full, zf = wk.draw_walk_randoms(seed, step, S, nc, nc)
            assert np.array_equal(full, np.broadcast_to(np.arange(nc), (len(S), nc)))
            assert np.array_equal(z, np.take_along_axis(zf, sub.astype(np.int64), axis=1))      # a row's normal does not depend on s0
            r, zk = wk.draw_kde_randoms(seed, step, S, nc, d)
            assert r.min() >= 0 and r.max() < nc and zk.shape == (len(S), d) and np.all(np.isfinite(zk))


def test_subset_rule_is_uniform_over_subsets():
    """Nc = 5, s0 = 2: ten subsets.  300 steps x 10 walkers = 3000 draws of the model's own streams with a fixed seed, 300 per
    subset expected; chi-square with 9 degrees of freedom, 27.88 is its 0.999 quantile."""
    counts = {}
    for step in range(300):
        sub, _ = wk.draw_walk_randoms(20240607, step, np.arange(10), 5, 2)
        for a, b in sub:
            counts[(int(a), int(b))] = counts.get((int(a), int(b)), 0) + 1
    assert set(counts) == set(itertools.combinations(range(5), 2))
    n = np.array(list(counts.values()), dtype=float)
    chi2 = float(np.sum((n - 300.0) ** 2 / 300.0))
    print("chi2", chi2)
    assert chi2 < 27.88


def test_literal_emcee_forms_run_and_move_walkers():
    lnp1 = lambda v: -0.5 * float(np.sum(v * v))                          # noqa: E731
    p0 = np.random.RandomState(4).normal(size=(16, 3))
    lp = np.array([lnp1(v) for v in p0])
    for step, kw in ((wk.emcee_literal_walk_step, dict(s=None)), (wk.emcee_literal_walk_step, dict(s=3)),
                     (wk.emcee_literal_kde_step, dict(bw_method=None))):
        c, l, acc = step(p0, lp, lnp1, np.random.RandomState(9), **kw)
        assert acc.any() and np.all(np.isfinite(c)) and np.allclose(l, [lnp1(v) for v in c])


# --------------------------------------------------------------------------------------------- what the statement samples


def _pooled_variance(moves, W, seed, **kw):
    lnp = lambda q: -0.5 * np.sum(q * q, axis=1)                          # noqa: E731
    p0 = np.random.RandomState(seed).normal(size=(W, 5))
    sing = []
    chain = wk.run_ensemble_moves(p0, 3000, lnp, seed=2024 + seed, moves=moves, singular_out=sing, **kw)[0]
    return float(chain[600:].reshape(-1, 5).var()), len(sing)


_YARD = {}


def _band(W):
    """The stretch move of the same model, length and seeds: its seed-to-seed range widened by that range's width."""
    if W not in _YARD:
        v = [_pooled_variance([("stretch", 2.0, 1.0)], W, s)[0] for s in (1, 2, 3)]
        lo, hi = min(v), max(v)
        _YARD[W] = (lo - (hi - lo), hi + (hi - lo), v)
    return _YARD[W]


@pytest.mark.parametrize("name,moves,W", [("walk", [("walk", None, 1.0)], 12), ("walk3", [("walk", 3, 1.0)], 12),
                                          ("kde", [("kde", None, 1.0)], 32)])
def test_moves_leave_a_gaussian_invariant(name, moves, W):
    """5-D unit Gaussian, 3000 steps, 600 dropped, seeds 1-3, pooled variance of all coordinates.  Measured:
        stretch, 12 walkers  1.0135 0.9981 1.0223   -> band [0.9738, 1.0465]
        stretch, 32 walkers  0.9944 1.0089 1.0000   -> band [0.9799, 1.0235]
        walk (s=None), 12    1.0132 1.0065 0.9815
        walk (s=3), 12       1.0417 0.9819 1.0068
        KDE (scott), 32      1.0021 1.0039 0.9882
    No half step of the KDE runs was singular."""
    lo, hi, yard = _band(W)
    for seed in (1, 2, 3):
        v, nsing = _pooled_variance(moves, W, seed)
        print(name, "seed", seed, "pooled variance", v, "band", lo, hi, "stretch", yard)
        assert nsing == 0
        assert lo <= v <= hi


def test_kde_without_its_hastings_factor_fails_the_same_check():
    """The log factor forced to 0: the ensemble contracts (measured: pooled variance 0.152, 486 singular half steps)."""
    lo, hi, _ = _band(32)
    v, nsing = _pooled_variance([("kde", None, 1.0)], 32, 1, kde_hastings=False)
    print("KDE without the factor: pooled variance", v, "singular half steps", nsing)
    assert nsing > 0 or not (lo <= v <= hi)


def test_mixture_of_all_five_moves_runs_every_move():
    lnp = lambda q: -0.5 * np.sum(q * q, axis=1)                          # noqa: E731
    moves = [("stretch", 2.0, .2), ("de", 1e-5, None, .2), ("snooker", 1.7, .2), ("walk", 4, .2), ("kde", "silverman", .2)]
    cnt = {}
    p0 = np.random.RandomState(2).normal(size=(17, 3))
    chain, lp, nacc, c, l = wk.run_ensemble_moves(p0, 60, lnp, seed=5, moves=moves, count_moves=cnt, thin_by=3)
    assert set(cnt) == {0, 1, 2, 3, 4} and chain.shape == (20, 17, 3) and np.allclose(l, lnp(c)) and nacc.sum() > 0
    # a set without a new move is the older statement's, bit for bit
    old = [("de", 1e-5, None, .8), ("snooker", 1.7, .2)]
    a = wk.run_ensemble_moves(p0, 40, lnp, seed=5, moves=old)
    b = sn.run_ensemble_moves(p0, 40, lnp, seed=5, moves=old)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
