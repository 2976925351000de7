"""CPU checks of the NUTS warm-up: the NumPy statement (tests/nuts_adapt_numpy.py) against tests/nuts_numpy.py and closed forms, the
honesty of every model run that tests/test_gpu_nuts_adapt.py compares the device with, the whole warm-up on two problems, and what
of ``tune_nuts`` / ``find_step_size`` / ``run_emcee``'s keys / ``searched_state`` / the ABI needs no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import hmc_adapt_numpy as han
import hmc_cases as hc
import hmc_numpy as hm
import moves_shapes_common as ms
import nuts_adapt_cases as nac
import nuts_adapt_numpy as nan_
import nuts_cases as nc
import nuts_numpy as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN08 = float(np.log(0.8))


# ---------------------------------------------------------------------------------------------------- 1. the transition
def _frozen(eps, n):
    state = np.zeros((n, 5))
    state[:, nan_.LN_E] = state[:, nan_.MU] = np.log(eps)
    return state


FROZEN_PAR = (0.8, np.inf, 10.0, 0.75)       # gamma = inf: ln e stays at mu


@pytest.mark.parametrize("name", ["d5m52", "ens3", "divergent"])
def test_a_frozen_state_is_nuts_numpys_transition(name):
    """With gamma = inf and mu = ln e the model's warm-up run is nuts_numpy.run_nuts at the step size e, bit for bit."""
    r = nac.model_run(name)
    tgt = hc.target_of(r.prob, r.ex)
    p0, lp0 = r.p0[:r.W], r.logp0[:r.W]                             # the first ensemble (run_nuts runs one)
    a = nan_.run_nuts_adapt(tgt, p0, 12, r.seed, r.move, FROZEN_PAR, _frozen(r.move[1], r.W), logp0=lp0)
    chain, lp, nacc, c_end, lp_end, counts, a_sum = nn.run_nuts(tgt, p0, 12, r.seed, [r.move], logp0=lp0)
    assert np.array_equal(a.chain, chain) and np.array_equal(a.chain_logp, lp) and np.array_equal(a.nacc, nacc)
    assert np.array_equal(a.counts, counts) and np.all(a.state[:, nan_.LN_E] == np.log(r.move[1])) and np.all(a.state[:, nan_.M] == 12)
    assert np.max(np.abs(a.a_sum - a_sum)) < 1e-12 and np.all((a.alpha >= 0) & (a.alpha <= 1))
    if name == "divergent":
        assert a.counts[:, 2].sum() > 0


@pytest.mark.parametrize("eps,sd0", [(0.9, 1.0), (0.06, 0.02)])
def test_a_t_is_the_mean_of_the_leaves_statistics(eps, sd0):
    """On a Gaussian in a box no leaf leaves, every a_t is the mean of min(1, exp(delta)) over the transition's recorded deltas, 0
    for a divergent leaf, which counts as a leaf.  The second target is nuts_cases' divergent construction: coordinate 0 has the
    standard deviation 0.02, so e = 0.06 is beyond the leapfrog map's stability bound 2 x 0.02 along it and trees diverge."""
    d, W, seed, depth = 3, 5, 77, 5
    sd = np.array([sd0, 1.0, 1.0])
    tgt = hm.GaussianTarget(np.zeros(d), np.diag(sd ** 2), np.stack([np.full(d, -1e200), np.full(d, 1e200)], axis=1))
    move = (1.0, eps, depth, None, 1.0)
    p0 = np.random.RandomState(seed).randn(W, d) * sd
    a = nan_.run_nuts_adapt(tgt, p0, 12, seed, move, FROZEN_PAR, _frozen(eps, W))
    coords, logp, grad = p0, han.gated(tgt, p0), tgt.value_grad(p0)[1]
    _, cum, tp0, tp1, scales = nn.move_table([move], d)
    some_zero = False
    for t in range(12):
        _, e, z0, dirw, u_leaf, u_tree = nn.draw_nuts_randoms(seed, t, np.arange(W), 0, cum, tp0, tp1, d)
        new = [None] * W
        for w in range(W):
            rec = {}
            new[w] = nn.transition(tgt, coords[w], float(logp[w]), grad[w], scales[0][0], e, z0[w], dirw[w], u_leaf[w], u_tree[w], depth, rec=rec)
            delta = np.asarray(rec["delta"])
            with np.errstate(all="ignore"):
                leaf_a = np.where(delta > nn.DIVERGENT_BELOW, np.minimum(1.0, np.exp(delta)), 0.0)
            assert len(delta) == new[w][3][1] >= 1 and abs(a.alpha[t, w] - np.sum(leaf_a) / len(delta)) < 1e-15
            some_zero |= bool(np.any(leaf_a == 0.0)) and bool(np.any(leaf_a > 0.0))
        coords, logp, grad = np.array([n[0] for n in new]), np.array([n[1] for n in new]), np.array([n[2] for n in new])
        assert np.array_equal(coords, a.chain[t])
    assert some_zero == (sd0 < 1)
    assert (a.counts[:, 2].sum() > 0) == (sd0 < 1)


def test_the_update_is_hmc_adapt_numpys():
    assert nan_.da_update is han.da_update


# ------------------------------------------------------------------------------------------------------------ 2. honesty
@pytest.mark.parametrize("key,rec", list(nac.all_model_runs()), ids=lambda v: "-".join(v) if isinstance(v, tuple) else "")
def test_every_model_run_is_honest(key, rec):
    """No tree decision near a tie, no U-turn product near zero, no leaf at a wall, no energy error near the divergence bound, and
    every comparison of the search further than MIN_MARGIN from ln 0.8."""
    h = nan_.honesty(rec, ms.MIN_MARGIN)
    assert h["ok"], (key, h)


def test_the_seed_rule():
    """Every case's seed is one of 100 + d, 200 + d, ... and no earlier one was skipped for honesty: find_seed's outcome is the
    default seed.  The one listed seed moved on by the GPU test's cap, one step (NOTES.md "NUTS warm-up")."""
    assert nac.SEEDS == {"d5m52": 205}
    for name in ("d1", "w1", "d5m52", "divergent"):
        assert nac.find_seed(name) == 100 + nac.CASES[name][0]
    for name in nac.CASES:
        assert nac.case_seed(name) % 100 == nac.CASES[name][0] % 100


def test_the_cases_cover_what_they_are_there_for():
    dv = nac.model_run("divergent").run
    assert dv.counts[:, 2].sum() >= 10 and dv.counts[:, 2].sum() == dv.diverged.sum()
    assert np.sum(dv.diverged & (dv.alpha > 0) & (dv.alpha < 1)) >= 5          # a_t with a zero leaf beside leaves with a > 0
    assert np.all(nac.model_run("d10").run.diverged.sum(axis=0) == nac.model_run("d10").run.counts[:, 2])
    for name in nac.CASES:
        a = nac.model_run(name).run.alpha
        assert np.any((a > 0) & (a < 1)) and np.all((a >= 0) & (a <= 1)), name
    assert nac.model_run("ens3").E == 3 and nac.case_problem("tiled").N == 520 and nac.model_run("w1").W == 1
    dirs = np.sign(np.round((nac.model_search("d5m52").ln_e - nac.model_search("d5m52").case.ln_e) / nan_.LN2))
    assert set(dirs) == {-1.0, 1.0}                                   # both directions in one launch
    assert np.all(nac.model_search("cap").iters == nan_.SEARCH_CAP) and nac.model_search("hmc").case.table == "hmc"


# ------------------------------------------------------------------------------------------------------------- 3. search
class _StdGaussian:
    """lnp = -|q|^2 / 2 in a wide box: with C = I one leapfrog step from (q, z) gives q' = q (1 - e^2 / 2) + e z and
    z' = z - (e / 2) (q + q'), so dH = (|q|^2 + |z|^2 - |q'|^2 - |z'|^2) / 2 in closed form."""

    def __init__(self, d, half=1e6):
        self.bounds = np.stack([np.full(d, -half), np.full(d, half)], axis=1)

    def value_grad(self, q):
        return -0.5 * np.sum(q * q, axis=1), -q, None


def _closed_dh(q, z, e):
    q1 = q * (1.0 - 0.5 * e * e) + e * z
    z1 = z - 0.5 * e * (q + q1)
    return 0.5 * (q @ q + z @ z - q1 @ q1 - z1 @ z1)


@pytest.mark.parametrize("e0", [1e-4, 50.0])
@pytest.mark.parametrize("d", [1, 8])
def test_the_search_brackets_the_crossing_on_a_standard_gaussian(d, e0):
    """From e = 1e-4 (doubling) and from e = 50 (halving): dH at the returned e and dH at e 2^-dir lie on opposite sides of ln 0.8 by
    the closed form, each with the draw of the iteration that judged it (the last one and the one before: every iteration draws
    afresh, so the bracket holds for these draws and for no others)."""
    tgt = _StdGaussian(d)
    W, seed, step = 6, 31 + d, 9
    q = np.random.RandomState(seed).randn(W, d)
    lp = tgt.value_grad(q)[0]
    rec = {}
    ln_e, iters = nan_.find_step_size(tgt, q, lp, np.eye(d), np.full(W, np.log(e0)), seed, step, rec=rec)
    want_dir = 1 if e0 < 1 else -1
    assert np.all((0 < iters) & (iters < nan_.SEARCH_CAP)) and min(rec["search"]) > 1e-9
    assert np.array_equal(np.round((ln_e - np.log(e0)) / nan_.LN2), want_dir * iters)
    for w in range(W):
        z = nan_.search_normals(seed, step, [w], int(iters[w]), d)[0]
        e = float(np.exp(ln_e[w]))
        z_before = nan_.search_normals(seed, step, [w], int(iters[w]) - 1, d)[0]
        here, before = _closed_dh(q[w], z, e), _closed_dh(q[w], z_before, e * 2.0 ** -want_dir)
        assert abs(here - nan_.search_dh(tgt, q[w], lp[w], -q[w], np.eye(d), e, z)) < 1e-9 * (1 + abs(here))
        if want_dir > 0:
            assert not here > LN08 and before > LN08
        else:
            assert not here < LN08 and before < LN08
        # the draws of the iterations in front of the last one all said "go on"
        for i in range(int(iters[w])):
            zi = nan_.search_normals(seed, step, [w], i, d)[0]
            dh = _closed_dh(q[w], zi, e0 * 2.0 ** (want_dir * i))
            assert dh > LN08 if want_dir > 0 else dh < LN08


class _Flat:
    def __init__(self, d, half):
        self.bounds = np.stack([np.full(d, -half), np.full(d, half)], axis=1)

    def value_grad(self, q):
        return np.zeros(len(q)), np.zeros_like(q), None


def test_the_cap_is_reported_on_a_flat_target():
    """A flat log-probability inside a box of half-width 1e30: dH = 0 > ln 0.8 at every step size, 40 doublings, iters = 40.  In a
    box of half-width 3 the doubling ends where the step leaves the box (dH = -inf)."""
    d, W = 3, 4
    q = np.zeros((W, d))
    ln_e, iters = nan_.find_step_size(_Flat(d, 1e30), q, np.zeros(W), np.eye(d), np.full(W, np.log(1e-4)), 5, 0)
    assert np.all(iters == 40) and np.allclose(ln_e, np.log(1e-4) + 40 * nan_.LN2, rtol=0, atol=1e-12)
    ln_e, iters = nan_.find_step_size(_Flat(d, 3.0), q, np.zeros(W), np.eye(d), np.full(W, np.log(1e-4)), 5, 0)
    assert np.all((iters > 10) & (iters < 25)) and np.all(np.exp(ln_e) > 1.0)


def test_search_draws_do_not_collide_with_a_moves():
    """Iteration i, coordinate k reads stream word 11 + 16 (64 (i + 1) + k) >= 11 + 16 * 64: beyond every b = k < 64 of streams
    11 ... 15 at the same counter."""
    words = {11 + 16 * (64 * (i + 1) + k) for i in range(40) for k in range(64)}
    moves = {s + 16 * b for s in (2, 3, 11, 12, 13) for b in range(64)} | {14 + 16 * b for b in range(1023)} | {15 + 16 * b for b in range(10)}
    assert len(words) == 40 * 64 and not (words & moves) and max(words) < 2 ** 32


# ------------------------------------------------------------------------------------------- 4. the model's whole warm-up
# NOTES.md "NUTS warm-up": five seeds of the model on the 8-D Gaussian gave mean acceptance statistics 0.7761 ... 0.7815 and variance
# ratios 0.883 ... 1.113; each band is that range widened by its own spread on either side.
GAUSS_ACCEPT_BAND = (0.7761 - 0.0054, 0.7815 + 0.0054)
GAUSS_RATIO_BAND = (0.883 - 0.230, 1.113 + 0.230)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_model_warmup_on_a_gaussian(seed):
    """README's 8-D Gaussian (standard deviations log-spaced 0.1 ... 1, 16 walkers, 300 transitions, identity start, max_depth 8,
    the search on): the terminal buffer's mean acceptance statistic and the recovered variances inside the bands above, and a pooled
    step size that is not hmc_adapt_numpy.warmup's with n_leapfrog = 4 -- the two adapt different statistics."""
    d = 8
    sd = np.logspace(-1.0, 0.0, d)
    tgt = hm.GaussianTarget(np.zeros(d), np.diag(sd ** 2), np.stack([np.full(d, -10.0), np.full(d, 10.0)], axis=1))
    p0 = np.random.RandomState(seed).randn(16, d) * sd
    w = nan_.warmup(tgt, p0, 300, seed, (1.0, hm.default_step_size(d), 8, None, 1.0), metric="diag")
    h = han.warmup(tgt, p0, 300, seed, (1.0, hm.default_step_size(d), 4, None, 1.0), metric="diag")
    ratio = w.cov / sd ** 2
    print(f"seed {seed}: mean accept stat {w.mean_accept_stat:.4f}, step size {w.step_size:.4f} (HMC, 4 leapfrog steps: {h.step_size:.4f}), "
          f"variance ratios {ratio.min():.3f} ... {ratio.max():.3f}, mean depth {w.mean_depth:.2f}")
    assert w.window_ends == [100, 150, 250] and len(w.step_sizes) == 3 and len(w.search_iters) == 4
    assert GAUSS_ACCEPT_BAND[0] < w.mean_accept_stat < GAUSS_ACCEPT_BAND[1]
    assert GAUSS_RATIO_BAND[0] < ratio.min() and ratio.max() < GAUSS_RATIO_BAND[1]
    assert abs(w.step_size - h.step_size) > 1e-3 * h.step_size


def test_model_warmup_on_the_end_to_end_problem():
    """The band tests/test_gpu_nuts_adapt.py puts on the device's terminal mean acceptance statistic (nac.E2E_BAND: the model's
    range over nac.E2E.seeds widened by its own spread, NOTES.md "NUTS warm-up"), checked on the model's first seed."""
    m = nac.e2e_model(nac.E2E.seed)
    print(f"seed {nac.E2E.seed}: mean accept stat {m.mean_accept_stat:.4f}, step size {m.step_size:.4f}, mean depth {m.mean_depth:.2f}")
    assert nac.E2E_BAND[0] < m.mean_accept_stat < nac.E2E_BAND[1]
    assert m.window_ends == [100, 150, 250] and m.cov.shape == (nac.E2E.d,) and np.all(m.cov > 0) and m.divergences == 0


# --------------------------------------------------------------------------------------------------------- 5. host pieces
def test_searched_state():
    from alabi_amd.hmc_adapt import DA_WORDS, searched_state
    ln_e = np.log([0.5, 0.01, 3.0])
    st = searched_state(ln_e)
    assert st.shape == (3, DA_WORDS) and np.array_equal(st, nan_.searched_state(ln_e))
    assert np.all(st[:, 0] == 0) and np.all(st[:, 1] == 0) and np.array_equal(st[:, 2], ln_e) and np.array_equal(st[:, 3], ln_e)
    assert np.array_equal(st[:, 4], np.log(10.0) + ln_e)
    import torch
    assert np.array_equal(searched_state(torch.as_tensor(ln_e)), st)


def test_abi_symbols():
    from alabi_amd import _lib
    text = open(os.path.join(ROOT, "include", "alabi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(alabi_[a-z0-9_]+)\s*\(", text))
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("alabi_ens_nuts_adapt", 15), ("alabi_ens_find_step_size", 8)):
        assert name in declared and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and hasattr(handle, name)
    assert "alabi_ens_hmc_adapt" in declared and len(_lib.SIGNATURES["alabi_ens_hmc_adapt"][1]) == 13          # unchanged


class _FakeGP:
    ndim = 4


def _fake_sampler(monkeypatch, **kw):
    import alabi_amd.sampler as sa
    monkeypatch.setattr(sa, "HipGP", _FakeGP)
    monkeypatch.setattr(sa.torch, "zeros", lambda *a, **k: None)
    monkeypatch.setattr(sa.torch.cuda, "Stream", lambda *a, **k: None)
    monkeypatch.setattr(sa, "_dev", lambda: "cpu")
    monkeypatch.setattr(sa.EnsembleSampler, "__del__", lambda self: None)
    return sa.EnsembleSampler(8, 4, _FakeGP(), None, np.array([[-1.0, 1.0]] * 4), seed=1, **kw)


def test_tune_nuts_refusals(monkeypatch):
    from alabi_amd.moves import GaussianMove, HMCMove, NUTSMove
    p0 = np.zeros((8, 4))
    with pytest.raises(ValueError, match="tune_nuts.*exactly one NUTSMove"):
        _fake_sampler(monkeypatch).tune_nuts(p0)                                          # the stretch move
    with pytest.raises(ValueError, match="exactly one NUTSMove"):
        _fake_sampler(monkeypatch, moves=[NUTSMove(0.5), NUTSMove(0.2, max_depth=3)]).tune_nuts(p0)
    with pytest.raises(ValueError, match="exactly one NUTSMove.*tune_hmc"):
        _fake_sampler(monkeypatch, moves=HMCMove(0.5)).tune_nuts(p0)
    with pytest.raises(ValueError, match="exactly one NUTSMove"):
        _fake_sampler(monkeypatch, moves=GaussianMove(0.1)).tune_nuts(p0)
    with pytest.raises(ValueError, match="tune_nuts needs the gradient"):
        _fake_sampler(monkeypatch, prior_fn=lambda q: np.zeros(len(q))).tune_nuts(p0)
    with pytest.raises(ValueError, match="tune_nuts needs the gradient"):
        _fake_sampler(monkeypatch, like_fn=lambda q: np.zeros(len(q))).tune_nuts(p0)
    with pytest.raises(ValueError, match="tune_nuts cannot run with shard=True"):
        _fake_sampler(monkeypatch, shard=True).tune_nuts(p0)
    s = _fake_sampler(monkeypatch, moves=NUTSMove(0.5))
    for bad in (dict(metric="full"), dict(init_step_size="stan"), dict(nwarmup=0), dict(target_accept=1.0), dict(gamma=0.0), dict(t0=-1.0),
                dict(kappa=0.5)):
        with pytest.raises(ValueError, match="metric|init_step_size|tune_nuts needs"):
            s.tune_nuts(p0, **bad)
    # tune_hmc still refuses the NUTSMove, and now names the route
    with pytest.raises(ValueError, match="tune_nuts"):
        s.tune_hmc(p0)


def test_find_step_size_refusals(monkeypatch):
    from alabi_amd.moves import GaussianMove, NUTSMove
    p0 = np.zeros((8, 4))
    with pytest.raises(ValueError, match="find_step_size searches the step size of an HMCMove or a NUTSMove"):
        _fake_sampler(monkeypatch).find_step_size(p0)
    with pytest.raises(ValueError, match="HMCMove or a NUTSMove"):
        _fake_sampler(monkeypatch, moves=GaussianMove(0.1)).find_step_size(p0)
    with pytest.raises(ValueError, match="find_step_size needs the gradient"):
        _fake_sampler(monkeypatch, prior_fn=lambda q: np.zeros(len(q))).find_step_size(p0)
    with pytest.raises(ValueError, match="find_step_size cannot run with shard=True"):
        _fake_sampler(monkeypatch, shard=True).find_step_size(p0)
    with pytest.raises(ValueError, match="k_move"):
        _fake_sampler(monkeypatch, moves=NUTSMove(0.5)).find_step_size(p0, k_move=1)
    with pytest.raises(ValueError, match="needs coords"):
        _fake_sampler(monkeypatch, moves=NUTSMove(0.5)).find_step_size()


def test_run_emcee_refuses_the_nuts_keys_without_a_single_nuts_move():
    from alabi_amd import SurrogateModel
    from alabi_amd.moves import GaussianMove, HMCMove, NUTSMove
    sm = SurrogateModel.__new__(SurrogateModel)
    sm.ndim = 3
    for moves in (None, GaussianMove(0.1), HMCMove(0.5), [NUTSMove(0.5), NUTSMove(0.2)]):
        for key, val in (("nuts_warmup", 50), ("nuts_target_accept", 0.7), ("nuts_metric", "dense"), ("nuts_init_step_size", None)):
            kw = {key: val} if moves is None else {"moves": moves, key: val}
            with pytest.raises(ValueError, match="single NUTSMove"):
                sm.run_emcee(sampler_kwargs=kw)
    with pytest.raises(ValueError, match="positive number of warm-up transitions"):
        sm.run_emcee(sampler_kwargs={"moves": NUTSMove(0.5), "nuts_target_accept": 0.7})
    with pytest.raises(ValueError, match="positive number of warm-up transitions"):
        sm.run_emcee(sampler_kwargs={"moves": NUTSMove(0.5), "nuts_warmup": 0})
    with pytest.raises(ValueError, match='tune an HMCMove.*|nuts_warmup'):          # the hmc_* keys keep refusing a NUTSMove
        sm.run_emcee(sampler_kwargs={"moves": NUTSMove(0.5), "hmc_warmup": 10})
