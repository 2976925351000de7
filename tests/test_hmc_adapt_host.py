"""Host checks of the HMC warm-up (no GPU): the window schedule, the shrunk covariance and the pooled step size of
alabi_amd/hmc_adapt.py, the honesty of every model run tests/test_gpu_hmc_adapt.py compares the device with, the CPU model's own
warm-up on an analytic Gaussian, and the refusals that need no device."""
import numpy as np
import pytest

import hmc_adapt_cases as hac
import hmc_adapt_numpy as han
import hmc_numpy as hm
import moves_shapes_common as ms


# ------------------------------------------------------------------------------------------------------ 1. the schedule
@pytest.mark.parametrize("n,ends", [(1000, [100, 150, 250, 450, 950]), (150, [100]), (100, [90]), (19, []), (500, [100, 150, 250, 450]),
                                    (20, [18]), (0, [])])
def test_warmup_windows(n, ends):
    from alabi_amd.hmc_adapt import warmup_segments, warmup_windows
    assert warmup_windows(n) == ends
    assert han.schedule(n)[1] == ends                       # the model states the schedule a second time
    segs = warmup_segments(n)
    assert [s[1] for s in segs if s[2]] == ends
    if n > 0:
        assert segs[0][0] == 0 and segs[-1][1] == n and all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
        assert all(e > f for f, e, _ in segs)
        assert warmup_segments(n, windows=False) == [(0, n, False)]
    if ends:
        assert not segs[-1][2]                              # a terminal buffer follows the last window


# ----------------------------------------------------------------------------------------------------- 2. the shrinkage
def test_regularised_covariance_by_hand():
    from alabi_amd.hmc_adapt import regularised_covariance
    x = np.array([[1.0, 2.0], [3.0, 1.0], [2.0, 6.0], [6.0, 3.0]])          # n = 4: means (3, 3)
    # sums of squares about the mean: 14 and 14, cross product (-2)(-1) + 0 + (-1)(3) + (3)(0) = -1; divided by n - 1 = 3
    S = np.array([[14.0, -1.0], [-1.0, 14.0]]) / 3.0
    want = 4.0 / 9.0 * S + 1e-3 * 5.0 / 9.0 * np.eye(2)
    assert np.allclose(regularised_covariance(x, "dense"), want, rtol=1e-14, atol=0)
    assert np.allclose(regularised_covariance(x, "diag"), np.diag(want), rtol=1e-14, atol=0)
    assert np.allclose(han.shrunk_covariance(x, "dense"), want, rtol=1e-14, atol=0)
    with pytest.raises(ValueError):
        regularised_covariance(x, "full")
    import torch
    assert np.allclose(regularised_covariance(torch.as_tensor(x), "dense"), want, rtol=1e-13, atol=0)
    assert np.allclose(regularised_covariance(torch.as_tensor(x).reshape(2, 2, 2), "diag"), np.diag(want), rtol=1e-13, atol=0)


def test_dense_shrinkage_stays_positive_definite_with_fewer_samples_than_dimensions():
    from alabi_amd.hmc_adapt import regularised_covariance
    from alabi_amd.moves import HMCMove
    x = np.random.RandomState(3).randn(5, 12)               # rank 4 at most
    S = regularised_covariance(x, "dense")
    assert np.array_equal(S, S.T)
    assert np.linalg.eigvalsh(S).min() >= 0.99 * 1e-3 * 5.0 / 10.0
    np.linalg.cholesky(S)
    HMCMove(S)                                              # the move factorises it


def test_pooled_step_size():
    from alabi_amd.hmc_adapt import pooled_step_size
    v = np.log(np.array([0.1, 0.4, 0.2, 0.8]))
    assert pooled_step_size(v) == pytest.approx((0.1 * 0.4 * 0.2 * 0.8) ** 0.25, rel=1e-15)
    import torch
    assert pooled_step_size(torch.as_tensor(v)) == pooled_step_size(v)


def test_the_states_of_the_module_and_of_the_model_agree():
    from alabi_amd import hmc_adapt as ha
    assert np.array_equal(ha.initial_state(3, 0.37), han.initial_state(3, 0.37))
    assert np.array_equal(ha.restart_state(3, 0.37), han.restart_state(3, 0.37))
    assert ha.DA_DEFAULTS == han.DEFAULT_PAR and ha.DA_WORDS == 5


def test_the_update_by_hand():
    """One update from the initial state at e = 0.5 with a = 1: H-bar = -0.2 / 11, ln e = ln 5 + 20 * 0.2 / 11, ln e-bar = ln e."""
    st = han.da_update(han.initial_state(1, 0.5), np.array([1.0]), han.DEFAULT_PAR)[0]
    assert st[0] == 1.0 and st[1] == pytest.approx(-0.2 / 11.0, rel=1e-14)
    assert st[2] == pytest.approx(np.log(5.0) + 20.0 * 0.2 / 11.0, rel=1e-14) and st[3] == st[2] and st[4] == np.log(5.0)
    frozen = han.da_update(han.initial_state(1, 0.5), np.array([0.0]), (0.8, np.inf, 10.0, 0.75))[0]
    assert frozen[2] == frozen[4]                           # gamma = inf: ln e stays at mu


# ------------------------------------------------------------------------------- 3. the model runs the GPU tests compare with
@pytest.mark.parametrize("name", list(hac.CASES))
def test_every_model_run_is_honest_and_covers_the_acceptance_statistic(name):
    """``assert_honest``'s terms (no margin below MIN_MARGIN, an accept, an in-box reject, an out-of-box end point, a surrogate that
    varies), and acceptance statistics that are exactly 0, strictly between 0 and 1, and exactly 1."""
    r = hac.model_run(name)
    assert r.W <= 16 and len(r.run.alpha) == hac.ADAPT_STEPS == 40 and hac.PAR == (0.8, 0.05, 10.0, 0.75)
    ms.assert_honest(r.stats, name)
    zero, inner, one = hac.alpha_cover(r.run.alpha)
    assert zero >= 1 and inner >= 1 and one >= 1, (name, zero, inner, one)
    assert np.all(r.run.state[:, 0] == hac.ADAPT_STEPS) and np.all(np.isfinite(r.run.state))
    assert len(r.trace) == hac.ADAPT_STEPS


@pytest.mark.parametrize("name", list(hac.CASES))
def test_every_free_run_is_well_conditioned(name):
    """A start perturbed by 1e-15 relative moves ln e, ln e-bar and the sums of the acceptance statistic by less than 1e-8 over the
    40 steps -- a hundredth of the 1e-6 cap of the GPU test's tolerance, which leaves room for a device whose every sum rounds
    differently.  (At the default seeds d1 moved by 1.6 and matrix by 2.8e-7: their seeds are chosen for this.)"""
    s = hac.rounding_sensitivity(name)
    print(f"{name}: {s:.2e}")
    assert s < 1e-8


def test_the_ensembles_of_a_case_draw_their_own_jitter():
    r = hac.model_run("ens3")
    solo = han.run_hmc_adapt(hac.hc.target_of(r.prob, r.ex), r.p0[r.W:2 * r.W], 5, r.seed, r.move, hac.PAR, r.state0[r.W:2 * r.W],
                             id0=r.W)
    assert np.array_equal(solo.chain, r.run.chain[:5, r.W:2 * r.W]) and np.array_equal(solo.state[:, :4], r.trace[5][2][r.W:2 * r.W, :4])


# ------------------------------------------------------------------------------------------- 4. the model's whole warm-up
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_warmup_on_a_gaussian(seed):
    """8-D Gaussian with standard deviations log-spaced 0.1 ... 1, 16 walkers, nwarmup = 300, metric "diag" from identity mass:
    the terminal buffer's mean acceptance statistic is within 0.05 of 0.8 and the adapted variances within a factor 2 of the truth."""
    d = 8
    sd = np.logspace(-1.0, 0.0, d)
    tgt = hm.GaussianTarget(np.zeros(d), np.diag(sd ** 2), np.stack([np.full(d, -10.0), np.full(d, 10.0)], axis=1))
    p0 = np.random.RandomState(seed).randn(16, d) * sd
    w = han.warmup(tgt, p0, 300, seed, (1.0, hm.default_step_size(d), 8, None, 1.0), metric="diag")
    print(f"seed {seed}: mean accept stat {w.mean_accept_stat:.3f}, step size {w.step_size:.3f}, variance ratios "
          f"{np.min(w.cov / sd ** 2):.2f} ... {np.max(w.cov / sd ** 2):.2f}")
    assert w.window_ends == [100, 150, 250] and len(w.step_sizes) == 3
    assert abs(w.mean_accept_stat - 0.8) < 0.05
    assert np.all(w.cov / sd ** 2 < 2.0) and np.all(w.cov / sd ** 2 > 0.5)


def test_model_warmup_on_the_end_to_end_problem():
    """The bounds tests/test_gpu_hmc_adapt.py puts on the device, checked on the model first: over its seeds the terminal mean
    acceptance statistic stays within 0.05 of 0.8 (the device gets twice that) and the next 200 steps accept a fraction in (0.5, 1)."""
    for seed in hac.E2E.seeds:
        m = hac.e2e_model(seed)
        assert abs(m.warm.mean_accept_stat - 0.8) < 0.05, (seed, m.warm.mean_accept_stat)
        assert 0.5 < m.acc_frac < 1.0
        assert m.warm.cov.shape == (hac.E2E.d,) and np.all(m.warm.cov > 0)


# --------------------------------------------------------------------------------------------------------- 5. refusals
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


def test_tune_hmc_refusals(monkeypatch):
    from alabi_amd.moves import GaussianMove, HMCMove
    p0 = np.zeros((8, 4))
    with pytest.raises(ValueError, match="exactly one HMCMove"):
        _fake_sampler(monkeypatch).tune_hmc(p0)                                           # the stretch move
    with pytest.raises(ValueError, match="exactly one HMCMove"):
        _fake_sampler(monkeypatch, moves=[HMCMove(0.5), HMCMove(0.2, n_leapfrog=1)]).tune_hmc(p0)
    with pytest.raises(ValueError, match="exactly one HMCMove"):
        _fake_sampler(monkeypatch, moves=GaussianMove(0.1)).tune_hmc(p0)
    with pytest.raises(ValueError, match="gradient"):
        _fake_sampler(monkeypatch, prior_fn=lambda q: np.zeros(len(q))).tune_hmc(p0)
    with pytest.raises(ValueError, match="gradient"):
        _fake_sampler(monkeypatch, like_fn=lambda q: np.zeros(len(q))).tune_hmc(p0)
    with pytest.raises(ValueError, match="shard=True"):
        _fake_sampler(monkeypatch, shard=True).tune_hmc(p0)
    s = _fake_sampler(monkeypatch, moves=HMCMove(0.5))
    for bad in (dict(metric="full"), dict(nwarmup=0), dict(target_accept=1.0), dict(gamma=0.0), dict(t0=-1.0), dict(kappa=0.5)):
        with pytest.raises(ValueError, match="metric|tune_hmc needs"):
            s.tune_hmc(p0, **bad)


def test_run_emcee_refuses_the_warmup_keys_without_a_single_hmc_move():
    from alabi_amd import SurrogateModel
    from alabi_amd.moves import GaussianMove, HMCMove
    sm = SurrogateModel.__new__(SurrogateModel)
    sm.ndim = 3
    for moves in (None, GaussianMove(0.1), [HMCMove(0.5), HMCMove(0.2)]):
        for key, val in (("hmc_warmup", 50), ("hmc_target_accept", 0.7), ("hmc_metric", "dense")):
            kw = {key: val} if moves is None else {"moves": moves, key: val}
            with pytest.raises(ValueError, match="single HMCMove"):
                sm.run_emcee(sampler_kwargs=kw)
    with pytest.raises(ValueError, match="positive number of warm-up steps"):
        sm.run_emcee(sampler_kwargs={"moves": HMCMove(0.5), "hmc_target_accept": 0.7})
    with pytest.raises(ValueError, match="positive number of warm-up steps"):
        sm.run_emcee(sampler_kwargs={"moves": HMCMove(0.5), "hmc_warmup": 0})
