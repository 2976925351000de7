"""Host tests of the HMC move: the NumPy model (tests/hmc_numpy.py) against finite differences, the leapfrog map's symmetries, the
sampled distribution on analytic Gaussians with and without a cutting box, ``parse_moves`` / ``MoveSet`` for ``HMCMove``, and the
honesty of every model run the GPU tests compare against.  No GPU, no library."""
import pickle

import numpy as np
import pytest

import hmc_cases as hc
import hmc_numpy as hm
import moves_shapes_common as ms
from oracle.autocorr_oracle import integrated_time


# ------------------------------------------------------------------------------------------------- 1. the model's gradient
GRAD_CASES = [(3, k, {}) for k in ("ExpSquared", "Matern32", "Matern52", "RationalQuadratic")] + [
    (5, "ExpSquared", dict(ymap="nlog")), (5, "ExpSquared", dict(ymap="log")),
    (17, "Matern52", dict(affine=ms.AFFINE, prior=ms.normal_prior(17))), (4, "ExpSquared", dict(affine=ms.AFFINE, prior=ms.normal_prior(4)))]


@pytest.mark.parametrize("d,kernel,ex", GRAD_CASES, ids=lambda v: str(v) if not isinstance(v, dict) else "+".join(sorted(v)) or "bare")
def test_model_gradient_against_central_differences(d, kernel, ex):
    """grad lnp of the model equals central differences of the model's own lnp (h = 1e-5) to 1e-6 relative."""
    prob = ms.problem(d, kernel, ymap=ex.get("ymap"))
    tgt = hc.target_of(prob, ex)
    q = np.random.RandomState(d).uniform(-2.5, 2.5, (6, d))
    _, g, _ = tgt.value_grad(q)
    h = 1e-5
    num = np.empty_like(g)
    for k in range(d):
        dq = np.zeros(d); dq[k] = h
        num[:, k] = (tgt.value_grad(q + dq)[0] - tgt.value_grad(q - dq)[0]) / (2 * h)
    assert np.max(np.abs(g)) > 1e-3
    assert np.max(np.abs(num - g)) < 1e-6 * np.max(np.abs(g))


# ------------------------------------------------------------------------------------------------------- 2. the leapfrog
def _leapfrog_setup(form, L):
    d = 5
    prob = ms.problem(d, "Matern52")
    tgt = hc.target_of(prob, hc.extras(d))
    rs = np.random.RandomState(11)
    x, z0 = rs.uniform(-2, 2, (8, d)), rs.randn(8, d)
    C, _ = hm.gm.scale_factor(hc.cov_of(form, d), d)
    lp, g, _ = tgt.value_grad(x)
    return tgt, x, z0, C, lp, g


@pytest.mark.parametrize("form,L", [("vector", 1), ("matrix", 4), ("scalar", 8)])
def test_leapfrog_is_reversible(form, L):
    """Forward, negate z, forward again returns x and z0 to 1e-10."""
    tgt, x, z0, C, lp, g = _leapfrog_setup(form, L)
    e = 0.3
    q, z, lpq, gq, _ = hm.leapfrog(tgt, x, g, C, e, z0, L)
    assert np.max(np.abs(q - x)) > 0.05
    x2, z2, lp2, _, _ = hm.leapfrog(tgt, q, gq, C, e, -z, L)
    assert np.max(np.abs(x2 - x)) < 1e-10 and np.max(np.abs(-z2 - z0)) < 1e-10 and np.max(np.abs(lp2 - lp)) < 1e-10


@pytest.mark.parametrize("form", ["vector", "matrix"])
def test_one_leapfrog_step_is_mala(form):
    """With n_leapfrog = 1 the proposal is x + (e^2 / 2) C C^T g + e C z0 and the energy difference is the Hastings ratio of the
    Metropolis-adjusted Langevin proposal N(x + (e^2 / 2) cov g, e^2 cov), to 1e-12."""
    tgt, x, z0, C, lp, g = _leapfrog_setup(form, 1)
    e = 0.35
    cov = C @ C.T
    q, z, lpq, gq, _ = hm.leapfrog(tgt, x, g, C, e, z0, 1)
    assert np.max(np.abs(q - (x + 0.5 * e * e * g @ cov + e * z0 @ C.T))) < 1e-13
    dh = lpq - 0.5 * np.sum(z * z, axis=1) - lp + 0.5 * np.sum(z0 * z0, axis=1)
    Ci = np.linalg.inv(C)

    def log_q(to, frm, g_frm):        # log N(to; frm + (e^2 / 2) cov g_frm, e^2 cov) up to the shared constant
        r = (to - frm - 0.5 * e * e * g_frm @ cov) @ Ci.T
        return -0.5 * np.sum(r * r, axis=1) / (e * e)
    hastings = lpq - lp + log_q(x, q, gq) - log_q(q, x, g)
    assert np.max(np.abs(dh - hastings)) < 1e-12 * (1 + np.max(np.abs(hastings)))


# ------------------------------------------------------------------------------------------------------- 3. invariance
def _gauss5():
    d = 5
    sd = np.array([0.4, 1.0, 0.7, 1.5, 0.9])
    corr = 0.6 ** np.abs(np.arange(d)[:, None] - np.arange(d)[None, :])
    return np.array([0.3, -0.5, 0.0, 1.0, -0.2]), sd[:, None] * corr * sd[None, :]


def _sample_hmc(tgt, x0, nsteps, C, eps, L, jitter, seed):
    rs = np.random.RandomState(seed)
    W, d = x0.shape
    x = x0.copy()
    lp, g, _ = tgt.value_grad(x)
    chain = np.empty((nsteps, W, d))
    nacc = 0
    for t in range(nsteps):
        e = eps * np.exp(rs.uniform(-np.log(jitter), np.log(jitter)))
        x, lp, g, acc = hm.hmc_step_arrays(tgt, x, lp, g, C, e, rs.randn(W, d), L, rs.rand(W))
        chain[t] = x
        nacc += acc.sum()
    return chain, nacc / (nsteps * W)


def _assert_moments(chain, mean, cov):
    """Mean and covariance of the chain within 5 standard errors, the standard error of each estimate from the run's own
    effective sample size: sd(series) sqrt(tau / n) with tau the integrated autocorrelation time (oracle.autocorr_oracle) of that
    very series -- a coordinate, or a product of two centred coordinates."""
    nsteps, W, d = chain.shape
    n = nsteps * W
    tau = integrated_time(chain)
    flat = chain.reshape(-1, d)
    se = flat.std(axis=0) * np.sqrt(np.maximum(tau, 1.0) / n)
    assert np.all(np.abs(flat.mean(axis=0) - mean) < 5 * se), (flat.mean(axis=0) - mean, se)
    cen = chain - mean
    iu = np.triu_indices(d)
    prod = cen[:, :, iu[0]] * cen[:, :, iu[1]]                   # [nsteps, W, d (d + 1) / 2]
    tau2 = integrated_time(prod)
    p = prod.reshape(n, -1)
    se2 = p.std(axis=0) * np.sqrt(np.maximum(tau2, 1.0) / n)
    assert np.all(np.abs(p.mean(axis=0) - cov[iu]) < 5 * se2), (p.mean(axis=0) - cov[iu], se2)
    return se, se2


def test_hmc_leaves_a_correlated_gaussian_invariant():
    """16 walkers x 4000 steps on an analytic 5-D correlated Gaussian whose box is far away, started from exact draws: mean and
    covariance within 5 standard errors of the run's own effective sample size."""
    mean, cov = _gauss5()
    tgt = hm.GaussianTarget(mean, cov, np.stack([mean - 50.0, mean + 50.0], axis=1))
    x0 = np.random.RandomState(1).multivariate_normal(mean, cov, 16)
    C = np.linalg.cholesky(cov * 0.8)                            # a slightly wrong mass matrix
    chain, acc = _sample_hmc(tgt, x0, 4000, C, 0.9, 3, 1.3, 2)
    assert 0.5 < acc < 1.0
    se, _ = _assert_moments(chain, mean, cov)
    assert np.all(se < 0.05 * np.sqrt(np.diag(cov)) * 2)         # the bound is tight enough to mean something


def test_the_box_rule_leaves_the_truncated_gaussian_invariant():
    """The same with a box that cuts coordinate 0 at mean + 1 sigma: only the end point of a trajectory is tested against the
    box, and the chain has the moments of the Gaussian truncated there."""
    from scipy.stats import norm
    mean, cov = _gauss5()
    b = np.stack([mean - 50.0, mean + 50.0], axis=1)
    b[0, 1] = mean[0] + np.sqrt(cov[0, 0])
    tgt = hm.GaussianTarget(mean, cov, b)
    lam = norm.pdf(1.0) / norm.cdf(1.0)
    m1, v = -lam, 1.0 - lam - lam * lam                          # mean and variance of the standard normal truncated to (-inf, 1)
    s0 = np.sqrt(cov[0, 0])
    t_mean = mean + cov[:, 0] / s0 * m1
    t_cov = cov - np.outer(cov[:, 0], cov[0, :]) / cov[0, 0] * (1.0 - v)
    rs = np.random.RandomState(3)
    x0 = rs.multivariate_normal(mean, cov, 200)
    x0 = x0[tgt.inside(x0)][:16]
    chain, acc = _sample_hmc(tgt, x0, 4000, np.linalg.cholesky(cov), 0.8, 2, 1.3, 4)
    assert 0.4 < acc < 1.0
    assert np.all(chain[:, :, 0] < b[0, 1])
    _assert_moments(chain, t_mean, t_cov)
    # the untruncated moments are NOT what the chain has: the test can tell the two apart
    flat0 = chain[:, :, 0].ravel()
    assert abs(flat0.mean() - mean[0]) > 10 * flat0.std() * np.sqrt(max(integrated_time(chain)[0], 1.0) / flat0.size)


# ------------------------------------------------------------------------------------------- 4. parse_moves / MoveSet
def test_hmc_move_validation():
    from alabi_amd.moves import HMCMove
    for bad in (dict(step_size=0.0), dict(step_size=-1.0), dict(step_size=np.inf), dict(step_size=np.nan), dict(n_leapfrog=0),
                dict(n_leapfrog=65), dict(n_leapfrog=2.5), dict(n_leapfrog=True), dict(jitter=1.0), dict(jitter=0.5), dict(jitter=np.inf)):
        with pytest.raises(ValueError):
            HMCMove(1.0, **bad)
    for bad_cov in (-1.0, [1.0, 0.0], [[1.0, 2.0], [2.0, 1.0]], np.zeros((2, 3)), [np.nan], np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            HMCMove(bad_cov)
    m = HMCMove([[2.0, 0.3], [0.3, 1.0]], step_size=0.2, n_leapfrog=64, jitter=1.5)
    assert not m.diagonal and m.ndim == 2 and np.allclose(m.scale_matrix(2) @ m.scale_matrix(2).T, m.cov)
    assert HMCMove(0.5).diagonal and HMCMove(0.5).n_leapfrog == 8 and HMCMove(0.5).step_size is None and HMCMove(0.5).jitter is None
    m2 = pickle.loads(pickle.dumps(m))
    assert repr(m2) == repr(m) and np.array_equal(m2.scale_matrix(2), m.scale_matrix(2))


def test_parse_moves_hmc_rows_and_mixtures():
    from alabi_amd.moves import KIND_HMC, HMCMove, MoveSet, StretchMove, parse_moves
    d = 16
    ms1 = parse_moves(HMCMove(0.5), d)
    assert isinstance(ms1, MoveSet) and ms1.all_hmc and ms1.has_hmc and not ms1.all_metropolis and not ms1.has_gauss and not ms1.multi_partner
    assert list(ms1.kind) == [KIND_HMC] and ms1.p0[0] == d ** -0.25 == 0.5 and ms1.p1[0] == 8.0
    mix = parse_moves([(HMCMove(np.full(d, 0.2), step_size=0.1, n_leapfrog=3, jitter=1.5), 3.0),
                       (HMCMove(0.4 * np.eye(d), n_leapfrog=1), 1.0)], d)
    assert mix.all_hmc and np.allclose(mix.cum, [0.75, 1.0]) and list(mix.p0) == [0.1, 0.5]
    L = np.floor(mix.p1); lnj = (mix.p1 - L) * 512.0
    assert list(L) == [3.0, 1.0] and lnj[1] == 0.0
    assert lnj[0] == hm.ln_jitter(1.5) and abs(lnj[0] - np.log(1.5)) < 2.0 ** -36    # both parts come apart exactly
    kinds, cum, p0, p1, _ = hm.move_table([(np.full(d, 0.2), 0.1, 3, 1.5, 3.0), (0.4 * np.eye(d), None, 1, None, 1.0)], d)
    assert np.array_equal(kinds, mix.kind) and np.array_equal(cum, mix.cum) and np.array_equal(p0, mix.p0) and np.array_equal(p1, mix.p1)
    sc = mix.scales()
    assert [(k, diag) for k, _, diag in sc] == [(0, True), (1, False)]
    assert np.allclose(sc[0][1], np.sqrt(0.2) * np.eye(d)) and np.allclose(sc[1][1], np.sqrt(0.4) * np.eye(d))
    assert parse_moves(None, d) is None and not parse_moves(StretchMove(), 4).has_hmc and not parse_moves(StretchMove(), 4).all_hmc
    with pytest.raises(ValueError, match="Dimension mismatch"):
        parse_moves(HMCMove(np.ones(3)), d)


def test_an_hmc_set_holds_hmc_moves_only():
    from alabi_amd.moves import DEMove, GaussianMove, HMCMove, MHMove, StretchMove, parse_moves
    for other in (StretchMove(), DEMove(), GaussianMove(0.1), MHMove(lambda c, r: (c, np.zeros(len(c))))):
        with pytest.raises(ValueError, match="not built|MHMove"):
            parse_moves([HMCMove(0.5), other], 4)
        with pytest.raises(ValueError, match="not built|MHMove"):
            parse_moves([(other, 0.5), (HMCMove(0.5), 0.5)], 4)


class _FakeGP:
    ndim = 4


def test_sampler_refusals_without_a_gradient(monkeypatch):
    """A Python prior_fn or like_fn and shard=True are refused with a clear ValueError; any nwalkers >= 1 is accepted."""
    import alabi_amd.sampler as sa
    from alabi_amd.moves import HMCMove
    monkeypatch.setattr(sa, "HipGP", _FakeGP)
    monkeypatch.setattr(sa.torch, "zeros", lambda *a, **k: None)
    monkeypatch.setattr(sa.torch.cuda, "Stream", lambda *a, **k: None)
    monkeypatch.setattr(sa, "_dev", lambda: "cpu")
    monkeypatch.setattr(sa.EnsembleSampler, "__del__", lambda self: None)
    b = np.array([[-1.0, 1.0]] * 4)
    with pytest.raises(ValueError, match="gradient"):
        sa.EnsembleSampler(8, 4, _FakeGP(), None, b, moves=HMCMove(0.5), prior_fn=lambda q: np.zeros(len(q)))
    with pytest.raises(ValueError, match="gradient"):
        sa.EnsembleSampler(8, 4, _FakeGP(), None, b, moves=HMCMove(0.5), like_fn=lambda q: np.zeros(len(q)))
    with pytest.raises(ValueError, match="shard=True cannot run an HMCMove"):
        sa.EnsembleSampler(8, 4, _FakeGP(), None, b, moves=HMCMove(0.5), shard=True)
    for W in (1, 2, 3, 40):
        s = sa.EnsembleSampler(W, 4, _FakeGP(), None, b, moves=[(HMCMove(0.5), 1.0), (HMCMove(0.2, n_leapfrog=1), 2.0)], seed=1)
        assert s._move_set.all_hmc and [type(m).__name__ for m, _ in s.moves] == ["HMCMove", "HMCMove"]
        st = s.__getstate__()
        assert st["_ens"] is None and st["_move_set"].all_hmc


def test_existing_error_texts_are_unchanged():
    from alabi_amd.moves import GaussianMove, MHMove, parse_moves
    with pytest.raises(ValueError, match="a move set that holds an MHMove must consist of MHMove objects only"):
        parse_moves([MHMove(lambda c, r: (c, 0)), GaussianMove(0.1)], 3)

    class DESnookerMove:
        pass
    with pytest.raises(NotImplementedError, match="move DESnookerMove is not available on the GPU"):
        parse_moves(DESnookerMove(), 3)


# ---------------------------------------------------------------------------------- 5. the model runs the GPU tests use
@pytest.mark.parametrize("name,st", list(hc.all_model_runs()), ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else "")
def test_every_model_run_is_honest(name, st):
    """At least one accept, one in-box reject and one out-of-box end point, the smallest accept-test margin above MIN_MARGIN, a
    surrogate that varies: ``assert_honest``'s terms."""
    ms.assert_honest(st, name)


def test_the_mixture_chooses_both_moves_and_the_ensembles_differ():
    two = hc.model_chain("two")
    assert set(two.counts[0]) == {0, 1}
    ens = hc.model_chain("ens3")
    assert len({tuple(np.round(r, 12)) for r in ens.chain[-1].reshape(3, -1)}) == 3
