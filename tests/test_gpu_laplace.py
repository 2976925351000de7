"""SurrogateModel.find_map(method="bfgs-gpu") and SurrogateModel.laplace_approximation end to end on a surrogate trained on a 3-D
Gaussian log-likelihood: the device optimiser against the Nelder-Mead default, the Laplace attributes, the evidence estimate
against the formula evaluated from tests/hess_reference.py's truth Hessian, the covariance handed to an HMCMove, and a model whose
maximum sits on a wall."""
import warnings

import numpy as np
import pytest

import hess_reference as hr

pytestmark = pytest.mark.gpu

BOUNDS = [(-3.0, 3.0)] * 3
PREC = np.array([[2.0, 0.6, 0.0], [0.6, 1.5, -0.4], [0.0, -0.4, 1.0]])


class _Gauss:
    """-(theta - mean)^T PREC (theta - mean) / 2; a class at module level, so that a model holding it can be pickled."""

    def __init__(self, mean):
        self.mean = np.asarray(mean, dtype=np.float64)

    def __call__(self, theta):
        r = np.asarray(theta, dtype=np.float64).reshape(-1) - self.mean
        return float(-0.5 * r @ PREC @ r)


_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """The models hold device handles (``_map_sampler``): let go of them with the module, not at interpreter shutdown."""
    yield
    _MODELS.clear()


def _model(tmp_path_factory, key, mean):
    if key not in _MODELS:
        from alabi_amd import SurrogateModel
        sm = SurrogateModel(lnlike_fn=_Gauss(mean), bounds=BOUNDS, savedir=str(tmp_path_factory.mktemp(key)), verbose=False, random_state=0)
        sm.init_samples(ntrain=80, ntest=20, sampler="uniform")
        sm.init_gp(kernel="ExpSquaredKernel", fit_amp=True, fit_mean=True, white_noise=-12, hyperopt_method="ml", gp_nopt=1)
        _MODELS[key] = sm
    return _MODELS[key]


def test_find_map_on_the_device_agrees_with_the_default(tmp_path_factory):
    sm = _model(tmp_path_factory, "interior", (0.5, -0.3, 0.2))
    p0 = sm.find_map(nRestarts=3)                                     # the Nelder-Mead default, untouched
    nm_theta, nm_lp = sm.map_theta.copy(), sm.map_lnprob
    p1 = sm.find_map(method="bfgs-gpu", nRestarts=16)
    assert p0.shape == p1.shape == (30, 3)
    assert sm.map_status == 0 and sm.map_evaluations > 16 and sm.map_theta.shape == (3,)
    sm.laplace_approximation(nRestarts=16)
    # Nelder-Mead stops within xatol = 1e-4 of its optimum: it may lie below the true maximum by |H| d xatol^2 / 2 (and by its
    # fatol = 1e-4); the device value may lie below Nelder-Mead's by no more than the first
    slack = 0.5 * np.linalg.norm(sm.map_hessian, 2) * 3 * 1e-4 ** 2
    print("MAP nelder-mead %.12g, device %.12g (slack %.1e); |theta difference| %.1e" % (nm_lp, sm.map_lnprob, slack,
                                                                                          np.max(np.abs(nm_theta - sm.map_theta))))
    assert sm.map_lnprob >= nm_lp - slack
    assert abs(sm.map_lnprob - nm_lp) <= 1e-4 + slack
    assert np.max(np.abs(nm_theta - sm.map_theta)) < 1e-2
    like = float(np.asarray(sm.surrogate_log_likelihood(sm.map_theta.reshape(1, -1))).reshape(-1)[0])   # the box prior adds 0
    assert abs(sm.map_lnprob - like) <= 1e-9 * max(1.0, abs(like))


def test_laplace_approximation_sets_every_attribute(tmp_path_factory):
    from alabi_amd import laplace as lap
    sm = _model(tmp_path_factory, "interior", (0.5, -0.3, 0.2))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        logz = sm.laplace_approximation(nRestarts=16)
    d = 3
    assert sm.map_status == 0 and logz == sm.laplace_logz and np.isfinite(logz)
    assert sm.map_on_bound.dtype == bool and sm.map_on_bound.shape == (d,) and not sm.map_on_bound.any()
    assert sm.map_hessian.shape == sm.map_cov.shape == sm.map_cov_scaled.shape == (d, d)
    assert np.max(np.abs(sm.map_cov @ (-sm.map_hessian) - np.eye(d))) <= 1e-10
    plan = sm._map_plan
    assert np.allclose(lap.covariance_to_theta(sm.map_cov_scaled, plan.t_mult), sm.map_cov, rtol=1e-14, atol=0)
    # the surrogate of a Gaussian: the covariance is near the likelihood's
    assert np.allclose(sm.map_cov, np.linalg.inv(PREC), rtol=0.2, atol=0.05)
    # the evidence from the truth Hessian at the same point, the Hessian's bound propagated through ln det / 2 to first order:
    # d (ln det(-H) / 2) = tr(H^-1 dH) / 2 <= sum_ab |H^-1_ab| tol_ab / 2
    g = sm._map_sampler.gp
    amp, _, inv_len = hr.ksr.hyper_fp64(g.log_constant, g.white_noise_value, g.log_M)
    Ht, tol = hr.log_prob_hessian(g._x, np.asarray(g._alpha, dtype=np.float64), amp, inv_len, sm._map_coords[None, :], g.mean_value,
                                  g.kernel_name, g.log_alpha, affine=plan.logp_affine, ymap=plan.logp_map, prior=plan.normal_prior)
    Hc = Ht[0].astype(np.float64)
    widths = np.array([b[1] - b[0] for b in BOUNDS])
    want = lap.laplace_log_evidence(sm.map_lnprob, lap.hessian_to_theta(Hc, plan.t_mult), widths)
    allowed = 0.5 * float(np.sum(np.abs(np.linalg.inv(Hc)) * tol[0])) + 8 * d * d * 2.0 ** -53 * max(1.0, abs(want))
    print("LAPLACE log Z %.12g, from the truth Hessian %.12g: difference %.2e, allowed %.2e" % (logz, want, abs(logz - want), allowed))
    assert abs(logz - want) <= allowed
    exact = 0.5 * d * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(PREC)[1] - np.sum(np.log(widths))
    assert abs(logz - exact) < 0.2, "the surrogate's evidence is near the Gaussian's own"


def test_the_model_is_saved_after_a_laplace_approximation(tmp_path_factory):
    """find_map(method="bfgs-gpu") leaves a device handle and a plan (closures) on the model as working state; neither goes into
    the pickle: ``pickle.dumps`` and ``save()`` work afterwards, the Laplace results travel, and the reloaded model can go on."""
    import os
    import pickle
    sm = _model(tmp_path_factory, "interior", (0.5, -0.3, 0.2))
    sm.laplace_approximation(nRestarts=16)
    assert hasattr(sm, "_map_sampler") and hasattr(sm, "_map_plan")
    back = pickle.loads(pickle.dumps(sm))
    assert not hasattr(back, "_map_sampler") and not hasattr(back, "_map_plan")
    for k in ("map_theta", "map_hessian", "map_cov", "map_cov_scaled", "map_on_bound"):
        assert np.array_equal(getattr(back, k), getattr(sm, k)), k
    assert back.laplace_logz == sm.laplace_logz and back.map_lnprob == sm.map_lnprob and back.map_status == 0
    sm.save()
    assert os.path.getsize(os.path.join(sm.savedir, sm.model_name + ".pkl")) > 0
    assert hasattr(sm, "_map_sampler"), "saving does not take the working state from the live model"
    logz = back.laplace_approximation(nRestarts=16)
    assert abs(logz - sm.laplace_logz) <= 1e-9 * abs(sm.laplace_logz)


def test_run_emcee_takes_the_laplace_covariance(tmp_path_factory):
    from alabi_amd.moves import HMCMove
    sm = _model(tmp_path_factory, "interior", (0.5, -0.3, 0.2))
    sm.laplace_approximation(nRestarts=16)
    sm.run_emcee(nwalkers=12, nsteps=100, min_ess=0, sampler_kwargs={"moves": HMCMove(sm.map_cov_scaled, n_leapfrog=4)})
    assert sm.emcee_sampler.last_path == "hmc" and sm.emcee_samples_full.shape == (100, 12, 3)
    assert 0.3 < sm.acc_frac <= 1.0


def test_a_maximum_on_a_wall_gives_no_covariance(tmp_path_factory):
    sm = _model(tmp_path_factory, "wall", (3.8, -0.3, 0.2))
    with pytest.warns(UserWarning, match="on a wall"):
        logz = sm.laplace_approximation(nRestarts=16)
    assert logz is None and sm.laplace_logz is None and sm.map_cov is None and sm.map_cov_scaled is None
    assert sm.map_on_bound.tolist() == [True, False, False] and sm.map_hessian.shape == (3, 3)
    assert sm.map_theta[0] == 3.0 - 1e-9 * 6.0 or abs(sm.map_theta[0] - 3.0) < 1e-8


def test_host_callables_are_refused(tmp_path_factory):
    sm = _model(tmp_path_factory, "interior", (0.5, -0.3, 0.2))
    with pytest.raises(ValueError, match="needs the fused log-probability"):
        sm.find_map(method="bfgs-gpu", prior_fn=lambda th: 0.0)
