"""alabi_amd.laplace on the host: the evidence of an exact Gaussian, the changes of coordinates, a Hessian that is not negative
definite."""
import numpy as np
import pytest

from alabi_amd import laplace as lap


def _spd(d, seed):
    rs = np.random.RandomState(seed)
    A = rs.randn(d, d)
    return A @ A.T + d * np.eye(d)


@pytest.mark.parametrize("d", [1, 3, 10])
def test_log_evidence_of_an_exact_gaussian(d):
    """log-density = ln c - (x - m)^T P (x - m) / 2 has the integral c (2 pi)^(d/2) det(P)^(-1/2) exactly; with uniform-prior
    coordinates of widths w the estimate subtracts sum ln w."""
    P = _spd(d, d)
    lnc = -1.7 + 0.3 * d
    want = lnc + 0.5 * d * np.log(2.0 * np.pi) - 0.5 * np.linalg.slogdet(P)[1]
    assert abs(lap.laplace_log_evidence(lnc, -P) - want) <= 1e-12 * max(1.0, abs(want))
    w = np.linspace(0.5, 6.0, d)
    got = lap.laplace_log_evidence(lnc, -P, w)
    assert abs(got - (want - np.sum(np.log(w)))) <= 1e-12 * max(1.0, abs(want))
    cov = lap.laplace_covariance(-P)
    assert np.allclose(cov @ P, np.eye(d), rtol=0, atol=1e-12) and np.array_equal(cov, cov.T)


def test_coordinate_changes_round_trip():
    d = 5
    H = -_spd(d, 2)
    t = np.array([2.0, -0.5, 1.0, 1e3, 0.25])
    Ht = lap.hessian_to_theta(H, t)
    assert np.allclose(lap.hessian_to_scaled(Ht, t), H, rtol=1e-15, atol=0)
    cov = lap.laplace_covariance(H)
    cov_t = lap.covariance_to_theta(cov, t)
    assert np.allclose(lap.covariance_to_scaled(cov_t, t), cov, rtol=1e-15, atol=0)
    # the two frames describe one Gaussian: cov_theta is the inverse of -H_theta, and the quadratic form is the same number
    assert np.allclose(cov_t @ (-Ht), np.eye(d), rtol=0, atol=1e-10)
    dth = np.random.RandomState(0).randn(d)
    assert np.isclose(dth @ Ht @ dth, (t * dth) @ H @ (t * dth), rtol=1e-13)
    # the evidence in theta: ln det(-H_theta) = ln det(-H_c) + 2 sum ln|t|
    a, b = lap.laplace_log_evidence(0.0, Ht), lap.laplace_log_evidence(0.0, H)
    assert np.isclose(a, b - np.sum(np.log(np.abs(t))), rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        lap.hessian_to_theta(H, t[:3])
    with pytest.raises(ValueError):
        lap.hessian_to_theta(H, np.zeros(d))


def test_a_hessian_that_is_not_negative_definite_gives_none():
    H = -_spd(4, 3)
    H[2, 2] = 5.0                                     # a direction of ascent: a saddle
    assert lap.laplace_covariance(H) is None and lap.laplace_log_evidence(1.0, H) is None
    Z = -_spd(3, 1); Z[0, 1] = np.nan
    assert lap.laplace_covariance(Z) is None and lap.laplace_log_evidence(1.0, Z) is None
    assert lap.laplace_covariance(np.zeros((2, 2))) is None


def test_working_state_of_the_device_search_stays_out_of_the_pickle(tmp_path):
    """find_map(method="bfgs-gpu") leaves its sampler (a device handle) and its PosteriorPlan (local closures of plan_ensemble) on
    the model for laplace_approximation; ``__getstate__`` drops both, so ``save()`` -- which active_train and run_emcee call --
    keeps working.  No GPU: the plan is a real one (with a host likelihood, which needs no scalers), the sampler a stand-in that cannot be pickled either."""
    import pickle

    from alabi_amd import SurrogateModel
    from alabi_amd import posterior as post
    from alabi_amd.benchmarks import rosenbrock
    sm = SurrogateModel(lnlike_fn=rosenbrock["fn"], bounds=rosenbrock["bounds"], savedir=str(tmp_path), verbose=False, random_state=0)
    pickle.dumps(sm)
    sm._map_plan = post.plan_ensemble(rosenbrock["fn"], sm.surrogate_log_likelihood, None, sm.bounds, None, None, None)
    sm._map_sampler = lambda: None
    sm.map_cov_scaled = np.eye(2)
    with pytest.raises(Exception):
        pickle.dumps(sm._map_plan)
    back = pickle.loads(pickle.dumps(sm))
    assert not hasattr(back, "_map_plan") and not hasattr(back, "_map_sampler") and np.array_equal(back.map_cov_scaled, np.eye(2))
    sm.save()
    assert hasattr(sm, "_map_plan") and hasattr(sm, "_map_sampler")
