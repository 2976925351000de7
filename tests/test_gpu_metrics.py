"""DeviceKDE (csrc/kde.hip) against scipy.stats.gaussian_kde, and alabi_amd.metrics end to end on the GPU: the reference's
kl_divergence_kde with the same global-stream draws, the batched surrogate path of kl_divergence_integral,
compute_kl_full_parallel over a tree of sample files, and the KL of run_dynesty posteriors as training proceeds."""
import os

import numpy as np
import pytest
import torch
from scipy import stats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "reference_metrics_vectors.npz"))

RULES = [None, "silverman", 0.45, lambda k: 0.7 * k.scotts_factor()]


def _data(rng, d, n):
    A = rng.normal(size=(d, d)) / np.sqrt(d) + np.eye(d)
    return A @ rng.normal(size=(d, n)) + rng.normal(size=(d, 1))


def _queries(rng, X, m, h):
    """Half near samples (within a few bandwidths), half uniform over the data's box."""
    d, n = X.shape
    near = X[:, rng.integers(0, n, m)] + h * rng.normal(size=(d, m))
    lo, hi = X.min(1, keepdims=True), X.max(1, keepdims=True)
    box = lo + (hi - lo) * rng.uniform(size=(d, m))
    return np.where(rng.uniform(size=m) < 0.5, near, box)


def _ref_log(ref, Q):
    """scipy's log-density, through log(pdf) wherever the pdf is a normal number: scipy's logpdf adds its N terms one by one
    in the log domain and is itself off by ~2e-12 at N = 2e5, its pdf by ~5e-14."""
    pdf = ref.pdf(Q)
    with np.errstate(divide="ignore"):
        return np.where(pdf > 1e-250, np.log(pdf), ref.logpdf(Q)), pdf


def _check(ours_log, ours_pdf, ref, Q, idx):
    """logpdf: 1e-12 absolute where logpdf > -200, 1e-13 relative below (the augmented product's error grows as
    eps (|u|^2 + |z|^2), DESIGN.md "Gaussian KDE"); pdf: 1e-12 relative where scipy's pdf is above 1e-250 (same split)."""
    ref_log, ref_pdf = _ref_log(ref, Q[:, idx])
    assert np.all(np.isfinite(ours_log)) and not np.any(np.isnan(ours_pdf))
    err = np.abs(ours_log[idx] - ref_log)
    assert np.all(err <= np.maximum(1e-12, 1e-13 * np.abs(ref_log) * (ref_log < -200))), np.max(err)
    big = ref_pdf > 1e-250
    rel = np.abs(ours_pdf[idx][big] - ref_pdf[big]) / ref_pdf[big]
    tol = np.where(ref_log[big] > -200, 1e-12, 1e-13 * np.abs(ref_log[big]))
    assert np.all(rel <= tol), np.max(rel)


@pytest.mark.parametrize("d", [1, 2, 3, 5, 10, 17, 20])
@pytest.mark.parametrize("n_kind", ["d+2", 37, 4097, 200000])
def test_logpdf_and_pdf_match_scipy(d, n_kind):
    from alabi_amd import DeviceKDE
    n = d + 2 if n_kind == "d+2" else n_kind
    rng = np.random.default_rng(1000 * d + n)
    X = _data(rng, d, n)
    w = rng.uniform(0.05, 1.0, n)
    sub = 24 if n >= 100000 else 80                      # scipy is O(N M d) on one core: compare a subset of large M
    for i, M in enumerate([1, 15, 16, 17, 1000, 65537]):
        bw = RULES[(i + d) % len(RULES)]
        weights = w if i % 2 == 0 else None
        ref = stats.gaussian_kde(X, bw_method=bw, weights=weights)
        kde = DeviceKDE(X, bw_method=bw, weights=weights)
        assert kde.factor == ref.factor and np.array_equal(kde.cho_cov, ref.cho_cov) and kde.log_det == ref.log_det
        Q = _queries(rng, X, M, np.sqrt(np.diag(ref.covariance))[:, None])
        idx = np.arange(M) if M <= sub else np.unique(np.r_[0, M - 1, rng.integers(0, M, sub - 2)])
        _check(kde.logpdf(Q), kde.pdf(Q), ref, Q, idx)


@pytest.mark.parametrize("d", [2, 10])
def test_offset_samples_keep_their_digits(d):
    """Samples 1e4 from the origin: the same accuracy as at the origin (the centring).  Inputs sit on a 2^-30 grid so that
    the shifted values are exact and scipy can be asked about the unshifted set."""
    from alabi_amd import DeviceKDE
    rng = np.random.default_rng(5 + d)
    q = 2.0 ** -30
    X = np.round(_data(rng, d, 5000) / q) * q
    ref = stats.gaussian_kde(X)
    Q = np.round(_queries(rng, X, 300, np.sqrt(np.diag(ref.covariance))[:, None]) / q) * q
    kde = DeviceKDE(X + 1e4)
    assert np.max(np.abs(kde.cho_cov - ref.cho_cov) / np.abs(ref.cho_cov).max()) < 1e-12
    # np.cov of the shifted set rounds differently (~1e-15): give scipy the same bandwidth, so only the centring is compared
    ref.covariance, ref.cho_cov, ref.log_det = kde.covariance, kde.cho_cov, kde.log_det
    ours_log, ref_log = kde.logpdf(Q + 1e4), _ref_log(ref, Q)[0]
    assert np.all(np.abs(ours_log - ref_log) <= np.maximum(1e-12, 1e-13 * np.abs(ref_log) * (ref_log < -200)))


@pytest.mark.parametrize("d", [1, 2, 5, 20])
@pytest.mark.parametrize("weighted", [False, True])
def test_tail_logpdf_is_finite_and_matches_scipy(d, weighted):
    from alabi_amd import DeviceKDE
    rng = np.random.default_rng(77 + d)
    n = 3000
    X = rng.normal(size=(d, n))
    w = rng.uniform(0.1, 1.0, n) if weighted else None
    ref = stats.gaussian_kde(X, weights=w)
    kde = DeviceKDE(X, weights=w)
    dirs = rng.normal(size=(d, 64))
    dirs /= np.linalg.norm(dirs, axis=0)
    r_data = np.linalg.norm(X, axis=0).max()
    h = np.sqrt(np.linalg.eigvalsh(ref.covariance).max())
    far = dirs * (r_data + 40.0 * h * np.linspace(1.0, 3.0, 64))     # >= 40 bandwidths from every sample
    edge = dirs * (r_data + h * np.linspace(30.0, 45.0, 64))         # across the underflow threshold
    Q = np.concatenate([far, edge], axis=1)
    ref_log, ref_pdf = ref.logpdf(Q), ref.pdf(Q)
    assert np.all(ref_pdf[:64] == 0.0) and np.all(np.isfinite(ref_log))
    ours_log, ours_pdf = kde.logpdf(Q), kde.pdf(Q)
    assert np.all(np.isfinite(ours_log))
    assert np.all(ours_pdf[:64] == 0.0)
    assert np.max(np.abs(ours_log - ref_log) / np.abs(ref_log)) < 1e-9


def test_repeatable_bits_padding_and_zero_weights():
    from alabi_amd import DeviceKDE
    rng = np.random.default_rng(3)
    d, n = 4, 1001                                        # not a multiple of 16
    X = rng.normal(size=(d, n))
    w = rng.uniform(0.1, 1.0, n)
    Q = rng.normal(size=(d, 3000)) * 1.5
    kde = DeviceKDE(X, weights=w)
    a, b = kde.logpdf(Q), kde.logpdf(Q)
    assert np.array_equal(a, b)
    assert np.array_equal(kde.pdf(Q), kde.pdf(Q))
    assert DeviceKDE(rng.normal(size=(d, n))).plan(3000) == kde.plan(3000)   # the split depends on the shapes only
    # zero-weight samples far away contribute exactly nothing: same values (to rounding of the bandwidth) as without them,
    # and the same as scipy's, which also treats them as weight 0
    Xz = np.concatenate([X, 50.0 + rng.normal(size=(d, 7))], axis=1)
    wz = np.concatenate([w, np.zeros(7)])
    kz = DeviceKDE(Xz, weights=wz)
    ref = stats.gaussian_kde(Xz, weights=wz)
    lz = kz.logpdf(Q)
    assert np.all(np.isfinite(lz))
    assert np.max(np.abs(lz - a)) < 1e-12
    assert np.max(np.abs(lz[:200] - _ref_log(ref, Q[:, :200])[0])) < 1e-12


def test_device_tensors_in_and_out():
    from alabi_amd import DeviceKDE
    rng = np.random.default_rng(9)
    X = rng.normal(size=(3, 2000))
    Q = rng.normal(size=(3, 500))
    kt = DeviceKDE(torch.as_tensor(X, device="cuda"))
    out = kt.logpdf(torch.as_tensor(Q, device="cuda"))
    assert isinstance(out, torch.Tensor) and out.is_cuda
    ref = stats.gaussian_kde(X)
    assert np.max(np.abs(out.cpu().numpy() - _ref_log(ref, Q)[0])) < 1e-12
    assert np.max(np.abs(kt(Q[:, 0]) - ref(Q[:, 0])) / ref(Q[:, 0])) < 1e-12


def test_kl_divergence_kde_reproduces_reference():
    from alabi_amd import metrics
    np.random.seed(int(G["kde_seed"]))
    kl2 = metrics.kl_divergence_kde(G["kde_p2"], G["kde_q2"])
    assert abs(kl2 - G["kde_kl2"]) / G["kde_kl2"] < 1e-10
    np.random.seed(8)
    kl3 = metrics.kl_divergence_kde(G["kde_p3"], G["kde_q3"], bandwidth=0.3, n_eval=500)
    assert abs(kl3 - G["kde_kl3"]) / G["kde_kl3"] < 1e-10


def _gauss2(theta):
    t = np.asarray(theta, dtype=float).reshape(-1, 2)
    r = t - np.array([0.5, 0.5])
    out = -0.5 * np.sum(r * r, axis=1) / 0.1
    return out if np.ndim(theta) == 2 else float(out[0])


@pytest.fixture(scope="module")
def sm_trained(tmp_path_factory):
    from alabi_amd import SurrogateModel
    sm = SurrogateModel(lnlike_fn=_gauss2, bounds=[(0.0, 1.0), (0.0, 1.0)], savedir=str(tmp_path_factory.mktemp("kl")),
                        verbose=False, random_state=4, cache=False)
    sm.init_samples(ntrain=60)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1)
    return sm


def test_integral_batched_surrogate_equals_row_by_row(sm_trained):
    from alabi_amd import metrics
    sm = sm_trained
    bounds = np.array([[0.0, 1.0], [0.0, 1.0]])
    log_q = lambda x: -0.5 * np.sum((np.atleast_2d(x) - 0.45) ** 2, axis=1)[0] / 0.12  # noqa: E731
    cached = sm.create_cached_surrogate_likelihood()
    for fn in (sm.surrogate_log_likelihood, cached):
        np.random.seed(21)
        batched = metrics.kl_divergence_integral(fn, log_q, bounds, method="mc", n_samples=512)
        np.random.seed(21)
        rows = metrics.kl_divergence_integral(lambda x: fn(x), log_q, bounds, method="mc", n_samples=512)  # noqa: PLW0108
        assert np.all(np.abs(np.array(batched) - np.array(rows)) <= 1e-12 * np.abs(np.array(rows)))


def _narrow2(theta):
    t = np.asarray(theta, dtype=float).reshape(-1, 2)
    r = (t - np.array([0.3, 0.6])) / np.array([0.07, 0.1])
    out = -0.5 * np.sum(r * r, axis=1)
    return out if np.ndim(theta) == 2 else float(out[0])


def test_kl_falls_as_training_proceeds(tmp_path):
    from alabi_amd import SurrogateModel, metrics
    sm = SurrogateModel(lnlike_fn=_narrow2, bounds=[(0.0, 1.0), (0.0, 1.0)], savedir=str(tmp_path), verbose=False,
                        random_state=11, cache=False)
    sm.init_samples(ntrain=4)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1, fit_white_noise=False, white_noise=-6)
    sm.run_dynesty(like_fn="true", mode="static", sampler_kwargs={"seed": 1}, min_ess=4000)
    true = sm.dynesty_samples
    kl = []
    for niter in (0, 20):
        if niter:
            sm.active_train(niter=niter, algorithm="bape", gp_opt_freq=10)
        sm.run_dynesty(mode="static", sampler_kwargs={"seed": 2}, min_ess=4000)
        np.random.seed(0)
        kl.append(metrics.kl_divergence_kde(sm.dynesty_samples, true))
    assert np.all(np.isfinite(kl)) and kl[1] < 0.5 * kl[0], kl


def test_compute_kl_full_parallel_matches_reference_in_one_process(tmp_path, monkeypatch):
    from alabi_amd import metrics
    root = tmp_path
    trials, iters = G["full_trials"], G["full_iters"]
    for t in trials:
        for ii in iters:
            os.makedirs(root / "ex" / "k" / str(t), exist_ok=True)
            np.savez(root / "ex" / "k" / str(t) / f"dynesty_samples_final_surrogate_iter_{ii}.npz", samples=G[f"full_p_{t}_{ii}"])
    np.savez(root / "ex" / "k" / "dynesty_samples_final_true.npz", samples=G["full_q"])
    import multiprocessing
    started = []
    monkeypatch.setattr(multiprocessing.Process, "start", lambda self: started.append(self))
    np.random.seed(int(G["full_seed"]))
    out = metrics.compute_kl_full_parallel(str(root), "ex", "k", trials=trials, iterations=iters, n_jobs=16)
    assert not started
    assert out.shape == G["full_out"].shape == (len(iters), 5)
    assert np.max(np.abs(out - G["full_out"]) / np.abs(G["full_out"])) < 1e-10
