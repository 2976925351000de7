"""Chain diagnostics on the device: alabi_chain_split_stats (alabi_amd/csrc/chain_acf.hip) and alabi_amd/diagnostics.py's device path
against the NumPy model tests/diagnostics_numpy.py; EnsembleSampler.diagnostics and SurrogateModel.mcmc_diagnostics on real chains.

Bounds.
  acov_mean   2e-11 x acov_mean[k][0]: what tests/test_gpu_autocorr.py holds the same transforms to.
  chain_mean, chain_var   a rounding count of acf_moments_kernel's summation tree, u = 2^-53.  A sum of n terms there is: thread i
      adds x[i], x[i + 256], ... in order (ceil(n / 256) - 1 additions), six xor steps across the wave, then the four wave sums
      in order (3): D(n) = ceil(n / 256) + 8 additions on any path from a term to the total, each losing at most u of a partial
      sum that is at most the sum of magnitudes.
        mean = sum / n:  (D + 1) u sum|y| / n                                   (the division is one more rounding)
        var  = sum (y - mean)^2 / (n - 1):  every term carries the subtraction's rounding twice and the multiply's once, the sum
               D, the division one:  (D + 4) u var;  the error delta of the mean itself adds n delta^2 / (n - 1) exactly
               (sum (y - mu) = 0), with delta at its bound above.
      (1 + u)^k - 1 <= 1.01 k u for these k.  Nothing here is fitted to device output; the truth is summed in np.longdouble."""
import functools

import numpy as np
import pytest
from scipy.signal import lfilter

import diagnostics_numpy as dn

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble


def _ar1(n, w, d, phi, seed):
    return lfilter([1.0], [1.0, -phi], np.random.RandomState(seed).randn(n, w, d), axis=0)


def _data(n_t, n_w, n_d):
    rng = np.random.RandomState(n_t % 1000 + n_w)
    return _ar1(n_t, n_w, n_d, 0.8, 5) + 3.0 + rng.randn(1, n_w, n_d)              # offsets: the mean removal matters


def _device_chain(x, stride_factor):
    """x on the device with a step stride of stride_factor * n_w * n_d; the gaps hold NaN."""
    import torch
    n_t, n_w, n_d = x.shape
    buf = torch.full((n_t, stride_factor * n_w * n_d), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :n_w * n_d] = torch.as_tensor(x.reshape(n_t, -1), device="cuda")
    v = buf[:, :n_w * n_d].unflatten(1, (n_w, n_d))
    assert v.stride() == (stride_factor * n_w * n_d, n_d, 1) and v.data_ptr() == buf.data_ptr()
    return v, buf


def _call(xd, n_split, transform=0, par=None, acov=True):
    import torch
    from alabi_amd import _lib
    n_t, n_w, n_d = xd.shape
    m, n = n_split * n_w, n_t // n_split
    mean = torch.full((m, n_d), float("nan"), dtype=torch.float64, device="cuda")
    var = torch.full((m, n_d), float("nan"), dtype=torch.float64, device="cuda")
    g = torch.full((n_d, n), float("nan"), dtype=torch.float64, device="cuda") if acov else None
    pd = None if par is None else torch.as_tensor(par, device="cuda")
    rc = _lib.lib().alabi_chain_split_stats(_lib.ptr(xd), n_t, xd.stride(0), n_w, n_d, n_split, transform, _lib.ptr(pd), _lib.ptr(mean),
                                            _lib.ptr(var), _lib.ptr(g), _lib.current_stream())
    assert rc == _lib.OK
    return mean.cpu().numpy(), var.cpu().numpy(), None if g is None else g.cpu().numpy()


def _transformed(x, transform, par):
    if transform == 1:
        return (x <= par).astype(np.float64)
    if transform == 2:
        return np.abs(x - par)
    return x


def _check_moments(y, mean_k, var_k):
    """y [m, n]: the (split, transformed) chains of one parameter; the device's moments against extended-precision truth."""
    m, n = y.shape
    D = -(-n // 256) + 8
    yl = y.astype(LD)
    mu = yl.sum(axis=1) / n
    var = ((yl - mu[:, None]) ** 2).sum(axis=1) / (n - 1)
    tol_mean = 1.01 * (D + 1) * U * np.abs(y).sum(axis=1) / n
    tol_var = 1.01 * (D + 4) * U * var.astype(np.float64) + n / (n - 1.0) * tol_mean ** 2
    err_mean, err_var = np.abs(mean_k - mu).astype(np.float64), np.abs(var_k - var).astype(np.float64)
    assert np.all(err_mean <= tol_mean), (np.max(err_mean / np.maximum(tol_mean, 1e-300)))
    assert np.all(err_var <= tol_var), (np.max(err_var / np.maximum(tol_var, 1e-300)))


def _check_acov(y, got_k):
    ref = dn.acov_fft(y).mean(axis=0)
    assert np.max(np.abs(got_k - ref)) <= 2e-11 * ref[0]


# ------------------------------------------------------------------------------------------------------ 1. the entry
@pytest.mark.parametrize("n_t,n_w,n_d", [(4, 2, 1), (7, 3, 2), (100, 33, 2), (1025, 40, 3), (4097, 6, 5)])
def test_entry_against_the_model(n_t, n_w, n_d):
    """Both splits, a dense and a strided chain, the three transforms, with and without the autocovariances."""
    x = _data(n_t, n_w, n_d)
    par = 3.0 + 0.25 * np.arange(n_d)
    for stride_factor in (1, 3):
        xd, _keep = _device_chain(x, stride_factor)
        for n_split in (1, 2):
            for transform in (0, 1, 2):
                mean, var, g = _call(xd, n_split, transform, par if transform else None)
                mean_only, var_only, none = _call(xd, n_split, transform, par if transform else None, acov=False)
                assert none is None
                np.testing.assert_array_equal(mean_only, mean)                      # the moments-only route: the same values
                np.testing.assert_array_equal(var_only, var)
                for k in range(n_d):
                    y = dn.split(_transformed(x[:, :, k], transform, par[k]), n_split)
                    _check_moments(y, mean[:, k], var[:, k])
                    if np.all(y == y[:, :1]):                                       # indicator chains that never change: 0 everywhere
                        continue
                    _check_acov(y, g[k])


# ------------------------------------------------------------------------------------------------------ 2. two workspace batches
def test_more_than_one_workspace_batch():
    """(131075, 72, 2) split: 288 series of 2^18 complex points = 4 MiB each against 1 GiB of scratch: two batches."""
    n_t, n_w, n_d = 131075, 72, 2
    x = _data(n_t, n_w, n_d)
    xd, _keep = _device_chain(x, 1)
    mean, var, g = _call(xd, 2)
    for k in range(n_d):
        y = dn.split(x[:, :, k], 2)
        assert y.shape == (144, 65537)
        _check_acov(y, g[k])
        _check_moments(y, mean[:, k], var[:, k])


# ------------------------------------------------------------------------------------------------------ 3. summary end to end
MARGIN = 1e-6


@functools.lru_cache(maxsize=None)
def _summary_case(seed, phi):
    x = lfilter([1.0], [1.0, -phi], np.random.RandomState(seed).randn(2500, 12, 1), axis=0)[500:]
    ref = dn.summary(x, detail=True)
    return x, ref


def _assert_margin(ref):
    """Every examined pair sum, up to and including the first non-positive one, is at least MARGIN from zero in every pass: the
    truncation is a discrete decision that the comparison must not hinge on."""
    for name in ("z", "raw", "ind05", "ind95"):
        for e in ref["pairs"][name]:
            assert e.size and np.min(np.abs(e)) >= MARGIN, name
    assert dn.margin(ref) >= MARGIN


@pytest.mark.parametrize("phi", [0.0, 0.6, 0.9])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_summary_on_a_device_tensor(seed, phi):
    import torch
    from alabi_amd import diagnostics
    x, ref = _summary_case(seed, phi)
    _assert_margin(ref)
    got = diagnostics.summary(torch.as_tensor(x, device="cuda"))
    assert sorted(got) == sorted(dn.KEYS)
    for key in dn.KEYS:
        np.testing.assert_allclose(got[key], ref[key], rtol=1e-8, err_msg=key)
    np.testing.assert_array_equal(diagnostics.ess(torch.as_tensor(x, device="cuda"), method="tail"), got["ess_tail"])


# ------------------------------------------------------------------------------------------------------ 4. ties
def test_ties_on_the_device():
    import torch
    from alabi_amd import diagnostics
    base = lfilter([1.0], [1.0, -0.6], np.random.RandomState(7).randn(2000, 8), axis=0)
    ties = np.repeat(base[::4], 4, axis=0)
    v = dn.split(ties).ravel()
    z, s = diagnostics._rank_z_device(torch.as_tensor(v, device="cuda"))
    np.testing.assert_allclose(z.cpu().numpy(), dn.rank_z(v), rtol=0, atol=1e-14)
    np.testing.assert_array_equal(s.cpu().numpy(), np.sort(v))
    got, ref = diagnostics.summary(torch.as_tensor(ties[:, :, None], device="cuda")), dn.summary(ties)
    np.testing.assert_allclose(got["rhat"], ref["rhat"], rtol=1e-8)
    # the median and the quantiles read from the sorted array are NumPy's
    for p in (0.05, 0.5, 0.95):
        assert float(diagnostics._quantile_sorted(s, p)) == np.quantile(v, p)
    assert float(diagnostics._median_sorted(s)) == np.median(v)


# ------------------------------------------------------------------------------------------------------ 5. a real chain
def _c2_sampler(moves, seed):
    from alabi_amd import EnsembleSampler, HipGP
    from alabi_amd.workloads import make_config
    cfg = make_config("C2")
    h = cfg["hyper"]
    g = HipGP(cfg["d"], h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"]); g.compute(cfg["X"])
    return cfg, EnsembleSampler(cfg["W"], cfg["d"], g, cfg["y"], cfg["bounds"], seed=seed, moves=moves)


@pytest.mark.parametrize("move,nsteps", [("gaussian", 200), ("nuts", 50)])
def test_sampler_diagnostics_on_a_real_chain(move, nsteps):
    from alabi_amd.moves import GaussianMove, NUTSMove
    from alabi_amd.workloads import make_config
    b = make_config("C2")["bounds"]
    cov = (0.1 * (b[:, 1] - b[:, 0])) ** 2
    # the shells' surrogate is steep (log-probabilities of thousands over a length scale of sqrt(3)): a small leapfrog step
    cfg, s = _c2_sampler(GaussianMove(cov) if move == "gaussian" else NUTSMove(1.0, step_size=1e-3, max_depth=4), 3)
    s.run_mcmc(cfg["p0"], nsteps)
    print("%s: acceptance %.3f" % (move, s.acceptance_fraction.mean()))
    moved = np.ptp(s.get_chain(discard=20, thin=3), axis=0) > 0.0
    print("%s: %.3f of the walkers moved in the view" % (move, moved.mean()))
    assert moved.mean() > 0.5                            # W is a variance, not the rounding noise of chains that stand still
    assert s.last_path == ("metropolis" if move == "gaussian" else "nuts")
    view = s.get_chain_device(discard=20, thin=3)
    assert view.is_cuda and view.stride(0) == 3 * cfg["W"] * cfg["d"]                # read in place: no copy is made of this view
    got = s.diagnostics(discard=20, thin=3)
    ref = dn.summary(s.get_chain(discard=20, thin=3), detail=True)
    _assert_margin(ref)
    for key in dn.KEYS:
        np.testing.assert_allclose(got[key], ref[key], rtol=1e-8, err_msg=key)
    memo = s._diag_memo
    again = s.diagnostics(discard=20, thin=3)
    assert s._diag_memo is memo
    for key in dn.KEYS:
        np.testing.assert_array_equal(again[key], got[key])
    np.testing.assert_array_equal(s.get_rhat(discard=20, thin=3), got["rhat"])
    np.testing.assert_array_equal(s.get_ess(method="mean", discard=20, thin=3), got["ess_mean"])
    assert s._diag_memo is memo
    s.diagnostics()
    assert s._diag_memo is not memo


def test_model_mcmc_diagnostics(tmp_path):
    from alabi_amd import SurrogateModel
    from alabi_amd.benchmarks import rosenbrock
    sm = SurrogateModel(lnlike_fn=rosenbrock["fn"], bounds=rosenbrock["bounds"], savedir=str(tmp_path), verbose=False, random_state=0)
    with pytest.raises(AttributeError):
        sm.mcmc_diagnostics()
    sm.init_samples(ntrain=50, ntest=20, sampler="uniform")
    sm.init_gp(kernel="ExpSquaredKernel", fit_amp=True, fit_mean=True, white_noise=-12, hyperopt_method="ml", gp_nopt=1)
    sm.run_emcee(nwalkers=16, nsteps=600, min_ess=0)
    assert not hasattr(sm, "emcee_diagnostics")                                     # run_emcee itself does not call it
    out = sm.mcmc_diagnostics()
    assert out is sm.emcee_diagnostics and sorted(out) == sorted(dn.KEYS)
    full = sm.emcee_samples_full[sm.burn:]                                           # theta coordinates
    ref = dn.summary(full)
    for key in dn.KEYS:
        np.testing.assert_allclose(out[key], ref[key], rtol=1e-6, err_msg=key)      # the scaler's affine map, there and back
    assert np.all(out["rhat"] > 0.99) and np.all(out["ess_bulk"] > 1.0)


# ------------------------------------------------------------------------------------------------------ 6. refusals, NaN
def test_bad_arguments_and_a_planted_nan():
    import torch
    from alabi_amd import _lib, diagnostics
    x = _data(64, 4, 3)
    xd = torch.as_tensor(x, device="cuda")
    m = torch.empty((8, 3), dtype=torch.float64, device="cuda"); v = torch.empty_like(m)
    g = torch.empty((3, 64), dtype=torch.float64, device="cuda")
    par = torch.zeros(3, dtype=torch.float64, device="cuda")
    lib, st = _lib.lib(), _lib.current_stream()

    def rc(n_t=64, stride=12, n_split=2, transform=0, p=None):
        return lib.alabi_chain_split_stats(_lib.ptr(xd), n_t, stride, 4, 3, n_split, transform, _lib.ptr(p), _lib.ptr(m), _lib.ptr(v),
                                           _lib.ptr(g), st)
    assert rc() == _lib.OK
    assert rc(n_split=0) == _lib.BAD_ARG and rc(n_split=3) == _lib.BAD_ARG
    assert rc(n_t=3) == _lib.BAD_ARG and rc(n_t=1, n_split=1) == _lib.BAD_ARG       # chains shorter than 2
    assert rc(stride=11) == _lib.BAD_ARG
    assert rc(transform=3) == _lib.BAD_ARG and rc(transform=-1) == _lib.BAD_ARG
    assert rc(transform=1) == _lib.BAD_ARG and rc(transform=2) == _lib.BAD_ARG      # no par
    assert rc(transform=1, p=par) == _lib.OK
    assert rc(n_t=2 ** 21 + 1, n_split=1) == _lib.BAD_ARG and rc(n_t=2 ** 22 + 2) == _lib.BAD_ARG
    ref = diagnostics.summary(xd)
    xb = xd.clone(); xb[40, 2, 1] = float("nan")
    got = diagnostics.summary(xb)
    for key in dn.KEYS:
        assert np.isnan(got[key][1])
        np.testing.assert_array_equal(got[key][[0, 2]], ref[key][[0, 2]])
    short = diagnostics.summary(xd[:3])
    assert all(np.all(np.isnan(short[key])) for key in dn.KEYS)
    const = diagnostics.summary(torch.full((10, 4, 1), 2.5, dtype=torch.float64, device="cuda"))
    assert np.isnan(const["rhat"][0]) and const["ess_bulk"][0] == const["ess_tail"][0] == const["ess_mean"][0] == 40
    assert const["mcse_mean"][0] == 0.0 and const["mean"][0] == 2.5
