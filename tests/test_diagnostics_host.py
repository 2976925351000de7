"""Chain diagnostics (Vehtari et al. 2021) without a GPU: the NumPy model tests/diagnostics_numpy.py against itself (direct
extended-precision sums against its FFT route), against what the statistics are for (a shifted, a scaled, a trending chain; ties;
AR(1) theory), and the product's host path alabi_amd/diagnostics.py against the model."""
import numpy as np
import pytest
from scipy.signal import lfilter

import diagnostics_numpy as dn

KEYS = dn.KEYS


def _ar1(shape, phi, seed):
    return lfilter([1.0], [1.0, -phi], np.random.RandomState(seed).randn(*shape), axis=0)


def _cases():
    base = _ar1((2000, 8), 0.6, 7)
    shifted = base.copy(); shifted[:, :4] += 1.0
    scaled = base.copy(); scaled[:, ::2] *= 3.0
    trend = base + np.linspace(0.0, 2.0, 2000)[:, None]
    ties = np.repeat(base[::4], 4, axis=0)
    return dict(base=base, shifted=shifted, scaled=scaled, trend=trend, ties=ties)


CASES = _cases()


def test_direct_sums_agree_with_the_fft_route():
    """(a) gamma_c(l) as written, in np.longdouble, against the zero-padded FFT.  Bound: a forward and an inverse transform of
    length 2 * 2048 = 2^12 each lose at most ~ log2(length) u of the series' energy (lag 0): 2 * 12 * 2^-53 of lag 0."""
    rng = np.random.RandomState(3)
    x = lfilter([1.0], [1.0, -0.8], rng.randn(1025, 5), axis=0) + 3.0 + rng.randn(1, 5)
    y = dn.split(x, 1)
    a, b = dn.acov_direct(y), dn.acov_fft(y)
    err = np.max(np.abs(a - b) / a[:, :1])
    print("direct vs fft: %.2e of lag 0" % err)
    assert err <= 24 * 2.0 ** -53
    ys = dn.split(x, 2)
    assert ys.shape == (10, 512) and np.array_equal(ys[5], x[513:, 0]) and np.array_equal(ys[0], x[:512, 0])
    e_fft, e_dir = dn.ess(ys), dn.ess(ys, dn.acov_direct)
    assert abs(e_fft - e_dir) <= 1e-12 * e_dir


@pytest.mark.parametrize("name", sorted(CASES))
def test_product_host_path_equals_the_model(name):
    """(b)"""
    from alabi_amd import diagnostics
    x = np.stack([CASES[name], CASES["base"][::-1]], axis=-1)             # [2000, 8, 2]
    got, ref = diagnostics.summary(x), dn.summary(x)
    assert sorted(got) == sorted(KEYS)
    for key in KEYS:
        assert got[key].shape == (2,)
        np.testing.assert_allclose(got[key], ref[key], rtol=1e-12, err_msg=key)
    np.testing.assert_array_equal(diagnostics.rhat(x), got["rhat"])
    for method in ("bulk", "tail", "mean"):
        np.testing.assert_array_equal(diagnostics.ess(x, method=method), got["ess_" + method])
    np.testing.assert_array_equal(diagnostics.mcse_mean(x), got["mcse_mean"])
    with pytest.raises(ValueError):
        diagnostics.ess(x, method="median")
    # 1-D and 2-D inputs are promoted: one walker / one parameter
    one = diagnostics.summary(CASES[name][:, 0])
    np.testing.assert_allclose(one["ess_bulk"], dn.summary(CASES[name][:, :1, None])["ess_bulk"], rtol=1e-12)
    np.testing.assert_allclose(diagnostics.summary(CASES[name])["rhat"], ref["rhat"][:1], rtol=1e-12)


def test_what_the_statistics_say():
    """(c) values in brackets: the model's own figures."""
    base = dn.summary(CASES["base"], detail=True)
    assert base["rhat"][0] < 1.01
    shifted = dn.summary(CASES["shifted"])
    print("shifted rhat %.4f" % shifted["rhat"][0])
    assert shifted["rhat"][0] > 1.05                                       # [1.085]
    scaled = dn.summary(CASES["scaled"], detail=True)
    print("scaled rhat %.4f, unfolded part %.4f" % (scaled["rhat"][0], scaled["rhat_parts"][0, 0]))
    assert scaled["rhat"][0] > 1.1                                         # [1.154]
    assert scaled["rhat_parts"][0, 0] < 1.01                               # [1.001]: why the fold exists
    trend = dn.summary(CASES["trend"])
    y1 = dn.split(CASES["trend"], 1)
    unsplit = max(dn.plain_rhat(dn.rank_z(y1)), dn.plain_rhat(dn.rank_z(np.abs(y1 - np.median(y1)))))
    print("trend split rhat %.4f, unsplit %.4f" % (trend["rhat"][0], unsplit))
    assert trend["rhat"][0] > 1.05                                         # [1.087]
    assert unsplit < 1.01                                                  # [1.0005]: why the split exists


def test_average_ranks_with_ties():
    from scipy.stats import rankdata
    v = dn.split(CASES["ties"]).ravel()
    assert np.unique(v).size == v.size // 4
    np.testing.assert_array_equal(dn.average_ranks(v), rankdata(v, method="average"))
    from alabi_amd import diagnostics
    from scipy.special import ndtri
    z = diagnostics._rank_z_host(dn.split(CASES["ties"]))
    np.testing.assert_array_equal(z.ravel(), ndtri((rankdata(v, method="average") - 0.375) / (v.size + 0.25)))


@pytest.mark.parametrize("phi", [0.6, 0.9])
def test_ess_of_ar1_against_theory(phi):
    """(d) ess_mean / (m n) of an AR(1) chain against (1 - phi) / (1 + phi), 3500 steps x 16 walkers.  The factor: the model's
    figures over seeds 1-3 are 0.2408 / 0.2487 / 0.2496 (phi = 0.6, theory 0.25) and 0.0555 / 0.0506 / 0.0552 (phi = 0.9, theory
    0.0526) -- the largest over the smallest is 1.04 and 1.10; the factor allowed on either side of the theory is 1.2, twice the
    wider spread."""
    theory = (1.0 - phi) / (1.0 + phi)
    for seed in (1, 2, 3):
        x = _ar1((3500, 16), phi, seed)
        s = dn.summary(x)
        ratio = s["ess_mean"][0] / x.size
        print("phi %.1f seed %d: ess_mean / (m n) = %.4f against %.4f" % (phi, seed, ratio, theory))
        assert theory / 1.2 < ratio < theory * 1.2
        assert abs(s["mcse_mean"][0] - s["sd"][0] / np.sqrt(s["ess_mean"][0])) <= 1e-15
        assert abs(s["mean"][0]) < 5.0 * s["mcse_mean"][0]                 # the true mean is 0


@pytest.mark.parametrize("which", ["model", "product"])
def test_edge_cases(which):
    """(e)"""
    if which == "model":
        summary = dn.summary
    else:
        from alabi_amd import diagnostics
        summary = diagnostics.summary
    x = np.stack([CASES["base"], CASES["shifted"], np.full((2000, 8), 2.5)], axis=-1)
    for n_t in (1, 2, 3):
        s = summary(x[:n_t])
        assert all(np.all(np.isnan(s[k])) and s[k].shape == (3,) for k in KEYS)
    s4 = summary(x[:4])
    assert np.all(np.isfinite(s4["ess_mean"]))
    ref = summary(x)
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[1000, 3, 1] = bad
        s = summary(xb)
        for k in KEYS:
            assert np.isnan(s[k][1])
            np.testing.assert_array_equal(s[k][[0, 2]], ref[k][[0, 2]])
    assert np.isnan(ref["rhat"][2]) and ref["mcse_mean"][2] == 0.0 and ref["mean"][2] == 2.5 and ref["sd"][2] == 0.0
    assert ref["ess_mean"][2] == ref["ess_bulk"][2] == ref["ess_tail"][2] == 16 * 1000
    xo = x[:1999]                                                          # odd: the middle step is dropped
    so = summary(xo)
    sd = summary(np.concatenate([xo[:999], xo[1000:]], axis=0))
    for k in KEYS:
        np.testing.assert_array_equal(so[k], sd[k])
