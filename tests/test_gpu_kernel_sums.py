"""Every path that evaluates a kernel sum  amp sum_n alpha_n k(q, x_n)  against the extended-precision sum of the same terms
(tests/kernel_sum_reference.py), through the forward-error bound derived there from each path's own arithmetic: the reference is
~2000 times more precise than the code under test, alpha is the device's own (the solve is not under test), the GP mean is 0.

Training sets: one point (one term: the test of each exponential), a 130-point lattice nine length scales apart (K diagonal to
rounding, alpha > 0: a purely relative bound), make_problem (200, 3, e^-12), (130, 10, e^-8), (193, 20, e^-12) and an
ill-conditioned one (ell^2 = 8: alpha of mixed sign and large magnitude).  Queries: rays from training points out to 56 length
scales (r^2 from 0 through the denormal range of the terms to exact underflow) plus three at 1e3, 1e6, 1e9 length scales, where
the squared-exponential sum must be exactly 0.

Per path (E, c, A) as counted in tests/kernel_sum_reference.py.  Worst err/tol measured on an MI355X: see MEASURED below.
"""
import ctypes as C

import numpy as np
import pytest

import kernel_sum_reference as ksr
from conftest import make_problem

pytestmark = pytest.mark.gpu

MEASURED = """
Worst err/tol over the case grid on an MI355X (gfx950), with c = d + 2 / d + 3 as stated -- no path needed a re-count.  In
brackets the single-term case (N = 1, alpha < 0), where N - 1 = 0 leaves E and c A alone in the bound: the test of each
exponential.
  alabi_kernel_matrix (exp_neg_half)           0.74  [0.43]   bound and error in long double
  predict_mean_rowwise_kernel (exp_neg_half)   0.50  [0.50]
  predict_mean_mfma_kernel, split (tab256)     0.47  [0.47]
  predict_mean_mfma_kernel, unsplit, M ~ 2e5   0.58
  predict_mean_tile_kernel (exp_tab32)         0.57  [0.57]   lattice 0.41, N = 300 split over two workgroups 0.47, d = 40 0.13
  mean returned with the variance              0.50  [0.17, 0.39, 0.42, 0.50 at M = 7, 100, 300, 2085]
  batched fit-predict                          0.67  [0.67]
  alabi_ens_surrogate / alabi_ens_lnprob       0.67 / 0.67  [the same]
  chain rows: half-step, stream, pair kernels (se_pair_terms, exp_direct)   0.41  [0.41]  identical on the three; 94-96 % moved
  chain rows: group kernel (exp2s_tab256)      0.57  [0.57]
  nested prior draws (se_pair_terms)           0.61  [0.41 in the 60-length-scale box, 0.61 in the 6-length-scale one]
  Matern-3/2, Matern-5/2, rational quadratic on the three predict-mean paths:  0.22, 0.27, 0.04
"""

SE = "ExpSquaredKernel"
CASES = ["n1", "lattice", "p200x3", "p130x10", "p193x20", "ill200x3"]


def _training_set(name):
    if name == "n1":
        return np.array([[0.3, -1.1, 2.0]]), np.array([-1.7]), dict(log_white_noise=-12.0, log_amp=0.3, log_M=np.log([2.0, 1.5, 2.6]))
    if name == "lattice":
        h = dict(log_white_noise=-12.0, log_amp=0.3, log_M=np.log([2.0, 1.5, 2.6]))
        X, y = ksr.lattice(130, 3, 9.0, ksr.hyper_fp64(0.3, -12.0, h["log_M"])[2])
        return X, y, h
    N, d, log_wn, ell2 = {"p200x3": (200, 3, -12.0, None), "p130x10": (130, 10, -8.0, None), "p193x20": (193, 20, -12.0, None),
                          "ill200x3": (200, 3, -12.0, 8.0), "p65x3": (65, 3, -12.0, None), "p300x3": (300, 3, -12.0, None),
                          "p130x40": (130, 40, -8.0, None)}[name]
    X, y, h = make_problem(N, d, 11, log_wn=log_wn, ell2=ell2)
    return X, y, h


class Case:
    """One training set with its factorised GP (mean 0), the device's alpha and the references of the query sets asked for."""

    def __init__(self, name, family=SE, log_alpha=1.0):
        from alabi_amd import HipGP
        self.name, self.family, self.log_alpha = name, family, log_alpha
        self.X, self.y, h = _training_set(name)
        self.h = h
        self.d = self.X.shape[1]
        self.amp, self.wn, self.inv_len = ksr.hyper_fp64(h["log_amp"], h["log_white_noise"], h["log_M"])
        self.gp = HipGP(self.d, 0.0, h["log_white_noise"], h["log_amp"], h["log_M"], kernel=family, log_alpha=log_alpha)
        self.gp.compute(self.X)
        self.gp.predict(self.y, self.X[:1], return_cov=False)
        self.alpha = np.array(self.gp._alpha, dtype=np.float64)
        self._refs = {}

    def queries(self, M):
        """M queries, the last three of them the far ones."""
        return ksr.rays(self.X, self.inv_len, M - 3, seed=5)

    def ref(self, M, alpha=None):
        key = (M, None if alpha is None else alpha.tobytes())
        if key not in self._refs:
            Q = self.queries(M)
            keep = np.arange(0, M, ksr.QUERY_STRIDE)
            ref, terms = ksr.kernel_sum(self.X, self.alpha if alpha is None else alpha, self.amp, self.inv_len, Q[keep],
                                        self.family, self.log_alpha)
            self._refs[key] = (Q, keep, ref, terms)
        return self._refs[key]


@pytest.fixture(scope="module")
def cases():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    cache = {}

    def get(name, family=SE, log_alpha=1.0):
        key = (name, family, log_alpha)
        if key not in cache:
            cache[key] = Case(name, family, log_alpha)
        return cache[key]
    return get


def _A(case, Q, form):
    """(c, A) of a path: 'diff', 'dot' (matrix-core kernels) or 'pair' (se_pair_terms)."""
    d, fam = case.d, case.family
    if form == "diff":
        return ksr.c_difference(d, fam), ksr.arg_difference(case.X, case.inv_len, Q, fam, case.log_alpha)
    A = ksr.arg_dot(case.X, case.inv_len, Q, case.alpha if form == "pair" else None)
    if fam == SE:
        return ksr.c_dot(d), A
    # the matrix-core kernels of the other families recover r2 = max(-2 acc, 0) from the dot product: an absolute error
    # 2 c_dot u A_dot of r2 is a relative error |2 f'(r2) / f(r2)| c_dot u A_dot of the term, on top of the family's own count
    r2 = 2.0 * ksr.arg_difference(case.X, case.inv_len, Q, SE)
    if fam == "Matern32Kernel":
        g = 3.0 / (1.0 + np.sqrt(3.0 * r2))
    elif fam == "Matern52Kernel":
        s = np.sqrt(5.0 * r2); g = (5.0 / 3.0) * (1.0 + s) / (1.0 + s + s * s / 3.0)
    else:
        g = 1.0 / (1.0 + 0.5 * r2 / np.exp(case.log_alpha))
    own = ksr.arg_difference(case.X, case.inv_len, Q, fam, case.log_alpha)
    return 1, ksr.c_dot(d) * A * g + ksr.C_FAMILY_OWN[fam] * own


def _check(path, case, got, M, E, form, far_zero=True, alpha=None, rays_only=False):
    """got[M] against the reference of case.queries(M) within tolerance; prints the worst err/tol.  rays_only: got holds the
    M - 3 ray queries alone (a path that cannot take the far ones)."""
    Q, keep, ref, terms = case.ref(M, alpha)
    if rays_only:
        keep = keep[keep < M - 3]
        ref, terms, far_zero = ref[:len(keep)], terms[:len(keep)], False
        got = np.concatenate([np.asarray(got, dtype=np.float64), np.full(3, np.nan)])
    got = np.asarray(got, dtype=np.float64)[keep]
    assert np.all(np.isfinite(got)), path
    c, A = _A(case, Q[keep], form)
    tol = ksr.tolerance(terms, A, E, c, case.alpha if alpha is None else alpha, case.amp)
    err = np.abs(got.astype(ksr.LD) - ref).astype(np.float64)
    worst = float(np.max(err / tol))
    below = float(np.mean(np.abs(ref[:len(ref) - (0 if rays_only else 3)]).astype(np.float64) < 2.0 ** -1022))   # of the ray queries
    print("KSUM %-28s %-9s %-24s M=%-6d worst err/tol %.3f  (ref < 2^-1022: %.0f %%)" % (path, case.name, case.family, M, worst,
                                                                                        100 * below))
    if far_zero and case.family == SE and ksr.QUERY_STRIDE == 1:
        assert np.all(got[-3:] == 0.0), (path, got[-3:])
    if case.family == SE and M >= 100:
        assert below <= 0.25, (path, below)
    assert np.all(err <= tol), (path, case.name, worst, int(np.argmax(err / tol)))
    return worst


# ------------------------------------------------------------------------------------------------------ kernel matrix
@pytest.mark.parametrize("name", ["n1", "p200x3", "p193x20"])
def test_kernel_matrix(cases, name):
    """alabi_kernel_matrix: every element is one term (alpha = 1), so the bound has no summation part."""
    case = cases(name)
    M = 211
    Q = case.queries(M)
    K = case.gp.kernel.get_value(Q, case.X)
    one = np.ones(len(case.X))
    _, terms = ksr.kernel_sum(case.X, one, case.amp, case.inv_len, Q)
    c, A = _A(case, Q, "diff")
    # bound and error in long double: in the denormal tail a double would round both to the 2^-1074 grid.  There the element is
    # fl(amp fl(e)): half a grid unit from the exponential, scaled by amp, and half a unit from the product -- (1 + amp) / 2 units
    # at most, half of the bound's 2^-1074 (1 + amp)
    tol = ksr.tolerance(terms.reshape(-1, 1), A.reshape(-1, 1), ksr.E_EXP_NEG_HALF, c, one[:1], case.amp, dtype=ksr.LD).reshape(terms.shape)
    err = np.abs(K.astype(ksr.LD) - terms)
    below = float(np.mean(np.abs(terms[:-3]).astype(np.float64) < 2.0 ** -1022))
    print("KSUM %-28s %-9s worst err/tol %.3f  (ref < 2^-1022: %.0f %%)" % ("alabi_kernel_matrix", name, float(np.max(err / tol)), 100 * below))
    assert np.all(np.isfinite(K)) and np.all(K[-3:] == 0.0)
    assert below <= 0.25
    assert np.all(err <= tol)


# ------------------------------------------------------------------------------------------------- predict-mean paths
@pytest.mark.parametrize("name", CASES)
def test_predict_mean_rowwise(cases, name):
    """predict_mean_rowwise_kernel (M <= 4096 below the matrix-core threshold): difference form, exp_neg_half."""
    case = cases(name)
    M = 333
    mu = case.gp.predict(case.y, case.queries(M), return_cov=False)
    _check("predict_mean_rowwise", case, mu, M, ksr.E_EXP_NEG_HALF, "diff")


@pytest.mark.parametrize("name", CASES)
def test_predict_mean_matrix_core_split(cases, name, monkeypatch):
    """predict_mean_mfma_kernel with the training points split over parts + mean_combine_kernel: augmented dot product about the
    training mean, exp2s_tab256."""
    monkeypatch.delenv("ALABI_PM_MFMA", raising=False)
    case = cases(name)
    M = 2085
    mu = case.gp.predict(case.y, case.queries(M), return_cov=False)
    _check("predict_mean_mfma(split)", case, mu, M, ksr.E_EXP2S_TAB256, "dot")


def test_predict_mean_matrix_core_unsplit(cases, monkeypatch):
    """Three 256-query workgroups per CU and more: the matrix-core kernel writes mu itself (no parts)."""
    from alabi_amd import _lib
    monkeypatch.delenv("ALABI_PM_MFMA", raising=False)
    n_cu = C.c_int(0)
    _lib.check(_lib.lib().alabi_device_info(C.byref(n_cu), None, None), "alabi_device_info")
    case = cases("p65x3")
    M = 3 * 256 * n_cu.value + 37
    assert M * 65 < 2e7
    mu = case.gp.predict(case.y, case.queries(M), return_cov=False)
    _check("predict_mean_mfma(unsplit)", case, mu, M, ksr.E_EXP2S_TAB256, "dot")


@pytest.mark.parametrize("name", ["n1", "lattice", "p300x3", "p130x40"])
def test_predict_mean_tile(cases, name, monkeypatch):
    """predict_mean_tile_kernel (ALABI_PM_MFMA=0, or d + 2 > 32), M = 5000: the only user of exp_tab32, so the single-term case
    is the test of that exponential (its table, its ln2/32 constants, its denormal tail); N = 300 splits the training points over
    two workgroups per tile; d = 40 runs the widest bucket but one.  Difference form."""
    monkeypatch.setenv("ALABI_PM_MFMA", "0")
    case = cases(name)
    M = 5000
    mu = case.gp.predict(case.y, case.queries(M), return_cov=False)
    _check("predict_mean_tile", case, mu, M, ksr.E_EXP_TAB32, "diff")


@pytest.mark.parametrize("M", [7, 100, 300, 2085])
@pytest.mark.parametrize("name", ["n1", "lattice", "p200x3", "p130x10"])
def test_mean_returned_with_the_variance(cases, name, M):
    """return_var=True: the small-batch kernel (M = 7), the 16-query groups (100, 300) and the K* pre-pass with (300) and without
    (2085) its split.  Difference form, exp_neg_half."""
    case = cases(name)
    mu, _ = case.gp.predict(case.y, case.queries(M), return_var=True)
    _check("mean with variance", case, mu, M, ksr.E_EXP_NEG_HALF, "diff")


@pytest.mark.parametrize("family,log_alpha", [("Matern32Kernel", 1.0), ("Matern52Kernel", 1.0), ("RationalQuadraticKernel", 0.4)])
@pytest.mark.parametrize("name", ["p200x3", "p130x10"])
def test_other_families_on_the_predict_mean_paths(cases, name, family, log_alpha, monkeypatch):
    case = cases(name, family, log_alpha)
    E = ksr.E_FAMILY[family]
    monkeypatch.delenv("ALABI_PM_MFMA", raising=False)
    mu = case.gp.predict(case.y, case.queries(333), return_cov=False)
    _check("predict_mean_rowwise", case, mu, 333, E, "diff")
    mu = case.gp.predict(case.y, case.queries(2085), return_cov=False)
    _check("predict_mean_mfma(split)", case, mu, 2085, E, "dot")
    monkeypatch.setenv("ALABI_PM_MFMA", "0")
    mu = case.gp.predict(case.y, case.queries(5000), return_cov=False)
    _check("predict_mean_tile", case, mu, 5000, E, "diff")


# ------------------------------------------------------------------------------------------------ batched fit-predict
@pytest.mark.parametrize("name", ["n1", "lattice", "p200x3"])
def test_batched_fit_predict(cases, name):
    """gp_batch: one job fits the training rows and predicts the held-out rows in one call; its own alpha is read back."""
    import torch
    from alabi_amd.gp_batch import HipGPBatch
    case = cases(name)
    M, N = 211, len(case.X)
    Q = case.queries(M)
    dev = torch.device("cuda", 0)
    theta = torch.as_tensor(np.ascontiguousarray(np.vstack([case.X, Q])), device=dev)
    yy = torch.as_tensor(np.concatenate([case.y, np.zeros(M)]), device=dev)
    hyper = case.gp.full_hyper()[None, :]
    b = HipGPBatch(case.d)
    ll, status, mu, off = b.fit_predict(theta, yy, hyper, [np.arange(N)], [N + np.arange(M)])
    assert status[0] == 0
    alpha = b.get_alpha(0, N).cpu().numpy()
    _check("gp_batch fit-predict", case, mu.cpu().numpy(), M, ksr.E_EXP_NEG_HALF, "diff", alpha=np.ascontiguousarray(alpha))
    b.close()


# -------------------------------------------------------------------------------------- ensemble and nested samplers
def _box(case, half=60.0):
    c = case.X.mean(axis=0)
    return np.stack([c - half / case.inv_len, c + half / case.inv_len], axis=1)


@pytest.mark.parametrize("name", ["n1", "lattice", "p200x3", "p130x10"])
def test_ensemble_surrogate_and_lnprob(cases, name):
    """alabi_ens_surrogate (any number of points, no box gate) and alabi_ens_lnprob (the walkers): difference form, exp_neg_half."""
    from alabi_amd import EnsembleSampler
    case = cases(name)
    W = 64
    s = EnsembleSampler(W, case.d, case.gp, case.y, _box(case), seed=3, live_dangerously=True)
    M = 211
    _check("alabi_ens_surrogate", case, s.surrogate(case.queries(M)).cpu().numpy(), M, ksr.E_EXP_NEG_HALF, "diff")
    Mw = W + 3
    lp = s.compute_log_prob(case.queries(Mw)[:W]).cpu().numpy()
    assert np.all(np.isfinite(lp))
    _check("alabi_ens_lnprob", case, lp, Mw, ksr.E_EXP_NEG_HALF, "diff", rays_only=True)     # the far queries lie outside the box


ENS_PATHS = {"half-step": ({"ALABI_ENS_STREAM": "0"}, "launch-per-half-step", None, "pair", ksr.E_EXP_DIRECT),
             "stream": ({"ALABI_ENS_STREAM": "1", "ALABI_ENS_PAIR": "0"}, "stream", "single", "pair", ksr.E_EXP_DIRECT),
             "pair": ({"ALABI_ENS_STREAM": "1"}, "stream", "pair", "pair", ksr.E_EXP_DIRECT),
             "group": ({"ALABI_ENS_STREAM": "1", "ALABI_ENS_GROUP": "1"}, "group", None, "dot", ksr.E_EXP2S_TAB256)}


@pytest.mark.parametrize("path", list(ENS_PATHS))
@pytest.mark.parametrize("name", ["n1", "p200x3", "p130x10"])
def test_ensemble_chain_rows(cases, name, path, monkeypatch):
    """Every stored chain row is a (coords, logp) pair: logp must be the reference sum at coords.  Rows still at a walker's start
    carry the value of alabi_ens_lnprob (difference form); every other row the value of the path's own kernel.  The single
    training point is the test of exp_direct inside se_pair_terms (and of the sign bit of h: with one term a sign on the wrong
    lane of the pair flips the result) and of exp2s_tab256 in the group kernel: N - 1 = 0 leaves E alone in the bound."""
    from alabi_amd import EnsembleSampler
    env, want_path, want_variant, form, E = ENS_PATHS[path]
    for k in ("ALABI_ENS_STREAM", "ALABI_ENS_PAIR", "ALABI_ENS_GROUP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = cases(name)
    W, steps = 64, 8
    p0 = case.queries(W + 3)[:W]
    s = EnsembleSampler(W, case.d, case.gp, case.y, _box(case), seed=17, live_dangerously=True)
    s.run_mcmc(p0, steps, skip_initial_state_check=True)
    assert s.last_path == want_path, s.last_path
    if want_variant is not None:
        assert s.last_stream_variant == want_variant
    chain, lp = s.get_chain(), s.get_log_prob()
    assert chain.shape == (steps, W, case.d) and np.all(np.isfinite(lp))
    moved = np.any(chain != p0[None, :, :], axis=2).ravel()
    Q, got = chain.reshape(-1, case.d), lp.ravel()
    ref, terms = ksr.kernel_sum(case.X, case.alpha, case.amp, case.inv_len, Q)
    c0, A0 = _A(case, Q, "diff")
    c1, A1 = _A(case, Q, form)
    tol = np.where(moved, ksr.tolerance(terms, A1, E, c1, case.alpha, case.amp),
                   ksr.tolerance(terms, A0, ksr.E_EXP_NEG_HALF, c0, case.alpha, case.amp))
    err = np.abs(got.astype(ksr.LD) - ref).astype(np.float64)
    print("KSUM %-28s %-9s rows %d moved %.0f %%  worst err/tol %.3f (moved rows %.3f)" % (
        "ensemble " + path, name, len(got), 100 * moved.mean(), np.max(err / tol), np.max((err / tol)[moved], initial=0.0)))
    assert moved.mean() >= 0.25
    assert np.all(err <= tol)


@pytest.mark.parametrize("name,half", [("n1", 60.0), ("n1", 6.0), ("p200x3", 60.0), ("p130x10", 60.0), ("p200x3", 6.0)])
def test_nested_prior_draws(cases, name, half):
    """GPUWalkBackend.prior(call, n): logl of every draw against the reference at the point the kernels evaluated (transform(u)).
    The 60-length-scale box is the ensemble tests'; the 6-length-scale one keeps most draws out of the underflow."""
    from alabi_amd.nested import GPUWalkBackend
    case = cases(name)
    box = _box(case, half)
    b = GPUWalkBackend(case.gp, case.y, box, seed=5, to_theta=lambda u: box[:, 0] + u * (box[:, 1] - box[:, 0]))
    u, logl = b.prior(0, 512)
    Q = b.transform(u)
    assert np.max(np.abs(Q - b.theta(u))) <= 4 * ksr.U * np.max(np.abs(box))
    ref, terms = ksr.kernel_sum(case.X, case.alpha, case.amp, case.inv_len, Q)
    c, A = _A(case, Q, "pair")
    tol = ksr.tolerance(terms, A, ksr.E_EXP_DIRECT, c, case.alpha, case.amp)
    err = np.abs(logl.astype(ksr.LD) - ref).astype(np.float64)
    print("KSUM %-28s %-9s box %.0f worst err/tol %.3f  (ref < 2^-1022: %.0f %%)" % (
        "nested prior", name, half, np.max(err / tol), 100 * np.mean(np.abs(ref).astype(np.float64) < 2.0 ** -1022)))
    assert np.all(np.isfinite(logl)) and np.all(err <= tol)
    b.close()
