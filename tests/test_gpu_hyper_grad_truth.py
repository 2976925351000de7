"""alabi_gp_grad_log_likelihood (csrc/gp_grad.hip: grad_contract_kernel, grad_final_kernel, radial_with_derivative) and the
objective SurrogateModel._opt_gp hands to scipy, against the extended-precision truth of tests/hyper_grad_reference.py (hg).
The gradient is 0.5 tr((alpha alpha^T - K^-1) dK/dp), a difference of two large, nearly equal parts: its error is measured
against S_p = 0.5 sum (|alpha_i alpha_j| + |K^-1_ij|) |dK_ij/dp|, never against |g|.

Criteria (hg's docstring derives every count; tests/test_hyper_grad_reference_host.py shows that LAPACK and NumPy restatements
meet them and that planted defects of 1e-13 .. 1e-10 S_p do not):
  given inputs   solver.get_inverse() runs the kinv_block that grad_contract_kernel consumes, so with the handle's own alpha and
                 K^-1 every entry must lie within hg.given_bound ("device" counts) of hg.contract_given: this isolates gp_grad.hip.
                 Every case, N = 1473 (300 workgroups: grad_final_kernel's strided loop takes a second pass) included, under
                 every source of W: one tile (Npad = 64), the block-recursive inverse, ALABI_WINV_DNC=0, 63 appends.
  end to end     e_gpu <= 10 e_ref + the given-inputs bound per entry, e_ref the error of the NumPy statement W = L^-1,
                 K^-1 = W^T W of the same case; and e_gpu <= hg.first_order_bound.  LAPACK's error is printed beside it.
  frozen         fit_mean / fit_white_noise / fit_amp = False return the bits of the full vector without that entry
  determinism    two calls, and two handles built alike, return the same bits
  objective      the fun and jac that _opt_gp(hyperopt_method="ml") passes to scipy.optimize.minimize, captured: fun is the
                 truth's nll plus gp_utils.regularization_term within sr's first-order bound of the nll; jac is the assembly
                 core.py documents (under uniform_scales the shared slot receives the mean of the length-scale entries, the
                 others are copied by position; plus the regulariser's gradient, its mean under uniform_scales) of the truth
                 gradient, within the end-to-end criterion assembled the same way; not positive definite: 1e25 and zeros.
                 The test builds that assembly by name, with the reference's exchange of the amplitude and nugget slots
                 written out and commented, not with the model's index lists.

Measured on an MI355X: see MEASURED below.
"""
import numpy as np
import pytest

import hyper_grad_cases as hgc
import hyper_grad_reference as hg
import kernel_sum_reference as ksr
import solve_reference as sr
from conftest import make_problem

pytestmark = pytest.mark.gpu

MEASURED = """
An MI355X (gfx950), u = 2^-53.  33 cases with a truth under both builders of W, N = 1473, five append chains, four model
configurations.  No entry of any case missed a criterion: there is no exception to list, and gp_grad.hip was not changed.

  given inputs: worst |g - contract_given| / given_bound       block-recursive W     ALABI_WINV_DNC=0
  grid, Npad = 64 (N = 1, 2, 63, 64)                           0.222 (n2d10 log_wn)  0.222
  grid, N = 65 .. 200                                          0.054 (n65d10 mean)   0.054
  families, rq-lo, rq-hi                                       0.064                 0.064
  dimension buckets d = 1, 7, 17, 33, 64                       0.033                 0.033
  ill, clustered                                               0.015                 0.011
  duplicate, far                                               0.050                 0.029
  fitted                                                       0.020                 0.020
  wide (N = 1473, 300 workgroups)                              0.037                 0.036
  five append chains after 63 appends                          0.051 (n64d3 mean)

  end to end (both builders of W alike to the digits shown)
                     worst e_gpu / (10 e_ref + bound)   worst e_gpu / first-order bound   in units of u S_p, smallest .. largest entry:
                                                                                          e_gpu             W^T W (e_ref)     LAPACK
  grid               0.208 (n65d3 mean)                 0.13 (N = 1)                      0 .. 9.9e4        0 .. 1.4e5        0 .. 1.4e5
  families           0.155 (rq-hi mean)                 1.3e-3                            0.004 .. 6.7e3    0.06 .. 7.7e4     5e-4 .. 7.7e4
  buckets            0.163 (d64 log_wn)                 4.4e-4                            0.004 .. 1.1e3    0.003 .. 1.5e3    0.005 .. 1.5e3
  ill, clustered     0.267 (clustered mean)             2.9e-4                            0.02 .. 1.1e5     0.004 .. 2.8e5    0.01 .. 2.8e5
  duplicate, far     0.056 (duplicate-Matern32 log_M_0) 4.7e-3                            0.17 .. 4.9e4     0.02 .. 3.6e5     0.007 .. 3.6e5
  fitted             0.144 (fitted-n65d3 log_wn)        1.9e-3                            0.002 .. 1.7e7    0.02 .. 3.1e7     0.001 .. 3.1e7
  The large figures are the conditioning, common to every fp64 statement: K is assembled in fp64 before it is factorised, and the
  largest entries of W^T W and of LAPACK agree, the device's are 1.4 to 12 times smaller.  Entry by entry the device is up to
  290 times LAPACK's error where LAPACK's happens to be small (grid, fitted), and on duplicate-Matern32Kernel LAPACK is 300 times
  the W^T W statement in log_M_0 (the errors of W^T W in the two copies of a row cancel there): ratios of the two formulations,
  recorded, not criteria.

  the fit's objective (60 points, d = 3; uniform_scales x regularize; x0 and two vectors in the box)
  fun    error / first-order bound of the nll     <= 6.4e-3
  jac    worst error / (10 e_ref + bound)         <= 0.13;   / first-order bound  <= 0.10
  not positive definite: fun = 1e25 and jac = zeros in all four.  Before this change jac was the regulariser's gradient there
  (8.5e-4 per length scale) while fun was the constant 1e25; _opt_gp now returns zeros.
"""

U = hg.U
ENV = ("ALABI_CHOL_TASKS", "ALABI_CHOL_W8", "ALABI_CHOL_PANEL", "ALABI_CHOL_LOOKAHEAD", "ALABI_TRSV_STREAM", "ALABI_BATCH_QUEUE",
       "ALABI_PV_W", "ALABI_PV_LEGACY", "ALABI_PV_SMALL", "ALABI_WINV_DNC", "ALABI_NO_APPEND")
W_SOURCES = [("default", {}), ("ALABI_WINV_DNC=0", {"ALABI_WINV_DNC": "0"})]
NEEDS_EXTENDED = "np.longdouble is a double here: the truth beyond N = 65 needs the 64-bit significand"


def _params(names):
    return [n if (ksr.EXTENDED or hgc.size(n) <= 65) else pytest.param(n, marks=pytest.mark.skip(reason=NEEDS_EXTENDED)) for n in names]


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = hg.reference(hgc.case(name, make_problem))
        return cache[name]
    return get


def _setenv(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _mk(c, **kw):
    from alabi_amd import HipGP
    h = c["h"]
    return HipGP(c["X"].shape[1], h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=c["family"],
                 log_alpha=c["log_alpha"], **kw)


def _full(c, vec):
    """The handle's vector (the family's entries in the C ABI's order) as the [4 + d] vector of hg, 0 where the family has none."""
    names = hg.entry_names(c["X"].shape[1])
    assert len(vec) == len(c["entries"]), (c["name"], len(vec), c["entries"])
    out = np.zeros(len(names))
    out[[names.index(n) for n in c["entries"]]] = vec
    return out


def _idx(c):
    names = hg.entry_names(c["X"].shape[1])
    return [names.index(n) for n in c["entries"]]


def _check_given(fail, tag, c, g):
    """One handle, computed: its gradient against the contraction of its own alpha and K^-1.  Returns (gradient, bound)."""
    y = c["y"]
    dev = _full(c, g.grad_log_likelihood(y))
    alpha, Kinv = g._alpha.copy(), g.solver.get_inverse()
    assert alpha.shape == (len(y),) and Kinv.shape == (len(y), len(y)) and np.all(np.isfinite(dev))
    bound = hg.given_bound(alpha, Kinv, c, "device")
    r = sr._ratio(hg.error(dev, hg.contract_given(alpha, Kinv, c)), bound)
    idx = _idx(c)
    names = hg.entry_names(c["X"].shape[1])
    i = max(idx, key=lambda k: r[k])
    print("HGRAD %-34s %-18s given inputs: worst error / bound %.3f (%s)" % (c["name"], tag, r[i], names[i]))
    if not np.all(r[idx] <= 1.0):
        fail.append((c["name"], tag, "given inputs", [(names[k], float(r[k])) for k in idx if not r[k] <= 1.0]))
    return dev, bound


@pytest.mark.parametrize("name", _params(hgc.TRUTH_CASES))
def test_gradient_against_truth(torch_gpu, monkeypatch, refs, name):
    """Every case with a truth, under both builders of W: the given-inputs criterion and the end-to-end criteria."""
    ref = refs(name)
    idx = _idx(ref)
    names = hg.entry_names(ref["d"])
    fail = []
    for tag, env in W_SOURCES:
        _setenv(monkeypatch, env)
        g = _mk(ref); g.compute(ref["X"])
        dev, bound = _check_given(fail, tag if ref["N"] > 64 else tag + ", Npad = 64", ref, g)
        e_gpu = hg.error(dev, ref["g"])
        yard = 10.0 * ref["e_ref"] + bound
        r, fo = sr._ratio(e_gpu, yard), sr._ratio(e_gpu, ref["fo_grad"])
        i = max(idx, key=lambda k: r[k])
        uS = U * ref["S"]
        print("HGRAD %-34s %-18s end to end: worst e_gpu / (10 e_ref + bound) %.3f (%s), / first-order bound %.2e; in u S: e_gpu %.3g .. %.3g, "
              "W^T W %.3g .. %.3g, LAPACK %.3g .. %.3g; worst e_gpu / e_lapack %.3g" % (
                  name, tag, r[i], names[i], fo[idx].max(), sr._ratio(e_gpu, uS)[idx].min(), sr._ratio(e_gpu, uS)[idx].max(),
                  sr._ratio(ref["e_ref"], uS)[idx].min(), sr._ratio(ref["e_ref"], uS)[idx].max(),
                  sr._ratio(ref["e_lapack"], uS)[idx].min(), sr._ratio(ref["e_lapack"], uS)[idx].max(),
                  np.max(sr._ratio(e_gpu, ref["e_lapack"])[idx][np.asarray(ref["e_lapack"])[idx] > 0], initial=0.0)))
        if not np.all(r[idx] <= 1.0):
            fail.append((name, tag, "10 e_ref + bound", [(names[k], float(r[k])) for k in idx if not r[k] <= 1.0]))
        if not np.all(fo[idx] <= 1.0):
            fail.append((name, tag, "first-order bound", [(names[k], float(fo[k])) for k in idx if not fo[k] <= 1.0]))
    assert not fail, fail


@pytest.mark.skipif(not ksr.EXTENDED, reason=NEEDS_EXTENDED)
def test_wide_given_inputs(torch_gpu, monkeypatch):
    """N = 1473: 24 block rows, 300 workgroups, so each thread of grad_final_kernel adds a second partial sum."""
    c = hgc.case(hgc.WIDE, make_problem)
    fail = []
    for tag, env in W_SOURCES:
        _setenv(monkeypatch, env)
        g = _mk(c); g.compute(c["X"])
        _check_given(fail, tag, c, g)
    assert not fail, fail


def _chain(c, n0):
    """63 consecutive compute_from appends from n0 rows."""
    X = c["X"]
    g = _mk(c); g.compute(X[:n0])
    for n in range(n0 + 1, n0 + 64):
        g2 = _mk(c); g2.compute_from(g, X[:n]); g = g2
    return g


@pytest.mark.skipif(not ksr.EXTENDED, reason=NEEDS_EXTENDED)
@pytest.mark.parametrize("name,n0", sr.APPEND_CHAINS)
def test_append_chain_given_inputs(torch_gpu, monkeypatch, name, n0):
    """W extended one row at a time by gp_append.hip: the contraction still matches the handle's own alpha and K^-1."""
    c = hgc.case(name, make_problem)
    assert len(c["y"]) == n0 + 63
    fail = []
    _setenv(monkeypatch, {})
    g = _chain(c, n0)
    assert getattr(g, "appended", 0) == 63
    _check_given(fail, "63 appends", c, g)
    assert not fail, fail


@pytest.mark.parametrize("name", ["n65d3", "rq-lo"])
def test_frozen_parameters_same_bits(torch_gpu, monkeypatch, name):
    _setenv(monkeypatch, {})
    c = hgc.case(name, make_problem)
    g = _mk(c); g.compute(c["X"])
    full = g.grad_log_likelihood(c["y"])
    assert len(full) == len(c["entries"])
    for kw, entry in (("fit_mean", "mean"), ("fit_white_noise", "log_wn"), ("fit_amp", "log_amp")):
        gf = _mk(c, **{kw: False}); gf.compute(c["X"])
        part = gf.grad_log_likelihood(c["y"])
        keep = [i for i, n in enumerate(c["entries"]) if n != entry]
        assert len(part) == len(full) - 1 and np.array_equal(part, full[keep]), (name, kw, part, full)
        if c["family"] == "RationalQuadraticKernel":
            assert any("log_alpha" in n for n in gf.get_parameter_names())


@pytest.mark.parametrize("name", ["n200d3", "rq-hi", "d17"])
def test_same_bits_again(torch_gpu, monkeypatch, name):
    _setenv(monkeypatch, {})
    c = hgc.case(name, make_problem)
    g = _mk(c); g.compute(c["X"])
    first = g.grad_log_likelihood(c["y"])
    assert np.array_equal(g.grad_log_likelihood(c["y"]), first)
    g.compute(c["X"])                                    # factorise, solve and contract again
    assert np.array_equal(g.grad_log_likelihood(c["y"]), first)
    g2 = _mk(c); g2.compute(c["X"])
    assert np.array_equal(g2.grad_log_likelihood(c["y"]), first)


# ------------------------------------------------------------------------------------------------ the fit's objective
def _lnlike(theta):
    theta = np.asarray(theta, dtype=np.float64)
    return float(-0.5 * np.sum((theta - np.array([0.3, -0.2, 0.1])) ** 2 / np.array([0.6, 1.1, 0.8])))


def _captured_model(monkeypatch, tmp_path, uniform_scales, regularize):
    """A 60-point, three-parameter model whose ML fit is a stub: scipy.optimize.minimize records fun and jac and returns x0."""
    from scipy.optimize import OptimizeResult
    from alabi_amd import SurrogateModel, core
    got = {}

    def minimize(fun, x0, jac=None, **kw):
        got.update(fun=fun, jac=jac, x0=np.array(x0, dtype=np.float64), kw=kw)
        return OptimizeResult(x=np.array(x0, dtype=np.float64), fun=fun(x0), nit=0, success=True, message="stub")

    monkeypatch.setattr(core.op, "minimize", minimize)
    sm = SurrogateModel(lnlike_fn=_lnlike, bounds=[(-3.0, 3.0)] * 3, savedir=str(tmp_path), verbose=False, random_state=5, cache=False)
    sm.init_samples(ntrain=60, ntest=0)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1, uniform_scales=uniform_scales, regularize=regularize)
    assert callable(got.get("fun")) and callable(got.get("jac")) and got["kw"]["method"] == "l-bfgs-b"
    return sm, got


def _ld(v):
    """A number of the truth as a long double (the mpmath route's rounded)."""
    return v if isinstance(v, hg.LD) else ksr._mp_to_ld(v)


def _case_at(sm, p_opt, tag):
    full = np.asarray(sm.expand_hyperparameter_vector(np.asarray(p_opt, dtype=np.float64)), dtype=np.float64)
    names = list(sm.param_names_full)
    at = lambda key: float(full[[i for i, n in enumerate(names) if n.endswith(key)][0]])  # noqa: E731
    h = dict(mean=at("mean:value"), log_white_noise=at("white_noise:value"), log_amp=at(":log_constant"),
             log_M=np.array([at(":log_M_%d_%d" % (k, k)) for k in range(3)]))
    X, y = np.asarray(sm._theta, dtype=np.float64), np.asarray(sm._y, dtype=np.float64)
    c = dict(name=tag, X=X, y=y, h=h, family="ExpSquaredKernel", log_alpha=1.0, entries=hg.family_entries(3, "ExpSquaredKernel"))
    return c, full


@pytest.mark.parametrize("uniform_scales", [False, True])
@pytest.mark.parametrize("regularize", [False, True])
def test_fit_objective(torch_gpu, monkeypatch, tmp_path, uniform_scales, regularize):
    from alabi_amd import gp_utils
    _setenv(monkeypatch, {})
    sm, got = _captured_model(monkeypatch, tmp_path, uniform_scales, regularize)
    fun, jac, x0 = got["fun"], got["jac"], got["x0"]
    lo, hi = sm.hp_bounds[:, 0].astype(np.float64), sm.hp_bounds[:, 1].astype(np.float64)
    assert len(x0) == len(lo) == (4 if uniform_scales else 6)
    rng = np.random.RandomState(11)
    points = [x0] + [np.clip(x0 + 0.05 * rng.uniform(-1.0, 1.0, len(x0)), lo, hi) for _ in range(2)]
    names_full = list(sm.param_names_full)
    assert [n.split(":")[0] for n in names_full[:3]] == ["mean", "white_noise", "kernel"]      # the C ABI's order without log_alpha
    abi = [0, 1, 2, 4, 5, 6]
    fail = []
    for k, p in enumerate(points):
        tag = "objective uniform=%d reg=%d p%d" % (uniform_scales, regularize, k)
        c, full = _case_at(sm, p, tag)
        ref = hg.reference(c)
        reg = gp_utils.regularization_term(full, [3, 4, 5]) if regularize else 0.0
        f_dev, j_dev = fun(p), np.array(jac(p), dtype=np.float64)
        assert np.array_equal(sm.gp.get_parameter_vector(), full)
        # fun
        want = float(ref["nll_hg"]) + reg
        b_f = ref["fo"][3] + 4.0 * U * (abs(float(ref["nll_hg"])) + abs(reg))
        e_f = abs(float((hg.LD(f_dev) - hg.LD(reg)) - _ld(ref["nll_hg"])))
        # jac: the assembly of core.py applied to the truth, and to the per-entry allowances
        alpha, Kinv = sm.gp._alpha.copy(), sm.gp.solver.get_inverse()
        bound = hg.given_bound(alpha, Kinv, c, "device")
        yard_full, fo_full = (10.0 * ref["e_ref"] + bound)[abi], ref["fo_grad"][abi]
        g_true = -np.array([_ld(v) for v in np.asarray(ref["g"])[abi]], dtype=hg.LD)       # the order of param_names_full
        len_idx = [i for i, n in enumerate(names_full) if ":log_M_" in n]
        assert len_idx == [3, 4, 5]
        rg = gp_utils.regularization_gradient(full, len_idx) if regularize else np.zeros(len(full))

        def assemble(v, with_reg):
            """v in the GP's order (mean, white_noise, log_constant, log_M_0 ..) -> the order scipy sees, slot by NAME."""
            v = np.asarray(v)
            if not uniform_scales:
                return v + rg.astype(v.dtype) if with_reg else v
            opt = list(sm.param_names_optimized)
            assert [n.rsplit(":", 1)[1] for n in opt] == ["value", "log_constant", "value", "log_M"] and opt[0] == "mean:value"
            slot = {key: [i for i, n in enumerate(opt) if n.endswith(key)][0] for key in ("mean:value", ":log_constant", "white_noise:value", ":log_M")}
            out = np.zeros(len(opt), dtype=v.dtype)
            out[slot["mean:value"]] = v[0]
            # KNOWINGLY the reference's: it copies the non-length entries by POSITION from the GP's order (mean, white_noise,
            # log_constant) into scipy's (mean, log_constant, white_noise), so the amplitude's slot holds the nugget's
            # derivative and the reverse (NOTES.md "Likelihood gradient truth", "Left as the reference has it").  When that is
            # put right, exchange the two right-hand sides below.
            out[slot[":log_constant"]] = v[1]
            out[slot["white_noise:value"]] = v[2]
            out[slot[":log_M"]] = np.mean(v[len_idx])
            if with_reg:
                out[slot[":log_M"]] += np.mean(rg[len_idx])
            return out

        want_j = assemble(g_true, True)
        slack = 4.0 * U * (np.abs(assemble(np.abs(g_true), False)).astype(np.float64) + np.abs(assemble(np.zeros(len(full)), True)))
        yard, fo = assemble(yard_full, False) + slack, assemble(fo_full, False) + slack
        e_j = np.abs((j_dev.astype(hg.LD) - want_j).astype(np.float64))
        print("HGRAD %-34s fun: error / first-order bound %.2e; jac: worst error / (10 e_ref + bound) %.3f, / first-order bound %.2e" % (
            tag, e_f / b_f, np.max(sr._ratio(e_j, yard)), np.max(sr._ratio(e_j, fo))))
        if not (np.isfinite(f_dev) and e_f <= b_f):
            fail.append((tag, "fun", f_dev, want, e_f, b_f))
        if not (j_dev.shape == p.shape and np.all(e_j <= yard) and np.all(e_j <= fo)):
            fail.append((tag, "jac", j_dev, np.asarray(want_j, dtype=np.float64), e_j, yard))
    # not positive definite (length scales of e^6 box widths, a nugget of e^-41 amplitudes): the ordinary status, 1e25 and zeros
    bad = x0.copy()
    names_opt = list(sm.param_names_optimized) if uniform_scales else names_full
    for i, n in enumerate(names_opt):
        if "log_M" in n:
            bad[i] = 12.0
        if n == "white_noise:value":
            bad[i] = -40.0
        if n.endswith(":log_constant"):
            bad[i] = 1.0
    assert fun(bad) == 1e25
    assert np.array_equal(jac(bad), np.zeros(len(x0)))
    assert not fail, fail
