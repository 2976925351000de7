"""Every path that PRODUCES a factor or an alpha -- the launch-per-step, queue, panel and batched factorisations, both triangular
solve kernels, alabi_gp_fit_predict, the batched fit, the append of one row, the two reductions and K^-1 -- against the
extended-precision truth of tests/solve_reference.py (K, its Cholesky factor and the substitutions in 64-bit-significand
arithmetic from the library's own fp64 inputs, computed on the host from the test's inputs).

Criteria (solve_reference's docstring derives every count; tests/test_solve_reference_host.py shows that LAPACK and plain
NumPy restatements meet them and that planted defects of 1e-13 .. 1e-10 do not):
  factor, fresh      |L^ L^T - K|_ij <= allowed_ij element by element, the product in extended precision
  factor, appended   within append_bound (device counts, generic inverse) element by element, and the worst excess over the
                     fresh allowance at most 10 x that of append_numpy on the same chain, plus 1
  alpha              omega <= 10 omega_ref + 16 u (omega_ref: LAPACK's cho_solve on the same case), and |a - a_true| within the
                     first-order bound; solver.solve_path is asserted for every alpha
  reductions         log-determinant and likelihood within their tight bounds GIVEN the device's own factor and alpha, and
                     within the first-order bounds of the truth
  K^-1               inverse_omega <= 10 x that of the NumPy statement W = L^-1, W^T W, plus 16 u; symmetric
  variance           on the 63-append handles, e_gpu <= 10 e_ref + 64 u amp with e_ref the distance of append_numpy's variance
                     (W route; substitution route for ALABI_PV_W=0) from the truth

Measured on an MI355X: see MEASURED below.
"""
import numpy as np
import pytest

import kernel_sum_reference as ksr
import solve_reference as sr
from conftest import make_problem

pytestmark = pytest.mark.gpu

MEASURED = """
An MI355X (gfx950), u = 2^-53.  18 fresh cases (14 of make_problem, three more families, ill, clustered), N = 705, 2 x 6 jobs per
batch mode, five append chains.  No path missed a yardstick: there is no exception to list.

  factor path                          worst |L L^T - K| / allowed       (LAPACK on the same cases: 0.03 .. 0.47)
  ALABI_CHOL_TASKS=0                   0.46  (n128d3)
  queue, ALABI_CHOL_W8 = 1 / 0         0.52 / 0.52  (ill; below three block columns the queue does not run: path "steps")
  alabi_gp_fit_predict                 0.52  (ill)
  N = 705, queue (default)             0.40
  N = 705, ALABI_CHOL_PANEL=4          0.39
  batch, ALABI_BATCH_QUEUE = 1 / 0     0.37 / 0.34
  block of the last factorisation under 63 appends: 0.52, bit-identical before and after

  alpha path                           omega / u       worst omega / (10 omega_ref + 16 u)   worst |a - truth| / first-order bound
  trsv_stream_kernel (default)         0.27 .. 19.2    0.26  (n200d10)                       0.13
  step kernels (ALABI_TRSV_STREAM=0)   0.26 .. 19.2    0.26  (n200d10)                       0.13
  alabi_gp_fit_predict                 0.48 .. 19.2    0.26                                  0.13
  batch, queue = 1 / 0                 1.1 .. 19.1     0.26                                  0.11
  N = 705, stream / steps              5.5 / 4.9       0.11 / 0.10                           7.5e-4
  after 63 appends, stream / steps     4.3 .. 10.3     0.36  (n64d3)                         0.033
  LAPACK's cho_solve on the same cases: 0.66 .. 6.9 u.  The two kernels give the same bits up to two block rows (one
  off-diagonal product) and differ from three on.

  reductions, error / bound            logdet given L^   logdet end to end   nll given L^, a^   nll end to end
  gp_reduce_kernel, fresh handles      0.18              0.13                0.13               0.10          (worst: N = 1)
  alabi_gp_fit_predict                 -                 -                   0.13               0.10
  batch                                -                 -                   0.093              0.084
  after 63 appends                     0.0028            0.0051              0.020              0.0028

  append chain, 63 rows                excess over the FRESH allowance, device / append_numpy    worst error / append bound
  n128d3 from 65                       8.5 / 7.4                                                  0.25
  n128d10 from 65                      0.24 / 0.29                                                0.83
  n64d3 from 1                         3.5 / 11.1                                                 0.29
  ill from 129                         3.4 / 5.8                                                  0.16
  clustered from 65                    337 / 135                                                  0.27
  variance on those handles: e_gpu / (10 e_ref + 64 u amp) 0.03 .. 0.60 (ill), the W route and ALABI_PV_W=0 alike

  get_inverse                          inverse_omega / u, device / NumPy W^T W
  n64d3                                24.8 / 6.6
  n130d3                               11.6 / 33.0
  n128d3 after 63 appends              77.6 / 52.8
"""

U = sr.U
ENV = ("ALABI_CHOL_TASKS", "ALABI_CHOL_W8", "ALABI_CHOL_PANEL", "ALABI_CHOL_LOOKAHEAD", "ALABI_TRSV_STREAM", "ALABI_BATCH_QUEUE",
       "ALABI_PV_W", "ALABI_PV_LEGACY", "ALABI_PV_SMALL", "ALABI_WINV_DNC", "ALABI_NO_APPEND")
CHAINS = dict(sr.APPEND_CHAINS)
FRESH = sr.GRID + sr.FAMILY_CASES + ["ill", "clustered"]
# factor paths: (tag, environment, factor_path expected with and without three block columns)
FACTOR_PATHS = [("steps", {"ALABI_CHOL_TASKS": "0"}, "steps", "steps"),
                ("queue w8", {"ALABI_CHOL_TASKS": "1", "ALABI_CHOL_W8": "1"}, "queue", "steps"),
                ("queue w4", {"ALABI_CHOL_TASKS": "1", "ALABI_CHOL_W8": "0"}, "queue", "steps")]
SOLVE_PATHS = [("stream", {}, "stream"), ("steps", {"ALABI_TRSV_STREAM": "0"}, "steps")]


def _size(name):
    return {"ill": 192, "clustered": 128, "big": 705}.get(name) or int(name.partition("-")[0][1:].split("d")[0])


NEEDS_EXTENDED = "np.longdouble is a double here: the truth beyond N = 65 needs the 64-bit significand"


def _params(names):
    return [n if (ksr.EXTENDED or _size(n) <= 65) else pytest.param(n, marks=pytest.mark.skip(reason=NEEDS_EXTENDED)) for n in names]


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name, sub=None):
        key = (name, sub)
        if key not in cache:
            c = sr.case(name, make_problem)
            if sub is not None:                          # the leading ``sub`` rows of a case (the jobs of the batched fit)
                c = dict(c, name="%s[:%d]" % (name, sub), X=c["X"][:sub], y=c["y"][:sub])
            cache[key] = sr.reference(c, CHAINS.get(name) if sub is None else None)
        return cache[key]
    return get


def _setenv(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _mk(ref):
    from alabi_amd import HipGP
    h = ref["h"]
    return HipGP(ref["d"], h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=ref["family"], log_alpha=ref["log_alpha"])


def _handle_alpha(g, n):
    """alpha of the handle as it stands (after alabi_gp_fit_predict the Python object holds no y of its own)."""
    import torch
    from alabi_amd import _lib
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().alabi_gp_get_alpha(g._handle, _lib.ptr(out), _lib.current_stream()), "alabi_gp_get_alpha")
    return out.cpu().numpy()


def _check_factor(fail, tag, ref, Lh):
    assert Lh.shape == (ref["N"], ref["N"]) and np.all(np.triu(Lh, 1) == 0.0) and np.all(np.isfinite(Lh))
    worst = float(np.max(sr.factor_excess(Lh, ref["K"], ref["allowed"])))
    print("SOLVE %-28s %-26s factor: worst |L L^T - K| / allowed %.3f" % (ref["name"], tag, worst))
    if worst > 1.0:
        fail.append((ref["name"], tag, "factor excess", worst))
    return worst


def _check_alpha(fail, tag, ref, a, fo=None):
    b_alpha = (ref["fo"] if fo is None else fo)[0]
    om = sr.omega(ref["K"], ref["L"], a, ref["r"])
    yard = 10.0 * ref["omega_ref"] + 16.0 * U
    first = float(np.max(sr._ratio(np.abs(a - ref["alpha"].astype(np.float64)), b_alpha)))
    print("SOLVE %-28s %-26s alpha: omega/u %.2f (LAPACK %.2f), %.3f of the yardstick; |a - truth| / first-order bound %.2e" % (
        ref["name"], tag, om / U, ref["omega_ref"] / U, om / yard, first))
    if om > yard:
        fail.append((ref["name"], tag, "omega", om / U, yard / U))
    if not (np.all(np.isfinite(a)) and first <= 1.0):
        fail.append((ref["name"], tag, "alpha first-order bound", first))
    if fo is None and om > sr.omega_first_order(ref["N"]):      # a fresh factor: (3 N + 11) u; an appended one has append_bound instead
        fail.append((ref["name"], tag, "omega first-order bound", om / U))
    return om


def _check_reductions(fail, tag, ref, Lh, a, logdet_gpu, nll_gpu, fo=None):
    _, b_logdet, _, b_nll = ref["fo"] if fo is None else fo
    r = ref["r"]
    e = []
    if logdet_gpu is not None:
        e.append(("logdet given L^", abs(float(logdet_gpu - sr.logdet_given(Lh))) / sr.logdet_bound(Lh)))
        e.append(("logdet end to end", abs(float(logdet_gpu - ref["logdet"])) / b_logdet))
    e.append(("nll given L^, a^", abs(float(nll_gpu - sr.nll_given(Lh, r, a))) / sr.nll_bound(Lh, r, a)))
    e.append(("nll end to end", abs(float(nll_gpu - ref["nll"])) / b_nll))
    print("SOLVE %-28s %-26s reductions, error / bound: %s" % (ref["name"], tag, "  ".join("%s %.3g" % kv for kv in e)))
    for what, v in e:
        if not v <= 1.0:
            fail.append((ref["name"], tag, what, v))


def _solve_and_check(fail, monkeypatch, tag, ref, g, Lh, base_env, fo=None):
    """alpha, log-determinant and likelihood of a computed handle through both solve kernels."""
    for stag, senv, spath in SOLVE_PATHS:
        _setenv(monkeypatch, dict(base_env, **senv))
        g._y_set = False                                 # solve again with this switch
        nll = -g.log_likelihood(ref["y"])
        assert g.solver.solve_path == spath, (ref["name"], tag, stag, g.solver.solve_path)
        a = g._alpha.copy()
        _check_alpha(fail, "%s / solve %s" % (tag, stag), ref, a, fo)
        _check_reductions(fail, "%s / solve %s" % (tag, stag), ref, Lh, a, g.solver.log_determinant, nll, fo)


@pytest.mark.parametrize("name", _params(FRESH))
def test_fresh_factor_solve_and_reductions(torch_gpu, monkeypatch, refs, name):
    ref = refs(name)
    N = ref["N"]
    fail = []
    for tag, env, path3, path12 in FACTOR_PATHS:
        _setenv(monkeypatch, env)
        g = _mk(ref); g.compute(ref["X"])
        assert g.solver.factor_path == (path3 if N > 128 else path12), (name, tag, g.solver.factor_path)
        Lh = g.solver.get_factor().cpu().numpy()
        _check_factor(fail, tag, ref, Lh)
        _solve_and_check(fail, monkeypatch, tag, ref, g, Lh, env)
    # alabi_gp_fit_predict: compute + set_y + likelihood + mean in one call (default switches)
    _setenv(monkeypatch, {})
    import torch
    g = _mk(ref)
    ll, mu = g.fit_predict_device(torch.as_tensor(ref["X"], device="cuda"), torch.as_tensor(ref["y"], device="cuda"),
                                  torch.as_tensor(ref["X"][:1] + 0.01, device="cuda"))
    assert mu is not None and np.isfinite(ll)
    assert g.solver.factor_path == ("queue" if N > 128 else "steps") and g.solver.solve_path == "stream"
    Lh = g.solver.get_factor().cpu().numpy()
    a = _handle_alpha(g, N)
    _check_factor(fail, "fit_predict", ref, Lh)
    _check_alpha(fail, "fit_predict", ref, a)
    _check_reductions(fail, "fit_predict", ref, Lh, a, None, -ll)
    assert not fail, fail


@pytest.mark.skipif(not ksr.EXTENDED, reason=NEEDS_EXTENDED)
def test_eleven_block_rows(torch_gpu, monkeypatch, refs):
    """N = 705, d = 6: eleven workgroups on the hand-off chain of the dataflow solve; the default queue factor and the panel
    factor (the only two extended-precision products at this size), both solves on the default factor."""
    ref = refs("big")
    fail = []
    _setenv(monkeypatch, {})
    g = _mk(ref); g.compute(ref["X"])
    assert g.solver.factor_path == "queue"
    Lh = g.solver.get_factor().cpu().numpy()
    _check_factor(fail, "queue (default)", ref, Lh)
    _solve_and_check(fail, monkeypatch, "queue (default)", ref, g, Lh, {})
    _setenv(monkeypatch, {"ALABI_CHOL_TASKS": "0", "ALABI_CHOL_PANEL": "4"})
    g = _mk(ref); g.compute(ref["X"])
    assert g.solver.factor_path == "steps"
    _check_factor(fail, "panel 4", ref, g.solver.get_factor().cpu().numpy())
    assert not fail, fail


BATCH_SIZES = (1, 63, 64, 65, 129, 200)


@pytest.mark.skipif(not ksr.EXTENDED, reason=NEEDS_EXTENDED)
@pytest.mark.parametrize("name", ["n200d3", "n200d10"])
def test_batched_fit(torch_gpu, monkeypatch, refs, name):
    """One fit_predict call holds jobs of 1, 63, 64, 65, 129 and 200 rows (the leading rows of one table, one set of
    hyper-parameters), with the batched queue and with the launch-per-step factorisation per matrix."""
    import torch
    from alabi_amd.gp_batch import HipGPBatch
    full = refs(name)
    d, h = full["d"], full["h"]
    Xd, yd = torch.as_tensor(full["X"], device="cuda"), torch.as_tensor(full["y"], device="cuda")
    hyper = np.tile(np.r_[h["mean"], h["log_white_noise"], h["log_amp"], 1.0, h["log_M"]], (len(BATCH_SIZES), 1))
    train = [np.arange(n) for n in BATCH_SIZES]
    val = [np.array([198, 199]) for _ in BATCH_SIZES]
    fail = []
    for mode in ("1", "0"):
        _setenv(monkeypatch, {"ALABI_BATCH_QUEUE": mode})
        bt = HipGPBatch(d)
        ll, status, mu, off = bt.fit_predict(Xd, yd, hyper, train, val)
        assert bt.timeouts == 0 and np.all(status == 0) and np.all(np.isfinite(ll))
        for b, n in enumerate(BATCH_SIZES):
            ref = refs(name, n) if n < full["N"] else full
            tag = "batch queue=%s" % mode
            Lh = bt.get_factor(b, n).cpu().numpy()
            a = bt.get_alpha(b, n).cpu().numpy()
            _check_factor(fail, tag, ref, Lh)
            _check_alpha(fail, tag, ref, a)
            _check_reductions(fail, tag, ref, Lh, a, None, -ll[b])
        bt.close()
    assert not fail, fail


def _queries(X, inv_len, seed, M=100):
    """Half uniform in the box, a quarter within 1e-3 length scales of training points, a quarter outside the data."""
    rng = np.random.RandomState(seed)
    N, d = X.shape
    kind = np.arange(M) % 4
    Q = rng.uniform(-3.0, 3.0, (M, d))
    near = X[rng.randint(0, N, M)] + 1e-3 * rng.uniform(-1.0, 1.0, (M, d)) / inv_len[None, :] / np.sqrt(d)
    out = rng.uniform(3.0, 4.5, (M, d)) * rng.choice([-1.0, 1.0], (M, d))
    Q[kind == 2] = near[kind == 2]
    Q[kind == 3] = out[kind == 3]
    return Q


def _chain(ref, n0):
    """63 consecutive compute_from appends from n0 rows; returns (handle object, factor before the first append)."""
    X = ref["X"]
    g = _mk(ref); g.compute(X[:n0])
    L0 = g.solver.get_factor().cpu().numpy()
    for n in range(n0 + 1, n0 + 64):
        g2 = _mk(ref); g2.compute_from(g, X[:n]); g = g2
    return g, L0


@pytest.mark.skipif(not ksr.EXTENDED, reason=NEEDS_EXTENDED)
@pytest.mark.parametrize("name,n0", sr.APPEND_CHAINS)
def test_append_chain(torch_gpu, monkeypatch, refs, name, n0):
    from alabi_amd import _lib
    import torch
    ref = refs(name)
    N, X, y, amp, K = ref["N"], ref["X"], ref["y"], ref["amp"], ref["K"]
    assert N == n0 + 63
    fail = []
    _setenv(monkeypatch, {})
    g, L0 = _chain(ref, n0)
    assert getattr(g, "appended", 0) == 63
    Lh = g.solver.get_factor().cpu().numpy()
    assert np.all(np.triu(Lh, 1) == 0.0) and np.all(np.isfinite(Lh))
    assert np.array_equal(Lh[:n0, :n0], L0)                                # nothing moves
    # the factor: the block of the last factorisation to the fresh allowance, the appended rows to the append bound
    res = np.abs(sr.factor_residual(Lh, K))
    ex = res / ref["allowed"]
    ex_np = np.abs(sr.factor_residual(ref["L_app"], K)) / ref["allowed"]
    G = ref["G_device_generic"]
    worst_fresh, worst_app, worst_np, worst_G = ex[:n0, :n0].max(), ex[n0:].max(), ex_np[n0:].max(), (res / G)[n0:].max()
    print("SOLVE %-28s append chain from %d: fresh block excess %.3f; appended rows: excess over the fresh allowance %.2f "
          "(append_numpy %.2f), worst error / append bound %.3f" % (name, n0, worst_fresh, worst_app, worst_np, worst_G))
    if worst_fresh > 1.0:
        fail.append((name, "fresh block", worst_fresh))
    if not np.all(res <= G):
        fail.append((name, "append bound", worst_G))
    if worst_app > 10.0 * worst_np + 1.0:
        fail.append((name, "appended rows against append_numpy", worst_app, worst_np))
    # alpha and the reductions of the appended handle, both solve kernels; first-order bounds with the append bound for dK
    _solve_and_check(fail, monkeypatch, "63 appends", ref, g, Lh, {}, ref["fo_app"])
    # the variance, W route and substitution route, against append_numpy's own distance from the truth
    Q = _queries(X, ref["inv_len"], N + n0)
    ks = ksr.cross_matrix(X, amp, ref["inv_len"], Q)
    truth = ksr.variance(ref["L"], ks, amp)
    ks64 = sr.kernel_fp64(X, Q, amp, ref["inv_len"])
    v_w = ref["W_app"] @ ks64
    from scipy.linalg import solve_triangular
    v_s = solve_triangular(ref["L_app"], ks64, lower=True)
    for tag, env, v in (("ALABI_PV_W unset", {}, v_w), ("ALABI_PV_W=0", {"ALABI_PV_W": "0"}, v_s)):
        _setenv(monkeypatch, env)
        var = g.predict(y, Q, return_var=True)[1]
        e_ref = float(np.max(np.abs((amp - np.sum(v * v, axis=0)) - truth)))
        e_gpu = float(np.max(np.abs(var - truth)))
        bound = 10.0 * e_ref + 64.0 * U * amp
        print("SOLVE %-28s variance %-18s e_ref/amp %.2e  e_gpu/amp %.2e  e_gpu/bound %.3f" % (name, tag, e_ref / amp, e_gpu / amp, e_gpu / bound))
        if not (np.all(np.isfinite(var)) and e_gpu <= bound):
            fail.append((name, "variance " + tag, e_ref / amp, e_gpu / amp))
    _setenv(monkeypatch, {})
    if name == "n128d3":
        # K^-1 of the appended handle against the statement's W^T W
        Kinv = g.solver.get_inverse()
        assert np.array_equal(Kinv, Kinv.T)
        io, io_np = sr.inverse_omega(K, ref["L"], Kinv), sr.inverse_omega(K, ref["L"], ref["W_app"].T @ ref["W_app"])
        print("SOLVE %-28s get_inverse after 63 appends: inverse_omega/u %.2f (W^T W of append_numpy %.2f)" % (name, io / U, io_np / U))
        if io > 10.0 * io_np + 16.0 * U:
            fail.append((name, "inverse_omega", io / U, io_np / U))
    if N % 64 == 0:
        # no padding row left: the library refuses the append, and compute_from refits
        x_new = torch.as_tensor(np.random.RandomState(N).uniform(-3.0, 3.0, ref["d"]), device="cuda")
        assert _lib.lib().alabi_gp_append(g._handle, _lib.ptr(x_new), _lib.current_stream()) == _lib.BAD_ARG
        X1 = np.vstack([X, x_new.cpu().numpy()[None, :]])
        g2 = _mk(ref); g2.compute_from(g, X1)
        assert getattr(g2, "appended", 0) == 0 and g2._n == N + 1 and g2.solver.factor_path == ("queue" if N + 1 > 128 else "steps")
    assert not fail, fail


@pytest.mark.skipif(not ksr.EXTENDED, reason=NEEDS_EXTENDED)
@pytest.mark.parametrize("name", ["n64d3", "n130d3"])
def test_get_inverse(torch_gpu, monkeypatch, refs, name):
    ref = refs(name)
    _setenv(monkeypatch, {})
    g = _mk(ref); g.compute(ref["X"])
    Kinv = g.solver.get_inverse()
    assert Kinv.shape == (ref["N"], ref["N"]) and np.array_equal(Kinv, Kinv.T)
    W = sr.lower_inverse_fp64(ref["L_lapack"])
    io, io_np = sr.inverse_omega(ref["K"], ref["L"], Kinv), sr.inverse_omega(ref["K"], ref["L"], W.T @ W)
    print("SOLVE %-28s get_inverse: inverse_omega/u %.2f (NumPy W^T W %.2f)" % (name, io / U, io_np / U))
    assert io <= 10.0 * io_np + 16.0 * U
