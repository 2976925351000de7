"""Every way the library produces a Cholesky pivot must report a matrix that is not positive definite with LAPACK's ``info``: the
1-based index of the FIRST pivot that is not > 0 (NaN included), read through alabi_gp_last_pivot / the status array of the batch.

Paths (csrc/gp_cholesky.hip with its kernels in csrc/chol_steps.hpp and csrc/chol_queue.hpp, csrc/gp_append.hip): launch per step
with rank-64 updates; 2/4/8-column panels with and without look-ahead; the one-launch task queue with four and eight waves and its grouped-update shapes; the batched queue and its
launch-per-step fallback; the rank-1 append.  None of them tests a pivot inside the recurrence: a bad pivot turns its own and
every later column into NaN and the finished tile's diagonal is searched (potrf_first_bad), the first report wins through
atomicCAS(info, 0, kb * 64 + bad).

Inputs and reference: tests/notpd_numpy.py -- (a) a NaN / +inf / -inf coordinate in training row p, (b) two rows at one far
point with unit amplitude and no nugget, whose pivot is an exact 1 - 1 = 0.  Both fail at pivot p + 1 by netlib's dpotf2 rule
(test_not_pd_host.py checks that, and LAPACK's agreement on the finite case, on the oracle's matrix).  At the large sizes here
the expectation follows from two facts: the healthy K factors under LAPACK's dpotrf (``_problem`` checks it once per size, family
and hyper-parameter set), hence so does every leading minor, and pivot p is NaN or an exact zero.  Every assertion on an index is an
equality.

Finding, construction (b): it agrees with (a) on every path -- pivot_rsqrt(1.0) is exactly 1 and the exact zeros stay exact
through the panel solves and the matrix-core updates, so no exception to the equality was needed.
Finding, append: a rejected point used to be left in the padding column Xt[:, N] of the scaled training set, and the mean kernels
multiply that column by alpha = 0 instead of masking it -- a rejected NaN point made every later mean prediction of the "untouched"
factor NaN.  append_pivot_kernel now writes the column only once the pivot has passed (test_rejected_append_leaves_the_factor_alone)."""
import numpy as np
import pytest

from conftest import make_problem
from notpd_numpy import healthy_factors, nonfinite_row, ones_block, ones_hyper, ones_pairs, positions
from test_gpu_batch import _jobs

pytestmark = pytest.mark.gpu

D = 6
RQ_ALPHA = 0.4
CHOL_ENV = ("ALABI_CHOL_TASKS", "ALABI_CHOL_PANEL", "ALABI_CHOL_LOOKAHEAD", "ALABI_CHOL_W8", "ALABI_CHOL_UPDATE2", "ALABI_CHOL_UPDATE4",
            "ALABI_CHOL_SPIN_LIMIT")
MAX_REPORT = 6                               # discrepancies listed before a failing test stops trying further positions


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


_PROBLEMS = {}


def _problem(N, kernel="ExpSquaredKernel", ones=False):
    """(X, y, hyper) of size N with the premise of ``p + 1`` checked once: LAPACK factors the healthy matrix."""
    key = (N, kernel, ones)
    if key not in _PROBLEMS:
        from oracle.gp_oracle import OracleGP
        X, y, h = make_problem(N, D, 70 + N)
        if ones:
            h = ones_hyper(h)
        K = OracleGP(D, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel, log_alpha=RQ_ALPHA).get_matrix(X)
        assert healthy_factors(K), key
        _PROBLEMS[key] = (X, y, h)
    return _PROBLEMS[key]


def _gp(h, kernel="ExpSquaredKernel"):
    from alabi_amd import HipGP
    return HipGP(D, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel, log_alpha=RQ_ALPHA)


def _check_failure(g, Xb, y, want, path, tag, bad):
    """One failing compute on the handle of ``g``: NOT_PD (HipGP turns exactly that status into LinAlgError), index == want from
    alabi_gp_last_pivot and in the message, the forced path, and log_likelihood(quiet=True) == -inf (a second factorisation of the
    same matrix on the same handle, which must report the same index)."""
    try:
        g.compute(Xb)
        bad.append((tag, "no LinAlgError", g.last_pivot))
        return
    except np.linalg.LinAlgError as e:
        msg = str(e)
    if g.last_pivot != want:
        bad.append((tag, "last_pivot", g.last_pivot, "want", want))
    if msg != f"{want}-th leading minor of the array is not positive definite":
        bad.append((tag, "message", msg))
    if path is not None and g.solver.factor_path != path:
        bad.append((tag, "factor_path", g.solver.factor_path))
    ll = g.log_likelihood(y, quiet=True)
    if not (ll == -np.inf):
        bad.append((tag, "log_likelihood", ll))
    if g.last_pivot != want or (path is not None and g.solver.factor_path != path):
        bad.append((tag, "second factorisation", g.last_pivot, g.solver.factor_path))


def _check_fit_predict(torch, g, Xb, y, want, path, tag, bad):
    dev = torch.device("cuda")
    ll, mu = g.fit_predict_device(torch.as_tensor(Xb, device=dev), torch.as_tensor(y, device=dev), torch.as_tensor(Xb[:5] * 0.5, device=dev))
    if not (ll == -np.inf and mu is None and g.last_pivot == want and (path is None or g.solver.factor_path == path)):
        bad.append((tag, "fit_predict", ll, g.last_pivot, g.solver.factor_path))


def _inf_positions(N):
    pos = positions(N)
    return sorted({pos[0], 17 if N > 17 else pos[1], pos[len(pos) // 2], 64 * ((N - 1) // 64), N - 1})


def _run_cases(torch, N, path):
    """Constructions (a) and (b) at every position class of size N on one handle each (so every failure also follows another
    failure at a different pivot); returns the discrepancies."""
    X, y, h = _problem(N)
    _, _, h1 = _problem(N, ones=True)
    g, g1 = _gp(h), _gp(h1)
    bad = []
    for p in positions(N):
        _check_failure(g, nonfinite_row(X, p, np.nan, p % D), y, p + 1, path, ("nan", p), bad)
        if len(bad) >= MAX_REPORT:
            return bad
    for p in _inf_positions(N):
        for v in (np.inf, -np.inf):
            _check_failure(g, nonfinite_row(X, p, v, (p + 1) % D), y, p + 1, path, (str(v), p), bad)
        if len(bad) >= MAX_REPORT:
            return bad
    for q, p in ones_pairs(N):
        _check_failure(g1, ones_block(X, q, p), y, p + 1, path, ("ones", q, p), bad)
        if len(bad) >= MAX_REPORT:
            return bad
    pos = positions(N)
    for p in (pos[len(pos) // 3], pos[-1]):
        _check_fit_predict(torch, g, nonfinite_row(X, p, np.nan, 0), y, p + 1, path, ("nan", p), bad)
    q, p = ones_pairs(N)[-1]
    _check_fit_predict(torch, g1, ones_block(X, q, p), y, p + 1, path, ("ones", q, p), bad)
    return bad


def _clear_env(monkeypatch):
    for k in CHOL_ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("N", [70, 705, 1100, 2900])
@pytest.mark.parametrize("lookahead", ["0", "1"])
@pytest.mark.parametrize("panel", ["0", "2", "4", "8"])
def test_steps_path_reports_lapack_info(torch_gpu, monkeypatch, panel, lookahead, N):
    """Launch per step: rank-64 updates (panel 0) and 2/4/8-column panels, serial and with look-ahead.  The first tile is
    factorised by potrf_diag_kernel, the later ones by potrf_tile_lds_wg inside the update / panel kernels."""
    _clear_env(monkeypatch)
    monkeypatch.setenv("ALABI_CHOL_TASKS", "0")
    monkeypatch.setenv("ALABI_CHOL_PANEL", panel)
    monkeypatch.setenv("ALABI_CHOL_LOOKAHEAD", lookahead)
    bad = _run_cases(torch_gpu, N, "steps")
    assert bad == []


@pytest.mark.parametrize("N", [130, 705, 2000, 4096, 5200])
@pytest.mark.parametrize("w8", ["0", "1"])
def test_queue_path_reports_lapack_info(torch_gpu, monkeypatch, w8, N):
    """The one-launch task queue (ct_potrf_publish), four and eight waves: NaN tiles travel through the versioned hand-offs and the
    tag-validated slab buffers, whose "not written yet" marker is itself a NaN pattern.  factor_path must stay "queue": a
    "queue-timeout" would mean a waiter took a poisoned tile for an unwritten one.  N = 4096 has no padding row."""
    _clear_env(monkeypatch)
    monkeypatch.setenv("ALABI_CHOL_TASKS", "1")
    monkeypatch.setenv("ALABI_CHOL_W8", w8)
    bad = _run_cases(torch_gpu, N, "queue")
    assert bad == []


@pytest.mark.parametrize("w8,two,four", [("0", "1", "0"), ("1", "0", "0"), ("1", "1", "0"), ("1", "1", "1")])
def test_queue_update_shapes_report_lapack_info(torch_gpu, monkeypatch, w8, two, four):
    """The grouped-update shapes of test_cholesky_task_queue_four_and_eight_waves_same_bits at N = 2000."""
    _clear_env(monkeypatch)
    monkeypatch.setenv("ALABI_CHOL_TASKS", "1")
    monkeypatch.setenv("ALABI_CHOL_W8", w8)
    monkeypatch.setenv("ALABI_CHOL_UPDATE2", two)
    monkeypatch.setenv("ALABI_CHOL_UPDATE4", four)
    bad = _run_cases(torch_gpu, 2000, "queue")
    assert bad == []


@pytest.mark.parametrize("N,path", [(70, "steps"), (2000, "queue")])
def test_default_path_reports_lapack_info(torch_gpu, monkeypatch, N, path):
    """No switch set: below the queue's threshold of 3 block columns and above it.  (A wait that ran out earlier in this process --
    test_cholesky_task_queue forces one -- keeps the next 64 unforced fits off the queue; healthy fits use that up first.)"""
    _clear_env(monkeypatch)
    X, y, h = _problem(N)
    g = _gp(h)
    for _ in range(70):
        g.compute(X)
        if g.solver.factor_path == path:
            break
    assert g.solver.factor_path == path
    bad = _run_cases(torch_gpu, N, path)
    assert bad == []


PATHS = {"rank64": {"ALABI_CHOL_TASKS": "0", "ALABI_CHOL_PANEL": "0"},
         "panel4": {"ALABI_CHOL_TASKS": "0", "ALABI_CHOL_PANEL": "4", "ALABI_CHOL_LOOKAHEAD": "1"},
         "panel8-serial": {"ALABI_CHOL_TASKS": "0", "ALABI_CHOL_PANEL": "8", "ALABI_CHOL_LOOKAHEAD": "0"},
         "queue4": {"ALABI_CHOL_TASKS": "1", "ALABI_CHOL_W8": "0"},
         "queue8": {"ALABI_CHOL_TASKS": "1", "ALABI_CHOL_W8": "1"}}


def _force(monkeypatch, name):
    _clear_env(monkeypatch)
    for k, v in PATHS[name].items():
        monkeypatch.setenv(k, v)
    return "queue" if name.startswith("queue") else "steps"


@pytest.mark.parametrize("kernel", ["Matern52Kernel", "RationalQuadraticKernel"])
@pytest.mark.parametrize("name", list(PATHS))
def test_other_families_report_lapack_info(torch_gpu, monkeypatch, name, kernel):
    """One Matern-5/2 and one rational-quadratic case per path (N = 1100: 18 block columns); the rational quadratic kernel never
    underflows to zero, so it gets construction (a) only."""
    path = _force(monkeypatch, name)
    N = 1100
    X, y, h = _problem(N, kernel)
    g, bad = _gp(h, kernel), []
    for p in (40, 64 * 9 + 29, N - 1):
        _check_failure(g, nonfinite_row(X, p, np.nan, 2), y, p + 1, path, ("nan", p), bad)
    _check_failure(g, nonfinite_row(X, 700, -np.inf, 1), y, 701, path, ("-inf", 700), bad)
    if kernel != "RationalQuadraticKernel":
        _, _, h1 = _problem(N, kernel, ones=True)
        g1 = _gp(h1, kernel)
        for q, p in ((7, 64 * 9 + 33), (64 * 9, 64 * 9 + 63), (N - 2, N - 1)):
            _check_failure(g1, ones_block(X, q, p), y, p + 1, path, ("ones", q, p), bad)
    assert bad == []


@pytest.mark.parametrize("name,N", [("rank64", 705), ("panel4", 705), ("panel8-serial", 2900), ("queue4", 705), ("queue8", 705), ("queue8", 2000)])
def test_handle_reuse_after_failure(torch_gpu, monkeypatch, name, N):
    """After a failure the same handle factorises the healthy X: bit for bit the factor of a fresh handle, on the forced path --
    the status word, the queue's control words and the time-out penalty leave nothing behind.  Then failures at an EARLIER and at a
    LATER pivot report the new index (the status word is set by atomicCAS(info, 0, ..): a stale non-zero value would win)."""
    path = _force(monkeypatch, name)
    X, y, h = _problem(N)
    fresh = _gp(h)
    fresh.compute(X)
    assert fresh.solver.factor_path == path and fresh.last_pivot == 0
    L0 = fresh.solver.get_factor().cpu().numpy()
    g, bad = _gp(h), []
    p1, p2, p3 = N // 2, 17, N - 3
    _check_failure(g, nonfinite_row(X, p1, np.nan, 0), y, p1 + 1, path, ("nan", p1), bad)
    assert bad == []
    assert g.compute(X) is True and g.last_pivot == 0 and g.solver.factor_path == path
    assert np.array_equal(g.solver.get_factor().cpu().numpy(), L0)
    ll0 = fresh.log_likelihood(y)
    assert g.log_likelihood(y) == ll0
    _check_failure(g, nonfinite_row(X, p2, np.inf, 1), y, p2 + 1, path, ("inf", p2), bad)
    _check_failure(g, nonfinite_row(X, p3, np.nan, 2), y, p3 + 1, path, ("nan", p3), bad)
    assert bad == []
    assert g.compute(X) is True and g.last_pivot == 0 and g.solver.factor_path == path
    assert np.array_equal(g.solver.get_factor().cpu().numpy(), L0)


@pytest.mark.parametrize("mode", ["1", "0"])
def test_batch_reports_each_jobs_lapack_info(torch_gpu, monkeypatch, mode):
    """HipGPBatch.fit_predict (the batched queue, ALABI_BATCH_QUEUE=1, and its launch-per-step fallback, 0) with the job sizes of
    test_batch_not_positive_definite_job_is_isolated_and_fallback_agrees: three rows of the shared X are not finite, and three
    jobs train on one of them each -- in the first tile, deep in the matrix, on the last row -- beside two healthy jobs, one of
    which has a bad row among its validation points.  status[j] is each job's own index; the healthy jobs' factors are bit for bit
    those of the same batch on a clean X."""
    torch = torch_gpu
    from alabi_amd.gp_batch import HipGPBatch
    from oracle.gp_oracle import OracleGP
    _clear_env(monkeypatch)
    monkeypatch.setenv("ALABI_BATCH_QUEUE", mode)
    n, d = 900, 4
    sizes = [700, 640, 705, 512, 700]
    X, y, hyper, train, val = _jobs(n, d, 17, sizes)
    rng = np.random.RandomState(3)
    X = np.vstack([X, rng.uniform(-3, 3, (3, d))]); y = np.r_[y, y[:3]]          # rows 900..902: used by nobody so far
    train = [t.copy() for t in train]; val = [v.copy() for v in val]
    where = {0: (10, 900), 2: (500, 901), 4: (699, 902)}                          # job -> (position in its training list, row of X)
    for j, (p, r) in where.items():
        train[j][p] = r
    val[3][5] = 900                                                               # a healthy job predicts AT a bad row
    for j, N in enumerate(sizes):                                                 # premise: LAPACK factors every clean job
        assert healthy_factors(OracleGP(d, hyper[j, 0], hyper[j, 1], hyper[j, 2], hyper[j, 4:]).get_matrix(X[train[j]])), j
    Xbad = X.copy()
    Xbad[900, 1], Xbad[901, 0], Xbad[902, 3] = np.nan, np.inf, np.nan
    dev = torch.device("cuda")
    yd = torch.as_tensor(y, device=dev)
    healthy = [1, 3]
    res = {}
    for tag, Xv in (("clean", X), ("bad", Xbad)):
        bt = HipGPBatch(d)
        ll, status, mu, off = bt.fit_predict(torch.as_tensor(Xv, device=dev), yd, hyper, train, val)
        facs = {j: bt.get_factor(j, sizes[j]).cpu().numpy() for j in healthy}
        res[tag] = (ll.copy(), status.copy(), mu.cpu().numpy().copy(), facs, bt.timeouts)
        bt.close()
    ll0, st0, mu0, f0, to0 = res["clean"]
    ll1, st1, mu1, f1, to1 = res["bad"]
    assert to0 == 0 and to1 == 0
    assert np.all(st0 == 0) and np.all(np.isfinite(ll0)) and np.all(np.isfinite(mu0))
    want = np.zeros(5, dtype=int)
    for j, (p, r) in where.items():
        want[j] = p + 1
    assert list(st1) == list(want)
    for j in where:
        assert ll1[j] == -np.inf and np.all(np.isnan(mu1[off[j]:off[j + 1]]))
    for j in healthy:
        assert np.array_equal(f0[j], f1[j]), j
        assert abs(ll1[j] - ll0[j]) <= 1e-9 * (abs(ll0[j]) + 1)
        a, b = mu1[off[j]:off[j + 1]].copy(), mu0[off[j]:off[j + 1]].copy()
        if j == 3:
            assert np.isnan(a[5])
            a[5] = b[5] = 0.0
        assert np.all(np.isfinite(a))
        assert np.max(np.abs(a - b)) <= 1e-8 * (np.max(np.abs(b)) + 1)


def _record(g, y, qs):
    """Everything the old object is asked for around a rejected append, as raw arrays."""
    out = [g.predict(y, qs[300], return_cov=False)]
    for M in (7, 300, 5000):                                 # the three variance paths (the small one from Npad = 256 on)
        out += list(g.predict(y, qs[M], return_var=True))
    out += [np.array(a) for a in g.predict_grad_host(y, qs[7])]
    out += [np.array(a) for a in g.predict_grad_host(y, qs[7][0])]
    out += [np.array([g.log_likelihood(y)]), g.grad_log_likelihood(y)]
    return out


def _same_bits(a, b):
    return len(a) == len(b) and all(x.shape == z.shape and np.array_equal(x, z, equal_nan=True) for x, z in zip(a, b))


@pytest.mark.parametrize("kind", ["nan", "ones"])
@pytest.mark.parametrize("N,kernel", [(150, "ExpSquaredKernel"), (150, "Matern52Kernel"), (300, "ExpSquaredKernel")])
def test_rejected_append_leaves_the_factor_alone(torch_gpu, kind, N, kernel):
    """alabi_gp_append of a point whose pivot fails -- a NaN coordinate, or a construction-(b) duplicate of a far training point --
    reports N + 1 and leaves the old object's factor, training set and caches alone: mean, mean + variance on all three variance
    paths, prediction gradients, likelihood and its gradient are bit for bit what they were.  HipGP.compute_from then falls back
    to a full factorisation, which fails with the same index.  A healthy point appended afterwards matches the oracle within the
    tolerances of test_append_point_matches_full_factorisation."""
    torch = torch_gpu
    from alabi_amd import HipGP, _lib
    from oracle.gp_oracle import OracleGP
    from notpd_numpy import far_point
    X, y, h = make_problem(N + 1, D, 70 + N)
    if kind == "ones":
        h = ones_hyper(h)
        X = X.copy(); X[N // 3] = far_point(X)                # the far point is in the training set; its twin is appended
        x_bad = X[N // 3].copy()
    else:
        x_bad = X[N].copy(); x_bad[2] = np.nan
    mk = lambda: HipGP(D, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel)  # noqa: E731
    orc = lambda: OracleGP(D, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel)  # noqa: E731
    assert healthy_factors(orc().get_matrix(X))               # ... so the old factor AND the healthy append exist
    rng = np.random.RandomState(N)
    qs = {M: rng.uniform(-3, 3, (M, D)) for M in (7, 300, 5000)}
    g = mk(); g.compute(X[:N])
    yo = y[:N]
    _record(g, yo, qs)                                        # (builds the cached L^-1 and the matrix-core operands)
    base = _record(g, yo, qs)
    assert _same_bits(base, _record(g, yo, qs))               # the record itself is reproducible
    assert all(np.all(np.isfinite(a)) for a in base)
    # the library call itself
    st = _lib.lib().alabi_gp_append(g._handle, _lib.ptr(torch.as_tensor(x_bad, device=torch.device("cuda"))), _lib.current_stream())
    assert st == _lib.NOT_PD and g.last_pivot == N + 1
    assert _same_bits(base, _record(g, yo, qs))
    # the Python route: refused append, then the full factorisation fails at the same pivot
    gbad = mk()
    with pytest.raises(np.linalg.LinAlgError) as ei:
        gbad.compute_from(g, np.vstack([X[:N], x_bad]))
    assert g.last_pivot == N + 1 and gbad.last_pivot == N + 1
    assert str(ei.value) == f"{N + 1}-th leading minor of the array is not positive definite"
    assert g.computed and not g.dirty
    assert _same_bits(base, _record(g, yo, qs))
    # a healthy point still goes in
    g2 = mk()
    assert g2.compute_from(g, X[:N + 1]) is True
    assert getattr(g2, "appended", 0) == 1 and g2.last_pivot == 0
    o = orc().compute(X[:N + 1])
    amp = np.exp(h["log_amp"])
    Lf = g2.solver.get_factor().cpu().numpy()
    assert np.max(np.abs(Lf - o._L)) <= 1e-9 * np.max(np.abs(o._L))
    for M in (7, 300, 5000):
        mu, var = g2.predict(y, qs[M], return_var=True)
        mu_o, var_o = o.predict(y, qs[M], return_var=True)
        assert np.max(np.abs(mu - mu_o) / (np.abs(mu_o) + 1)) <= 1e-8
        assert np.max(np.abs(var - var_o)) <= 1e-7 * amp
    assert abs(g2.log_likelihood(y) - o.log_likelihood(y)) <= 1e-8 * abs(o.log_likelihood(y))
    go = o.grad_log_likelihood(y)
    np.testing.assert_allclose(g2.grad_log_likelihood(y), go, rtol=1e-6, atol=1e-7 * np.max(np.abs(go)))
