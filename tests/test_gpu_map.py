"""GPU parity of ``EnsembleSampler.maximize`` (ens_map_kernel, alabi_ens_maximize) with tests/map_numpy.py on the cases of
tests/map_cases.py: every (d, kernel) pair of hmc_cases.GRID -- every dimension bucket boundary -- and the tiled, nlog, log, prior
and offset problems.  tests/test_map_host.py shows on the CPU that the model runs are honest (they reach scipy's optimum, no traced
decision is a near tie); here the device is held to them.

Per case, for the eight starts (six random, one on a training point, one at a corner of the shrunk box) and a ninth outside the box:
  * status 0 for the eight, status 3 and NaN for the ninth;
  * grad_norm <= gtol, re-evaluated through the independent ``log_prob_grad`` at the returned point;
  * log_prob >= the start's;
  * the distance to the optimum on the free coordinates is at most 2 sqrt(d) gtol / lambda_min(-H_truth): g ~ H (x - x*), so
    |x - x*|_2 <= |g|_2 / lambda_min <= sqrt(d) gtol / lambda_min; the factor 2 covers the reference's own residual and the
    Hessian's variation.  x* is the model's end point polished by Newton steps with the truth Hessian (map_cases.optimum), H_truth
    tests/hess_reference.py's;
  * held coordinates sit exactly on the shrunk wall, and the coordinates on a wall are the model's held set (d = 64: one);
  * the first 6 iterations (trace=6) equal the model's in step length, held mask and update flag exactly, and in lp to 1e-9
    relative to |lp|.  Where lp nearly cancels (at d = 1 it is -8e-6, a sum of terms of size amp |alpha| k) 1e-9 |lp| is below
    the rounding of the sum itself; such an entry is held to 2 dM instead, dM = u sum_n |term_n| (E + N - 1 + c A) + u (|Mu| +
    |folded mean|) of tests/grad_reference.py at the model's point: the device's evaluation and the model's each lie within dM of
    the exact value, whatever the order of their sums.  The count of such entries is printed.
Cross-checks: the bits of a start's result depend neither on S nor on its place in the batch; maxiter=2 gives status 1; a table
beyond the LDS limit raises; host callables are refused; status 2 with the failed search's second attempt (gtol = 0) and status 3
after one evaluation (a value that is not finite) occur on the device.
"""
import numpy as np
import pytest

import hmc_cases as hc
import map_cases as mc
import map_numpy as mn
import moves_shapes_common as ms

pytestmark = pytest.mark.gpu

S = mc.S_STARTS


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def _sampler(name):
    prob, ex, _ = mc.case(name)
    return ms.sampler(prob, 2, 5, **hc.sampler_kw(ex))


def _numpy(res):
    keys = ("x", "log_prob", "iterations", "evaluations", "status", "grad_norm", "trace_log_prob", "trace_step", "trace_held",
            "trace_updated")
    return {k: getattr(res, k).cpu().numpy() for k in keys if getattr(res, k) is not None}


@pytest.mark.parametrize("name", mc.CASES, ids=mc.case_id)
def test_maximize_against_the_model(torch_gpu, name):
    torch = torch_gpu
    prob, ex, _ = mc.case(name)
    d = prob.d
    los, his, _ = mn.shrunk_box(prob.bounds)
    starts = mc.starts(name).copy()
    s = _sampler(name)
    r = _numpy(s.maximize(torch.as_tensor(starts, device="cuda"), maxiter=mc.MAXITER, gtol=mc.GTOL, trace=mc.NTRACE))
    model, tgt = mc.model(name), mc.case(name)[2]
    if name == "offset":
        # inputs thousands of length scales out and weights of 1e4: the oracle's alpha moves lp by 2e-8, so the model runs on the
        # device's own alpha here, as the truth tests do; the run is held to the same no-tie condition first
        g = ms.device_gp(prob)
        g.predict(prob.y, starts[:1], return_var=True)
        tgt = mc.ScaledInputTarget(prob, ex, np.asarray(g._alpha, dtype=np.float64))
        model = mn.maximize(tgt, starts, prob.bounds, mc.MAXITER, mc.GTOL, mc.NTRACE)
        assert min(mc.margins_of(model[:S]).values()) > mc.MIN_MARGIN, mc.margins_of(model[:S])
    print("MAP %-22s iterations %s evaluations %s (model %s)" % (mc.case_id(name), r["iterations"].tolist(), r["evaluations"].tolist(),
                                                                [m.iterations for m in model]))
    # the start outside the box
    assert r["status"][S] == mn.BAD_START and np.all(np.isnan(r["x"][S])) and np.isnan(r["log_prob"][S]) and np.isnan(r["grad_norm"][S])
    assert r["status"][:S].tolist() == [mn.CONVERGED] * S, r["status"]
    assert np.all(r["grad_norm"][:S] <= mc.GTOL)
    assert np.all((r["x"][:S] >= los) & (r["x"][:S] <= his))
    # the projected gradient by the independent evaluation, and the start's value
    lp_x, g_x = (t.cpu().numpy() for t in s.log_prob_grad(torch.as_tensor(r["x"][:S], device="cuda")))
    lp_0 = s.log_prob_grad(torch.as_tensor(np.minimum(np.maximum(starts[:S], los), his), device="cuda"))[0].cpu().numpy()
    held_dev = ((r["x"][:S] <= los) & (g_x < 0.0)) | ((r["x"][:S] >= his) & (g_x > 0.0))
    pg = np.max(np.abs(np.where(held_dev, 0.0, g_x)), axis=1)
    print("    projected gradient %.2e (reported %.2e)" % (pg.max(), r["grad_norm"][:S].max()))
    assert np.all(pg <= mc.GTOL)
    assert np.array_equal(lp_x, r["log_prob"][:S])
    assert np.all(r["log_prob"][:S] >= lp_0)
    failures, n_derived = [], 0
    for i in range(S):
        m = model[i]
        x_opt, lam, resid = mc.optimum(name, i) if name != "offset" else mc.optimum_of(prob, ex, tgt, m)
        assert resid < 1e-3 * mc.GTOL and lam > 0.0, (i, resid, lam)
        free = ~m.held
        dist = float(np.linalg.norm((r["x"][i] - x_opt)[free]))
        bound = 2.0 * np.sqrt(d) * mc.GTOL / lam
        on_wall = (r["x"][i] == los) | (r["x"][i] == his)
        if i == 0:
            print("    start 0: distance %.2e, bound %.2e (lambda_min %.3g); held %d" % (dist, bound, lam, int(m.held.sum())))
        if not dist <= bound:
            failures.append((i, "distance", dist, bound))
        if not (np.array_equal(on_wall, m.held) and np.array_equal(held_dev[i], m.held)):
            failures.append((i, "held set", np.nonzero(on_wall)[0].tolist(), np.nonzero(m.held)[0].tolist()))
        # the trace
        n = len(m.trace)
        done = ~np.isnan(r["trace_step"][i])
        if not (done[:n].all() and not done[n:].any() and (n == mc.NTRACE or r["iterations"][i] == n)):
            failures.append((i, "traced iterations", int(done.sum()), n))
            continue
        for k, (lp, t, mask, upd) in enumerate(m.trace):
            got = (float(r["trace_step"][i, k]), int(r["trace_held"][i, k]) & (2 ** 64 - 1), bool(r["trace_updated"][i, k]))
            if got != (t, mask, upd):
                failures.append((i, "trace", k, got, (t, mask, upd)))
            err = abs(r["trace_log_prob"][i, k] - lp)
            if not err <= 1e-9 * abs(lp):
                # lp nearly cancels here: the device and the model each lie within dM of the exact sum at the point
                dM = mc.value_rounding_bound(name, m.trace_x[k]) if name != "offset" else None
                n_derived += 1
                if dM is None or not err <= 2.0 * dM[0]:
                    failures.append((i, "trace lp", k, float(r["trace_log_prob"][i, k]), lp, None if dM is None else float(dM[0])))
    print("    traced lp beyond 1e-9 |lp|, held to the derived bound instead: %d" % n_derived)
    assert not failures, failures


@pytest.mark.parametrize("name", [(7, "Matern52"), (64, "ExpSquared"), "tiled"], ids=mc.case_id)
def test_bits_do_not_depend_on_the_batch(torch_gpu, name):
    """A start gives the same bits alone, in the batch of nine, and at another place of a permuted batch."""
    torch = torch_gpu
    starts = mc.starts(name).copy()
    s = _sampler(name)
    keys = ("x", "log_prob", "iterations", "evaluations", "status", "grad_norm")
    full = _numpy(s.maximize(torch.as_tensor(starts, device="cuda")))
    perm = np.random.RandomState(1).permutation(len(starts))
    mixed = _numpy(s.maximize(torch.as_tensor(starts[perm], device="cuda")))
    alone = _numpy(s.maximize(torch.as_tensor(starts[2:3], device="cuda")))
    for k in keys:
        assert np.array_equal(mixed[k], full[k][perm], equal_nan=True), k
        assert np.array_equal(alone[k], full[k][2:3]), k


def test_maxiter_gives_status_1(torch_gpu):
    torch = torch_gpu
    name = (10, "ExpSquared")
    s = _sampler(name)
    r = _numpy(s.maximize(torch.as_tensor(mc.starts(name)[:S].copy(), device="cuda"), maxiter=2))
    lp_0 = s.log_prob_grad(torch.as_tensor(mc.starts(name)[:S].copy(), device="cuda"))[0].cpu().numpy()
    assert r["status"].tolist() == [mn.MAXITER] * S and r["iterations"].tolist() == [2] * S
    assert np.all(r["grad_norm"] > mc.GTOL) and np.all(r["log_prob"] > lp_0)
    model = mc.model(name, maxiter=2)
    assert [m.status for m in model[:S]] == [mn.MAXITER] * S
    assert np.allclose(r["x"], np.array([m.x for m in model[:S]]), rtol=0, atol=1e-9)


def test_no_ascent_and_the_second_attempt_on_the_device(torch_gpu):
    """gtol = 0 can only be met by a gradient of exactly 0: the search runs on into the rounding of the value and the gradient
    until no trial is accepted, repeats the search once with B reset (30 more trials), and ends with status 2 and the best point
    kept -- the model does so on every start of this case.  The device's rounding differs, so a start may also end by a gradient
    of exactly 0 or by maxiter; what is asserted is that status 2 occurs with its 60 failed trials, and that every start ends at
    the maximum."""
    torch = torch_gpu
    name = (7, "Matern52")
    assert [m.status for m in mn.maximize(mc.case(name)[2], mc.starts(name)[:S], mc.case(name)[0].bounds, 200, 0.0, 0)] == [mn.NO_ASCENT] * S
    s = _sampler(name)
    starts = torch.as_tensor(mc.starts(name)[:S].copy(), device="cuda")
    ref = _numpy(s.maximize(starts))
    r = _numpy(s.maximize(starts, gtol=0.0))
    print("MAP gtol = 0: status %s iterations %s evaluations %s grad_norm %s" % (r["status"].tolist(), r["iterations"].tolist(),
                                                                             r["evaluations"].tolist(), r["grad_norm"].tolist()))
    assert set(r["status"].tolist()) <= {0, 1, 2} and (r["status"] == mn.NO_ASCENT).sum() >= 1
    stuck = r["status"] == mn.NO_ASCENT
    assert np.all(r["evaluations"][stuck] >= r["iterations"][stuck] + 1 + 2 * mn.LS_MAX - 1)   # two failed searches at the end
    assert np.all(r["grad_norm"] < 1e-10) and np.all(r["log_prob"] >= ref["log_prob"] - 1e-8 * np.maximum(1.0, np.abs(ref["log_prob"])))
    assert np.allclose(r["x"], ref["x"], rtol=0, atol=1e-6)


def test_a_start_without_a_finite_value_is_status_3(torch_gpu):
    """10^(1000 mu) overflows wherever mu > 0.31: the start lies inside the box, ONE evaluation finds the value not finite, and the
    outputs are NaN with status 3."""
    torch = torch_gpu
    prob, _ = hc.lpg_problem("log")
    s = ms.sampler(prob, 2, 5, logp_map="log", logp_affine=(1000.0, 0.0))
    x0 = prob.X[int(np.argmax(prob.y))][None, :]
    assert np.all((x0 > prob.bounds[:, 0]) & (x0 < prob.bounds[:, 1])) and prob.y.max() > 0.5
    r = _numpy(s.maximize(torch.as_tensor(x0, device="cuda")))
    assert r["status"].tolist() == [mn.BAD_START] and r["evaluations"].tolist() == [1] and r["iterations"].tolist() == [0]
    assert np.all(np.isnan(r["x"])) and np.isnan(r["log_prob"][0]) and np.isnan(r["grad_norm"][0])


def test_a_table_beyond_the_lds_is_refused(torch_gpu):
    """B [64][65] and the weights of 12400 training points need 132.5 KB of LDS: alabi_ens_maximize is ALABI_BAD_ARGUMENT (there is
    no other kernel for it), and the plan says so beforehand."""
    import ctypes as C
    from alabi_amd import EnsembleSampler, HipGP, _lib
    d, N = 64, 12400
    rs = np.random.RandomState(0)
    X = rs.uniform(-3.0, 3.0, (N, d))
    y = np.sin(X[:, 0]) + 0.1 * rs.randn(N)
    g = HipGP(d, 0.0, -2.0, 0.0, np.full(d, np.log(4.0 * d)))
    g.compute(X)
    s = EnsembleSampler(2, d, g, y, np.stack([np.full(d, -3.0), np.full(d, 3.0)], axis=1), seed=1, live_dangerously=True)
    s._ensure_ens()
    plan = (C.c_int * 4)()
    _lib.check(_lib.lib().alabi_ens_map_plan(s._ens, plan), "alabi_ens_map_plan")
    assert plan[1] > 128 * 1024 and plan[2] == 1 and plan[3] == 64
    with pytest.raises(_lib.AlabiHipError):
        s.maximize(np.zeros((1, d)))


def test_plan_and_refusals(torch_gpu):
    import ctypes as C
    from alabi_amd import EnsembleSampler, _lib
    prob, ex, _ = mc.case("tiled")
    s = _sampler("tiled")
    s._ensure_ens()
    plan = (C.c_int * 4)()
    _lib.check(_lib.lib().alabi_ens_map_plan(s._ens, plan), "alabi_ens_map_plan")
    assert plan[0] in (256, 512) and plan[1] >= (5 * 5 + 520) * 8 and plan[1] % 8 == 0 and plan[2] == 1 and plan[3] == 5, list(plan)
    with pytest.raises(ValueError):
        s.maximize(np.zeros((1, prob.d + 1)))
    with pytest.raises(ValueError):
        s.maximize(np.zeros((1, prob.d)), gtol=float("nan"))
    h = EnsembleSampler(2 * prob.d, prob.d, ms.device_gp(prob), prob.y, prob.bounds, seed=1, prior_fn=lambda q: np.zeros(len(q)))
    with pytest.raises(ValueError, match="needs the fused log-probability"):
        h.maximize(np.zeros((1, prob.d)))
    with pytest.raises(ValueError, match="needs the fused log-probability"):
        h.log_prob_hessian(np.zeros((1, prob.d)))
