"""The NumPy statement of the device optimiser (tests/map_numpy.py) is honest on every case of tests/map_cases.py, shown on the
CPU before tests/test_gpu_map.py holds the device to it:
  1. every one of the eight starts converges (status 0), the ninth (outside the box) is status 3 with NaN outputs;
  2. the model reaches the optimum scipy's L-BFGS-B finds from the same start on the same shrunk box, within 2 sqrt(d) gtol /
     lambda_min(-H_truth) on the free coordinates (the bound tests/test_gpu_map.py derives), and holds the coordinates scipy
     leaves on a wall.  scipy is asked for gtol 1e-11 and restarted from its own result, but its search stops short on most
     cases (projected gradient up to 8.5e-8, printed), so its point is polished by two Newton steps with the truth Hessian to a
     projected gradient below 1e-11 (asserted): a reference independent of the model, against which the bound is asserted as
     stated;
  3. its traced log-probabilities increase strictly on every step that the value decided (Armijo).  The steps of the flat zone,
     which the gradient decides (29 of the traced steps, all at d <= 2), are bounded separately: such a step may lower the value
     by the zone's width at the most, 1e-8 max(1, |lp|) -- monotonicity is NOT asserted for them, it cannot hold to the bit
     where the gain is of the size of the rounding of lp;
  4. no traced decision is a near tie: every margin of map_numpy.maximize_one exceeds 1e-9 -- a condition on the cases (the seeds of
     map_cases.SEEDS), not a tolerance;
  5. every status value occurs somewhere.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.optimize as op

import map_cases as mc
import map_numpy as mn


@pytest.mark.parametrize("name", mc.CASES, ids=mc.case_id)
def test_model_converges_without_near_ties(name):
    runs = mc.model(name)
    assert [r.status for r in runs] == [mn.CONVERGED] * mc.S_STARTS + [mn.BAD_START]
    assert np.all(np.isnan(runs[-1].x)) and np.isnan(runs[-1].lp) and runs[-1].evaluations == 0
    m = mc.margins(name)
    print("MAP model %-22s iterations %s margins %s" % (mc.case_id(name), [r.iterations for r in runs[:-1]],
                                                        {k: "%.1e" % v for k, v in m.items()}))
    assert min(m.values()) > mc.MIN_MARGIN, m
    prob, _, tgt = mc.case(name)
    lp0 = tgt.value_grad(np.minimum(np.maximum(mc.starts(name)[:mc.S_STARTS], mn.shrunk_box(prob.bounds)[0]),
                                    mn.shrunk_box(prob.bounds)[1]))[0]
    for r, start_lp in zip(runs[:-1], lp0):
        lps = np.array([start_lp] + [t[0] for t in r.trace])
        flat = np.array(r.trace_flat, dtype=bool)
        assert np.all(np.diff(lps)[~flat] > 0.0), lps                      # the value decided: strictly upward
        assert np.all(np.diff(lps)[flat] >= -mn.FLAT * np.maximum(1.0, np.abs(lps[:-1][flat]))), lps   # the gradient decided
        assert r.lp >= start_lp and r.grad_norm <= mc.GTOL and 1 <= len(r.trace) <= mc.NTRACE
        assert all(t[1] in [2.0 ** -k for k in range(mn.LS_MAX)] for t in r.trace)


@pytest.mark.parametrize("name", mc.CASES, ids=mc.case_id)
def test_model_reaches_scipys_optimum(name):
    prob, _, tgt = mc.case(name)
    los, his, _ = mn.shrunk_box(prob.bounds)
    d = prob.d

    def neg(x):
        L, g, _ = tgt.value_grad(x[None, :])
        return -float(L[0]), -np.asarray(g[0], dtype=np.float64)

    worst = worst_resid = 0.0
    for i, r in enumerate(mc.model(name)[:mc.S_STARTS]):
        x0 = np.minimum(np.maximum(mc.starts(name)[i], los), his)
        for _ in range(4):                                       # restarted from its own result while its search stops short
            res = op.minimize(neg, x0, jac=True, method="L-BFGS-B", bounds=list(zip(los, his)),
                              options=dict(gtol=1e-11, ftol=0.0, maxiter=1000, maxcor=20, maxls=60))
            x0 = res.x
            on = (res.x <= los) | (res.x >= his)
            if np.max(np.abs(res.jac[~on])) <= 1e-11:
                break
        g = -res.jac
        wall = (res.x <= los) | (res.x >= his)
        assert np.array_equal(wall, r.held), (i, np.nonzero(wall)[0], np.nonzero(r.held)[0])
        resid = float(np.max(np.abs(g[~wall])))
        _, lam, _ = mc.optimum(name, i)
        # scipy's point polished by Newton steps with the truth Hessian: a reference that owes nothing to the model
        x_ref, lam_ref, resid_ref = mc.optimum_of(prob, mc.case(name)[1], tgt, SimpleNamespace(x=res.x, held=wall))
        assert resid_ref <= 1e-11, (i, resid_ref)
        bound = 2.0 * np.sqrt(d) * mc.GTOL / min(lam, lam_ref)
        dist = float(np.linalg.norm((r.x - x_ref)[~r.held]))
        worst = max(worst, dist / bound)
        worst_resid = max(worst_resid, resid)
        assert dist <= bound, (i, dist, bound, lam)
        assert np.all(r.x[r.held] == np.where(r.x[r.held] < prob.off[r.held], los[r.held], his[r.held]))
    print("MAP model %-22s worst distance to scipy's optimum %.3f of the bound; scipy's own projected gradient at most %.1e" % (
        mc.case_id(name), worst, worst_resid))


class _LyingTarget:
    """A finite value at the start alone: no trial is ever accepted."""
    bounds = np.array([[-1.0, 1.0], [-1.0, 1.0]])
    x0 = np.array([0.3, -0.2])

    def value_grad(self, q):
        q = np.atleast_2d(q)
        return np.where(np.all(q == self.x0, axis=1), -np.sum(q * q, axis=1), np.nan), -2.0 * q, None


class _NaNTarget(_LyingTarget):
    def value_grad(self, q):
        q = np.atleast_2d(q)
        return np.full(len(q), np.nan), 2.0 * q, None


def test_every_status_occurs():
    name = (10, "ExpSquared")
    assert {r.status for r in mc.model(name)} == {mn.CONVERGED, mn.BAD_START}
    short = mc.model(name, maxiter=2)
    assert [r.status for r in short[:mc.S_STARTS]] == [mn.MAXITER] * mc.S_STARTS and all(r.iterations == 2 for r in short[:mc.S_STARTS])
    stuck = mn.maximize_one(_LyingTarget(), np.array([0.3, -0.2]), _LyingTarget.bounds)
    assert stuck.status == mn.NO_ASCENT and stuck.iterations == 0 and np.array_equal(stuck.x, [0.3, -0.2]) and stuck.lp == -0.13
    assert stuck.evaluations == 1 + mn.LS_MAX                    # B was fresh: one search, no second attempt
    nan = mn.maximize_one(_NaNTarget(), np.array([0.3, -0.2]), _LyingTarget.bounds)
    assert nan.status == mn.BAD_START and nan.evaluations == 1 and np.all(np.isnan(nan.x))
    on_wall = mn.maximize_one(_LyingTarget(), np.array([1.0, 0.0]), _LyingTarget.bounds)      # the box is open
    assert on_wall.status == mn.BAD_START and on_wall.evaluations == 0
