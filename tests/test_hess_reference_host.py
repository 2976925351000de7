"""tests/hess_reference.py on the host: the bound is attainable and not slack, and the truth is the Hessian.
  1. ens_lp_hess_kernel's formulation in plain fp64 (``log_prob_hessian_fp64``) lies inside ``log_prob_hessian``'s tolerance for
     all four families and under every setting (identity, affine, nlog, log, prior), at points that include a query ON a training
     point;
  2. planted defects lie outside: a dropped diagonal term, f'' of the wrong family, a missing dMu dMu^T term under a y map;
  3. the truth agrees with central differences of grad_reference's extended-precision gradient.
"""
import numpy as np
import pytest

import grad_reference as gr
import hess_reference as hr
import hmc_cases as hc
import map_cases as mc

LD = hr.LD
CASES = [(3, "ExpSquared"), (3, "Matern32"), (3, "Matern52"), (3, "RationalQuadratic"), (17, "Matern32"), (64, "RationalQuadratic"),
         "tiled", "nlog", "log", "prior", "offset"]


def _setup(name):
    prob, ex = hc.lpg_problem(name)
    pts = hc.lpg_points(prob)[[0, 4, 5, 6]]                      # row 0 sits on a training point
    X, al, amp, inv_len, mean, family, la = hr.problem_inputs(prob)
    kw = dict(affine=ex.get("affine", (1.0, 0.0)), ymap=ex.get("ymap"), prior=ex.get("prior"))
    return prob, pts, (X, al, amp, inv_len), (mean, family, la), kw


@pytest.mark.parametrize("name", CASES, ids=mc.case_id)
def test_tolerance_is_attainable_and_not_slack(name):
    prob, pts, (X, al, amp, inv_len), (mean, family, la), kw = _setup(name)
    assert np.array_equal(pts[0], prob.X[3])
    H, tol = hr.log_prob_hessian(X, al, amp, inv_len, pts, mean, family, la, **kw)
    assert np.all(np.isfinite(H.astype(np.float64))) and np.all(np.isfinite(tol)) and np.all(tol > 0)
    assert np.max(np.abs((H - np.swapaxes(H, 1, 2)).astype(np.float64))) <= 1e-17 * np.max(np.abs(H.astype(np.float64)))
    honest = hr.log_prob_hessian_fp64(X, al, amp, inv_len, pts, mean, family, la, **kw)
    frac = np.abs((honest.astype(LD) - H).astype(np.float64)) / tol
    defects = ["no_diag", "wrong_family"] + (["no_outer"] if kw["ymap"] is not None else [])
    out = {}
    for mut in defects:
        bad = hr.log_prob_hessian_fp64(X, al, amp, inv_len, pts, mean, family, la, mutate=mut, **kw)
        out[mut] = float(np.max(np.abs((bad.astype(LD) - H).astype(np.float64)) / tol, axis=(1, 2)).min())
    print("HESS host %-22s honest fp64 %.3f of the tolerance; defects (the least-hit query) %s" % (
        mc.case_id(name), frac.max(), {k: "%.1e" % v for k, v in out.items()}))
    assert np.all(frac <= 1.0), float(frac.max())
    assert frac.max() > 1e-4, "a bound no honest evaluation comes near says nothing"
    for mut, v in out.items():
        assert v > 100.0, (mut, v)


@pytest.mark.parametrize("name", CASES, ids=mc.case_id)
def test_truth_is_the_derivative_of_the_gradient_truth(name):
    """Central differences of ``grad_reference.log_prob_gradient``'s extended-precision gradient, step 1e-5 length scales: the
    truncation error is 1e-10 relative, the long double's rounding 1e-19 / 1e-5."""
    prob, pts, (X, al, amp, inv_len), (mean, family, la), kw = _setup(name)
    pts = pts[1:]                                                # off the training point: Matern-3/2 has no third derivative there
    H, _ = hr.log_prob_hessian(X, al, amp, inv_len, pts, mean, family, la, with_tolerance=False, **kw)
    d = prob.d
    cols = range(d) if d <= 5 else (0, d // 2, d - 1)
    worst = 0.0
    for k in cols:
        e = np.zeros(d); e[k] = 1e-5 / inv_len[k]
        # the step must be exact in the scaled coordinates the truth reads: difference the scaled queries it actually saw
        up = gr.log_prob_gradient(X, al, amp, inv_len, pts + e, mean, family, la, **kw)["grad"]
        dn = gr.log_prob_gradient(X, al, amp, inv_len, pts - e, mean, family, la, **kw)["grad"]
        sp = (hr.ksr.scaled(pts + e, inv_len)[:, k].astype(LD) - hr.ksr.scaled(pts - e, inv_len)[:, k].astype(LD)) / LD(inv_len[k])
        fd = (up - dn) / sp[:, None]
        scale = np.max(np.abs(H.astype(np.float64)), axis=(1, 2))
        worst = max(worst, float(np.max(np.abs((fd - H[:, :, k]).astype(np.float64)) / scale[:, None])))
    print("HESS host %-22s truth against central differences of the gradient truth: %.2e of the largest entry" % (mc.case_id(name), worst))
    assert worst < 1e-7
