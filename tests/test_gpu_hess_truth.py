"""``EnsembleSampler.log_prob_hessian`` (ens_lp_hess_kernel, alabi_ens_log_prob_hessian) against the extended-precision truth of
tests/hess_reference.py, within its bound, on the log_prob_grad cases and points of tests/hmc_cases.py: every (d, kernel) pair of
the grid and the tiled, nlog, log, prior and offset problems, 32 points each -- one on a training point, two outside the box (all
NaN), one on its wall (the box is open: NaN).  The device's own alpha is the truth's input, so the comparison isolates the sums.
The result is symmetric to the bit."""
import numpy as np
import pytest

import hess_reference as hr
import hmc_cases as hc
import map_cases as mc
import moves_shapes_common as ms

pytestmark = pytest.mark.gpu
LD = hr.LD


@pytest.mark.parametrize("name", mc.CASES, ids=mc.case_id)
def test_log_prob_hessian_against_extended_precision_truth(name):
    import torch
    prob, ex = hc.lpg_problem(name)
    d = prob.d
    pts = hc.lpg_points(prob)
    g = ms.device_gp(prob)
    g.predict(prob.y, pts[:1], return_var=True)
    alpha = np.asarray(g._alpha, dtype=np.float64)
    s = ms.sampler(prob, 2, 5, **hc.sampler_kw(ex))
    H = s.log_prob_hessian(torch.as_tensor(pts, device="cuda")).cpu().numpy()
    assert H.shape == (32, d, d)
    outside = ~np.all((pts > prob.bounds[:, 0]) & (pts < prob.bounds[:, 1]), axis=1)
    assert outside.tolist() == [False, True, True, True] + [False] * 28
    assert np.all(np.isnan(H[outside])) and np.all(np.isfinite(H[~outside]))
    assert np.array_equal(H[~outside], np.swapaxes(H[~outside], 1, 2)), "symmetric to the bit"
    keep = np.nonzero(~outside)[0][::hr.ksr.QUERY_STRIDE]
    Ht, tol = hr.problem_hessian(prob, ex, pts[keep], alpha=alpha, with_tolerance=True)
    assert np.all(np.isfinite(tol)) and np.all(tol > 0)
    frac = np.abs((H[keep].astype(LD) - Ht).astype(np.float64)) / tol
    scale = np.max(np.abs(Ht.astype(np.float64)), axis=(1, 2), keepdims=True)
    print("HESS %-22s worst err/tol %.3f | worst error %.2e of the largest entry | tol %.1e of it" % (
        mc.case_id(name), frac.max(), np.max(np.abs((H[keep].astype(LD) - Ht).astype(np.float64)) / scale), np.max(tol / scale)))
    assert np.all(frac <= 1.0), (float(frac.max()), np.argwhere(frac > 1.0)[:4].tolist())
