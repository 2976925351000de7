"""The cases of the likelihood-gradient truth tests (tests/test_hyper_grad_reference_host.py, tests/test_gpu_hyper_grad_truth.py).
Cases that solve_reference (sr) names are taken from there by name.

  sr.GRID + n2d3, n2d10   N in {1, 2, 63, 64, 65, 128, 129, 200} x (d = 3, nugget e^-12), (d = 10, e^-8): both sides of the 64-row
                          tile, one and several block rows
  sr.FAMILY_CASES         n129d3 with the other three kernel families
  rq-lo, rq-hi            the rational quadratic at log_alpha -1.2 and 2.5 on the n129d3 inputs: the log_alpha entry
  d1 d7 d17 d33 d64       N = 65, make_problem(65, d, 7, log_wn=-6, ell2=4 d): the padded dimension buckets 7 -> 8, 17 -> 20, 33 -> 48
  ill, clustered          sr's: conditioning near the limit of fp64
  duplicate-FAMILY        N = 65, d = 3, rows 60..64 exact copies of rows 0..4 (r2 = 0 off the diagonal), Matern-3/2 and
                          rational quadratic
  far                     ksr.lattice(130, 3, 9.0): K diagonal to rounding
  fitted-n65d3/-n129d3    the hyper-parameters at which a host fit stops (FITTED below)
  wide                    N = 1473, d = 3, nugget e^-6: 24 block rows, 300 workgroups, so that grad_final_kernel's strided loop
                          takes a second pass; given-inputs criterion only (no extended-precision factorisation)

FITTED: scipy's L-BFGS-B (maxiter 500, analytic gradient) on the plain fp64 NumPy negative log-likelihood (LAPACK's cho_factor
of sr.matrix_fp64, no regulariser) of make_problem(N, 3, 7), started from make_problem's own hyper-parameters clipped into the box
that SurrogateModel.set_hyperparam_prior_bounds builds for those targets with the model's default ranges (mean within one standard
deviation of mean(y); log_wn in [-15, -9]; log_amp in [0.1 var(y), 10 var(y)], the linear variance as the model has it; log_M in
[-2, 2]).  Both fits stop after 14 iterations on the projected gradient, in a corner of the box: the mean at its lower bound, the
nugget at e^-15, every length scale at its upper bound; the amplitude is interior.  cond(K) is 3e8 and 1.2e9; LAPACK and the
device factor both, so the nugget was not moved.  The vectors are committed as literals: no test refits.

Each case carries ``entries``, the names of the gradient entries it asserts: all that its kernel family has.
"""
import numpy as np

import hyper_grad_reference as hg
import kernel_sum_reference as ksr
import solve_reference as sr

SEED = sr.SEED
# (mean, log_wn, log_amp, log_M) at which the host fit stopped
FITTED = {
    "fitted-n65d3": (65, float.fromhex("-0x1.bfd43af7a0fd6p+1"), -15.0, float.fromhex("0x1.87c1f58651b1fp+0"), (2.0, 2.0, 2.0)),
    "fitted-n129d3": (129, float.fromhex("-0x1.223a537f87b56p+2"), -15.0, float.fromhex("0x1.07ed8003e363cp+1"), (2.0, 2.0, 2.0)),
}
GRID = sr.GRID + ["n2d3", "n2d10"]
RQ = {"rq-lo": -1.2, "rq-hi": 2.5}
BUCKETS = ["d1", "d7", "d17", "d33", "d64"]
DUPLICATE = ["duplicate-Matern32Kernel", "duplicate-RationalQuadraticKernel"]
GROUPS = {"grid": GRID, "families": sr.FAMILY_CASES + list(RQ), "buckets": BUCKETS, "ill, clustered": ["ill", "clustered"],
          "duplicate, far": DUPLICATE + ["far"], "fitted": list(FITTED)}
TRUTH_CASES = [n for names in GROUPS.values() for n in names]        # every case with an extended-precision truth
WIDE = "wide"


def size(name):
    """N of a case, without building it."""
    if name in FITTED:
        return FITTED[name][0]
    if name in RQ:
        return 129
    if name in BUCKETS or name in DUPLICATE:
        return 65
    if name in ("far", WIDE):
        return {"far": 130, WIDE: 1473}[name]
    return {"ill": 192, "clustered": 128}.get(name) or int(name.partition("-")[0][1:].split("d")[0])


def case(name, make_problem):
    """dict(name, X, y, h, family, log_alpha, entries).  ``make_problem`` is conftest's."""
    family, log_alpha = "ExpSquaredKernel", 1.0
    if name in FITTED:
        N, mean, log_wn, log_amp, log_M = FITTED[name]
        X, y, _ = make_problem(N, 3, SEED)
        h = dict(mean=mean, log_white_noise=log_wn, log_amp=log_amp, log_M=np.array(log_M))
    elif name in RQ:
        c = sr.case("n129d3", make_problem)
        X, y, h, family, log_alpha = c["X"], c["y"], c["h"], "RationalQuadraticKernel", RQ[name]
    elif name in BUCKETS:
        d = int(name[1:])
        X, y, h = make_problem(65, d, SEED, log_wn=-6.0, ell2=4.0 * d)
    elif name in DUPLICATE:
        family = name.partition("-")[2]
        X, y, h = make_problem(65, 3, SEED, log_wn=-12.0)
        X = X.copy(); y = y.copy()
        X[60:65], y[60:65] = X[0:5], y[0:5]
    elif name == "far":
        X, y = ksr.lattice(130, 3, 9.0)
        h = dict(mean=float(np.median(y)), log_white_noise=-12.0, log_amp=float(np.log(np.var(y))), log_M=np.zeros(3))
    elif name == WIDE:
        X, y, h = make_problem(1473, 3, SEED, log_wn=-6.0)
    else:
        c = sr.case(name, make_problem)
        X, y, h, family, log_alpha = c["X"], c["y"], c["h"], c["family"], c["log_alpha"]
    return dict(name=name, X=X, y=y, h=h, family=family, log_alpha=log_alpha, entries=hg.family_entries(X.shape[1], family))
