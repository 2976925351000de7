"""Cases and NumPy model runs shared by tests/test_map_host.py (which checks on the CPU that every run is honest: it reaches
scipy's optimum, no traced decision is a near tie, every status occurs) and tests/test_gpu_map.py (which compares the device with
them).  No GPU is touched here.  A model run is computed once per process and shared: the results are not to be modified."""
from functools import lru_cache

import numpy as np

import hmc_cases as hc
import map_numpy as mn
import moves_shapes_common as ms

S_STARTS, NTRACE, MAXITER, GTOL = 8, 6, 200, 1e-8
MIN_MARGIN = 1e-9
CASES = tuple(hc.GRID) + tuple(hc.LPG_EXTRAS)

# Seeds of the six random starts.  A case's seed is 300 + d unless it is listed here (a listed seed was chosen because the default
# one gave a traced decision a margin below MIN_MARGIN); NOTES.md ("MAP and Laplace") records the search.
SEEDS = {}


def case_id(name):
    return name if isinstance(name, str) else "%d-%s" % name


class ScaledInputTarget:
    """hmc_numpy.GPTarget's contract by lp_grad_eval's formulation in plain fp64 (grad_reference.log_prob_grad_fp64): the
    differences are formed from the scaled coordinates fl(x inv_len), as the device forms them.  The oracle behind GPTarget forms
    q - x before it scales; thousands of length scales from the origin that is a difference of INPUTS of some 1000 u relative
    (grad_reference.oracle_gradients), which six iterations of a quasi-Newton search amplify past the 1e-9 the traces are
    compared to.  Used for the "offset" case only.  ``alpha``: the device's own where a GPU test has it (with inputs that far out
    and weights of 1e4 the oracle's alpha differs enough to move lp by 2e-8), else the oracle's."""

    def __init__(self, prob, ex, alpha=None):
        import hess_reference as hr
        self.prob, self.ex, self.bounds = prob, ex, prob.bounds
        self.inputs = hr.problem_inputs(prob, alpha)

    def value_grad(self, q):
        import grad_reference as gr
        X, al, amp, inv_len, mean, family, la = self.inputs
        lp, g = gr.log_prob_grad_fp64(X, al, amp, inv_len, np.atleast_2d(q), mean, family, la, affine=self.ex.get("affine", (1.0, 0.0)),
                                      ymap=self.ex.get("ymap"), prior=self.ex.get("prior"))
        return lp, g, lp


@lru_cache(maxsize=None)
def case(name):
    """(problem, extras, target) of a case: a (d, kernel) pair of hmc_cases.GRID under hmc_cases.extras(d), or one of
    hmc_cases.LPG_EXTRAS."""
    if isinstance(name, tuple):
        prob, ex = ms.problem(*name), hc.extras(name[0])
    else:
        prob, ex = hc.lpg_problem(name)
    return prob, ex, ScaledInputTarget(prob, ex) if name == "offset" else hc.target_of(prob, ex)


@lru_cache(maxsize=None)
def starts(name):
    """[S_STARTS + 1, d]: six random starts, one on a training point, one at a corner of the shrunk box (alternating faces), and
    a last one outside the box."""
    prob = case(name)[0]
    d = prob.d
    rs = np.random.RandomState(SEEDS.get(name, 300 + d))
    x = prob.off + rs.uniform(-2.9, 2.9, (S_STARTS + 1, d))
    x[6] = prob.X[3]
    los, his, _ = mn.shrunk_box(prob.bounds)
    x[7] = np.where(np.arange(d) % 2 == 0, los, his)
    x[8, d - 1] = prob.off[d - 1] + 3.5
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def model(name, maxiter=MAXITER, gtol=GTOL):
    """The model's runs of the case's starts, traced over the first NTRACE iterations."""
    prob, _, tgt = case(name)
    return mn.maximize(tgt, starts(name), prob.bounds, maxiter, gtol, NTRACE)


def margins(name):
    return margins_of(model(name)[:S_STARTS])


def optimum_of(prob, ex, tgt, run):
    """(x*, lambda_min of -H on the free coordinates, the projected gradient left at x*) of a model run: its end point polished
    by two Newton steps on its free coordinates with the truth Hessian of tests/hess_reference.py, which leaves a projected
    gradient of rounding size -- the reference the device's distance is measured from."""
    import hess_reference as hr
    free = ~run.held
    x = run.x.copy()
    for _ in range(2):
        H = hr.problem_hessian(prob, ex, x[None, :])[0][np.ix_(free, free)]
        x[free] -= np.linalg.solve(H, tgt.value_grad(x[None, :])[1][0][free])
    H = hr.problem_hessian(prob, ex, x[None, :])[0][np.ix_(free, free)]
    return x, float(np.min(np.linalg.eigvalsh(-H))), float(np.max(np.abs(tgt.value_grad(x[None, :])[1][0][free])))


@lru_cache(maxsize=None)
def optimum(name, i):
    prob, ex, tgt = case(name)
    return optimum_of(prob, ex, tgt, model(name)[i])


def margins_of(runs):
    return {k: min(r.margins[k] for r in runs) for k in ("armijo", "flat", "wolfe", "curv", "wall", "gtol")}


def value_rounding_bound(name, pts):
    """dM[M] of tests/grad_reference.py at the points: u sum_n |a amp alpha_n f_n| (E + N - 1 + c A) + u (|Mu| + |folded mean|), the
    bound on the rounding of ONE fp64 evaluation of the affine-mapped GP mean, whatever the order of its sum.  For the cases
    without a y map and without a normal prior (where the log-probability IS that mean); None for the others."""
    import grad_reference as gr
    import hess_reference as hr
    prob, ex, _ = case(name)
    if ex.get("ymap") is not None or ex.get("prior") is not None:
        return None
    X, al, amp, inv_len, mean, family, la = hr.problem_inputs(prob)
    affine = ex.get("affine", (1.0, 0.0))
    pts = np.atleast_2d(pts)
    lpg = gr.log_prob_gradient(X, al, amp, inv_len, pts, mean, family, la, affine=affine)
    A = hr.ksr.arg_difference(X, inv_len, pts, family, la)
    Mf = np.abs(np.asarray(lpg["M_aff"]).astype(np.float64))
    return hr.ksr.tolerance(lpg["vterms"], A, hr.ksr.E_FAMILY[family] + 1, hr.ksr.c_difference(prob.d, family), al, abs(affine[0]) * amp) + \
        hr.U * (Mf + abs(affine[0] * mean + affine[1]))
