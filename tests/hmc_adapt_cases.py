"""Cases and NumPy model runs shared by tests/test_hmc_adapt_host.py (which checks on the CPU that every run is honest and that the
acceptance statistic covers its range) and tests/test_gpu_hmc_adapt.py (which compares the device with them).  The problems, extras,
starts and covariance forms are tests/hmc_cases.py's; no GPU is touched here.  A model run is computed once per process and shared:
the results are not to be modified."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import hmc_adapt_numpy as han
import hmc_cases as hc
import hmc_numpy as hm
import moves_shapes_common as ms

ADAPT_STEPS = 40
PAR = han.DEFAULT_PAR

# name -> (d, kernel, W, E, (cov form, n_leapfrog, jitter), N or None for ms.problem's); the start step size is hc.step_size(d, L)
CASES = {name: hc.CHAIN_CASES[name][:4] + ((hc.CHAIN_CASES[name][4][0][0],) + hc.CHAIN_CASES[name][4][0][2:4], hc.CHAIN_CASES[name][5])
         for name in ("d1", "d5jitter", "d17", "d33", "d64", "matrix", "tiled", "ens3", "w1")}

# Seeds.  A case's seed is 100 + d unless it is listed here; NOTES.md ("HMC warm-up") records the search.
SEEDS = {"w1": 201, "d1": 214, "matrix": 238}


def case_seed(name):
    return SEEDS.get(name, 100 + CASES[name][0])


def case_problem(name):
    d, kernel, W, E, mv, N = CASES[name]
    return ms.problem(d, kernel) if N is None else hc.gc.big_problem(d, N)


def case_move(name):
    """The model's move (cov, step size, n_leapfrog, jitter, weight) of a case."""
    d, _, _, _, (form, L, jitter), _ = CASES[name]
    return (hc.cov_of(form, d), hc.step_size(d, L), L, jitter, 1.0)


@lru_cache(maxsize=None)
def model_run(name):
    """ADAPT_STEPS warm-up steps of a case on the model from the initial state, with the state in front of every step (``trace``)
    for the stepwise comparison."""
    d, kernel, W, E, mv, N = CASES[name]
    prob = case_problem(name)
    ex = hc.extras(d)
    tgt = hc.target_of(prob, ex)
    seed = case_seed(name)
    move = case_move(name)
    p0 = hc.start(prob, W * E, seed)
    state0 = han.initial_state(W * E, move[1])
    rec, trace = {}, []
    r = han.run_hmc_adapt(tgt, p0, ADAPT_STEPS, seed, move, PAR, state0, nwalkers=W, record=rec, trace=trace)
    return SimpleNamespace(name=name, W=W, E=E, d=d, prob=prob, ex=ex, seed=seed, move=move, p0=p0, logp0=tgt(p0), state0=state0, run=r,
                           trace=trace, stats=hm.stats(rec, tgt))


def rounding_sensitivity(name, trials=3):
    """How far ln e, ln e-bar and the sums of the acceptance statistic of a case's free run move when the start is perturbed by
    1e-15 relative (the size of a rounding error): adaptation feeds a step's error into every later trajectory of the walker, so a
    free run compares with another implementation only where this stays small."""
    r = model_run(name)
    tgt = hc.target_of(r.prob, r.ex)
    worst = 0.0
    for k in range(trials):
        p = r.p0 * (1.0 + 1e-15 * np.random.RandomState(k).randn(*r.p0.shape))
        q = han.run_hmc_adapt(tgt, p, ADAPT_STEPS, r.seed, r.move, PAR, r.state0, nwalkers=r.W, logp0=r.logp0)
        worst = max(worst, np.max(np.abs(q.state[:, 2:4] - r.run.state[:, 2:4])), np.max(np.abs(q.alpha.sum(axis=0) - r.run.alpha.sum(axis=0))))
    return float(worst)


def alpha_cover(alpha):
    """How many acceptance statistics are exactly 0, strictly inside (0, 1), exactly 1."""
    a = np.asarray(alpha).ravel()
    return int(np.sum(a == 0.0)), int(np.sum((a > 0.0) & (a < 1.0))), int(np.sum(a == 1.0))


# ---- the whole warm-up on the surrogate problem of the end-to-end GPU test
E2E = SimpleNamespace(d=5, kernel="ExpSquared", W=16, nwarmup=300, nrun=200, n_leapfrog=4, seeds=(11, 12, 13), seed=11)


def e2e_problem():
    prob = ms.problem(E2E.d, E2E.kernel)
    return prob, dict(affine=ms.AFFINE, prior=None)


def e2e_move():
    return (1.0, None, E2E.n_leapfrog, None, 1.0)      # identity cov, the default step size d ** -0.25


def e2e_start(prob, seed):
    return prob.off + np.random.RandomState(seed).uniform(-1.0, 1.0, (E2E.W, prob.d))


@lru_cache(maxsize=None)
def e2e_model(seed):
    """The model's warm-up and the acceptance fraction of its next E2E.nrun steps."""
    prob, ex = e2e_problem()
    tgt = hc.target_of(prob, ex)
    mv = e2e_move()
    mv = (mv[0], hm.default_step_size(prob.d), mv[2], mv[3], mv[4])
    w = han.warmup(tgt, e2e_start(prob, seed), E2E.nwarmup, seed, mv, metric="diag")
    _, _, nacc, _, _ = hm.run_hmc(tgt, w.coords, E2E.nrun, seed, [w.move], step0=E2E.nwarmup, logp0=w.logp)
    return SimpleNamespace(warm=w, acc_frac=float(np.mean(nacc) / E2E.nrun))
