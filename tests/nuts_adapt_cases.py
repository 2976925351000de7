"""Cases and NumPy model runs shared by tests/test_nuts_adapt_host.py (which checks on the CPU that every run is honest) and
tests/test_gpu_nuts_adapt.py (which compares the device with them).  Built on tests/hmc_cases.py and tests/nuts_cases.py (problems,
targets, starts, covariance forms, the ``divergent`` construction, the seed rule); no GPU is touched here.  A model run is computed
once per process and shared: the results are not to be modified."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import hmc_cases as hc
import hmc_numpy as hm
import moves_shapes_common as ms
import nuts_adapt_numpy as nan_
import nuts_cases as nc
import nuts_numpy as nn

ADAPT_STEPS = 40
PAR = nan_.DEFAULT_PAR

# name -> (d, kernel, W, E, cov form, max_depth, jitter, N or None for ms.problem's).  The start step size is nuts_cases.step_size(d)
# (DIVERGENT_STEP for "divergent").  The project's kernel families are the squared exponential, Matern 3/2, Matern 5/2 and the
# rational quadratic; the last three run the GENERIC instantiations, "m32" and "rq" are the two that no other case covers.
CASES = {
    "d1": (1, "ExpSquared", 6, 1, "scalar", 3, None, None),
    "d5m52": (5, "Matern52", 6, 1, "matrix", 3, None, None),          # dense cov
    "d10": (10, "ExpSquared", 4, 1, "vector", 3, None, None),
    "d24": (24, "ExpSquared", 4, 1, "vector", 3, None, None),         # a part of the tree waits in scratch
    "d64": (64, "ExpSquared", 4, 1, "vector", 2, None, None),
    "m32": (3, "Matern32", 6, 1, "vector", 3, None, None),
    "rq": (3, "RationalQuadratic", 6, 1, "vector", 3, None, None),
    "ens3": (5, "ExpSquared", 4, 3, "vector", 3, 1.5, None),          # three ensembles, each with its own jitter draw
    "tiled": (5, "ExpSquared", 4, 1, "vector", 3, None, 520),         # a lane takes more than one training point
    "w1": (2, "Matern52", 1, 1, "vector", 3, 1.5, None),
    "divergent": (3, "ExpSquared", 8, 1, "unit", 2, None, None),      # a_t with a zero leaf; max_depth: see below
}
# max_depth of "divergent".  nuts_cases' construction makes the leapfrog map unstable along coordinate 0 on purpose: at the start
# step e = 0.06 against the prior's 0.02 the map's multiplier there is l = 1 - 4.5 - sqrt(3.5^2 - 1) = -6.85 per leaf (and dual
# averaging starts its iterates above e), so a rounding error grows by |l|^leaves within a tree: 6.85^15 = 3e12 at max_depth 4,
# 6.85^3 = 3e2 at max_depth 2.  A single transition carries that (its points of any weight are the first few leaves), but a free run
# of 40 transitions feeds it back through the adapted step size, and two fp64 implementations that agree to 1e-13 per transition
# cannot stay within 1e-6 of each other at max_depth 4 -- on an MI355X seeds 103 ... 903 gave |ln e| differences of 2e-6 to 1e-1
# there, every count but two identical (NOTES.md "NUTS warm-up").  Two doublings keep what the case is for -- the energy error
# passes -1000 within three leaves (0.5 x 47^3), so transitions end in a divergent leaf that counts with a = 0 beside leaves with
# a > 0 -- at an amplification the comparison can carry.

# Seeds.  A case's seed is the first of 100 + d, 200 + d, ... whose model run (the free run, which the single transitions are
# taken from) is honest: nuts_numpy.honesty(rec, ms.MIN_MARGIN)["ok"] -- and whose free run the device follows within the cap of
# tests/test_gpu_nuts_adapt.py.  Every default seed is honest; one was moved on by the cap's rule after the first run on an MI355X
# (NOTES.md "NUTS warm-up" has the figures): "d5m52", where ln e was off by 2.3e-7 at seed 105, which would have put FREE_TOL past
# 1e-6.
SEEDS = {"d5m52": 205}

# ---- the step-size search: name -> (case whose problem, start and seed it takes, table, k_move, ln e in)
#   "hmc": an all-HMC table of two moves, the search on the second
SEARCH_CASES = {
    "d5m52": ("d5m52", "nuts", 0, None),
    "d24": ("d24", "nuts", 0, None),
    "ens3": ("ens3", "nuts", 0, float(np.log(1e-3))),
    "hmc": ("d10", "hmc", 1, float(np.log(20.0))),
    "cap": ("m32", "nuts", 0, float(np.log(1e-20))),                  # 40 doublings later dH is still 0: the cap
}
SEARCH_STEP = 5        # the global step whose counter the search reads


def case_seed(name):
    return SEEDS.get(name, 100 + CASES[name][0])


def case_problem(name):
    d, kernel, W, E, form, depth, jitter, N = CASES[name]
    return ms.problem(d, kernel) if N is None else hc.gc.big_problem(d, N)


def case_extras(name):
    d = CASES[name][0]
    return nc._divergent_extras(d) if name == "divergent" else hc.extras(d)


def case_move(name):
    """The model's move (cov, step size, max_depth, jitter, weight) of a case."""
    d, _, _, _, form, depth, jitter, _ = CASES[name]
    return (nc._cov(form, d), nc.DIVERGENT_STEP if name == "divergent" else nc.step_size(d), depth, jitter, 1.0)


def _model_run(name, seed):
    d, kernel, W, E, form, depth, jitter, N = CASES[name]
    prob = case_problem(name)
    ex = case_extras(name)
    tgt = hc.target_of(prob, ex)
    move = case_move(name)
    p0 = nc._start(prob, W * E, seed, name)
    state0 = nan_.han.initial_state(W * E, move[1])
    rec, trace = {}, []
    r = nan_.run_nuts_adapt(tgt, p0, ADAPT_STEPS, seed, move, PAR, state0, nwalkers=W, rec=rec, trace=trace)
    return SimpleNamespace(name=name, W=W, E=E, d=d, prob=prob, ex=ex, seed=seed, move=move, p0=p0, logp0=tgt(p0), state0=state0, run=r,
                           trace=trace, rec=rec)


@lru_cache(maxsize=None)
def model_run(name):
    """ADAPT_STEPS warm-up transitions of a case on the model from the initial state, with the state in front of every transition
    (``trace``) for the stepwise comparison and the record of every decision's margin."""
    return _model_run(name, case_seed(name))


def find_seed(name, tries=8):
    """The seed rule: the first of 100 + d, 200 + d, ... whose model run is honest (run when the cases change; SEEDS holds the
    outcome)."""
    for k in range(tries):
        seed = 100 * (k + 1) + CASES[name][0]
        if nan_.honesty(_model_run(name, seed).rec, ms.MIN_MARGIN)["ok"]:
            return seed
    raise AssertionError(f"no honest seed for {name}")


def search_tables(name):
    """(problem, extras, model moves, k_move, ln e in, W, E, seed, p0) of a search case."""
    base, table, k_move, ln_e = SEARCH_CASES[name]
    d, kernel, W, E, form, depth, jitter, N = CASES[base]
    if table == "nuts":
        moves = [case_move(base)]
    else:
        moves = [(hc.cov_of("scalar", d), 0.3, 2, None, 0.5), (hc.cov_of("vector", d), 0.2, 3, 1.3, 0.5)]
    ln_e = float(np.log(moves[k_move][1])) if ln_e is None else ln_e
    seed = case_seed(base)
    return SimpleNamespace(prob=case_problem(base), ex=case_extras(base), table=table, moves=moves, k_move=k_move, ln_e=ln_e, W=W, E=E,
                           d=d, seed=seed, p0=nc._start(case_problem(base), W * E, seed, base))


@lru_cache(maxsize=None)
def model_search(name):
    """The model's search of a search case: ln e out, iters, and the record of every comparison's margin."""
    c = search_tables(name)
    tgt = hc.target_of(c.prob, c.ex)
    C = hm.gm.scale_factor(c.moves[c.k_move][0], c.d)[0]
    logp0 = tgt(c.p0)
    n = c.W * c.E
    rec = {}
    ln_e, iters = nan_.find_step_size(tgt, c.p0, logp0, C, np.full(n, c.ln_e), c.seed, SEARCH_STEP, rec=rec)
    return SimpleNamespace(case=c, logp0=logp0, ln_e=ln_e, iters=iters, rec=rec)


def all_model_runs():
    """(name, record) of every model run a GPU test compares against."""
    for name in CASES:
        yield ("adapt", name), model_run(name).rec
    for name in SEARCH_CASES:
        yield ("search", name), model_search(name).rec


# ---- the whole warm-up on the surrogate problem of test_tune_hmc_end_to_end (hmc_adapt_cases.E2E)
E2E = SimpleNamespace(d=5, kernel="ExpSquared", W=16, nwarmup=300, nrun=100, max_depth=6, seeds=(11, 12, 13, 14, 15), seed=11)


# The terminal buffer's mean acceptance statistic of the model over E2E.seeds: 0.7698, 0.7719, 0.7677, 0.7721, 0.7673 (NOTES.md
# "NUTS warm-up"); the band is that range widened by its own spread (0.0048) on either side.
E2E_BAND = (0.7673 - 0.0048, 0.7721 + 0.0048)


def e2e_problem():
    prob = ms.problem(E2E.d, E2E.kernel)
    return prob, dict(affine=ms.AFFINE, prior=None)


def e2e_move():
    return (1.0, None, E2E.max_depth, None, 1.0)       # identity cov, the default step size d ** -0.25


def e2e_start(prob, seed):
    return prob.off + np.random.RandomState(seed).uniform(-1.0, 1.0, (E2E.W, prob.d))


@lru_cache(maxsize=None)
def e2e_model(seed):
    prob, ex = e2e_problem()
    tgt = hc.target_of(prob, ex)
    mv = e2e_move()
    mv = (mv[0], hm.default_step_size(prob.d), mv[2], mv[3], mv[4])
    return nan_.warmup(tgt, e2e_start(prob, seed), E2E.nwarmup, seed, mv, metric="diag", search=True)
