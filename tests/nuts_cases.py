"""Cases and NumPy model runs shared by tests/test_nuts_move_host.py (which checks on the CPU that every run is honest: no
comparison near a tie, no U-turn product near zero, no leaf at a wall, no energy error near the divergence bound) and
tests/test_gpu_nuts_move.py (which compares the device with them).  Built on tests/hmc_cases.py's problems, targets and starts.
No GPU is touched here.  A model run is computed once per process and shared: the results are not to be modified."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import hmc_cases as hc
import hmc_numpy as hm
import moves_shapes_common as ms
import nuts_numpy as nn

W_STEP, STEP_N, STEP_DEPTH = 8, 6, 3
CHAIN_STEPS, CONT_STEPS, THIN = 40, 10, 3

GRID = hc.GRID

# Seeds.  A case's seed is 100 + d unless it is listed here; a listed seed would be the first of 100 + d, 200 + d, ... whose model
# run meets every margin condition of nuts_numpy.honesty.  The search on the CPU found every default seed to meet them, so none
# is listed (NOTES.md, "NUTS move", has the closest calls).
SEEDS = {}


def case_seed(*key):
    return SEEDS.get(key, 100 + key[1])


def step_size(d):
    """hmc_cases.step_size of a three-step trajectory: 1.6 / sqrt(d) up to d = 10, 0.2 under the N(0, 0.5^2) prior beyond."""
    return float(hc.step_size(d, 3))


# ---- single transitions from injected draws
def injected_draws(W, d, seed, it, eps, depth):
    rs = np.random.RandomState(seed + it)
    return SimpleNamespace(z=rs.randn(W, d), dirw=rs.randint(0, 1 << 32, size=W, dtype=np.uint64).astype(np.uint32),
                           u_leaf=rs.rand(W, (1 << depth) - 1), u_tree=rs.rand(W, depth), e=float(eps) * (1.0 if it % 2 == 0 else 1.2))


# name -> (d, kernel, cov form, max_depth, step size, extras or None for hmc_cases.extras(d), start)
def _divergent_extras(d):
    pm, ps = np.full(d, np.nan), np.full(d, np.nan)
    pm[0], ps[0] = 0.0, 0.02
    return dict(affine=(1.0, 0.0), prior=(pm, ps))


DIVERGENT_STEP = 0.06       # C = I: e sqrt(1 / 0.02^2) = 3 > 2, the leapfrog map is unstable along coordinate 0
EXTRA_STEP_CASES = {
    "matrix": (5, "Matern52", "matrix", 3, step_size(5), None),
    "depth1": (3, "ExpSquared", "vector", 1, step_size(3), None),
    "divergent": (3, "ExpSquared", "unit", 4, DIVERGENT_STEP, _divergent_extras(3)),
    "depth5": (2, "ExpSquared", "vector", 5, 0.25, None),
}


def _cov(form, d):
    return 1.0 if form == "unit" else hc.cov_of(form, d)


def step_case(name):
    """(d, kernel, cov, max_depth, e, extras) of a step case: a (d, kernel) pair of GRID or a name of EXTRA_STEP_CASES."""
    if isinstance(name, tuple):
        d, kernel = name
        return d, kernel, hc.cov_of("vector", d), STEP_DEPTH, step_size(d), hc.extras(d)
    d, kernel, form, depth, eps, ex = EXTRA_STEP_CASES[name]
    return d, kernel, _cov(form, d), depth, eps, hc.extras(d) if ex is None else ex


def _start(prob, W, seed, name):
    p0 = hc.start(prob, W, seed)
    if name == "divergent":                     # coordinate 0 starts inside its narrow prior: the orbit blows up after a few leaves
        p0[:, 0] = 0.02 * np.random.RandomState(seed + 1).randn(W)
    return p0


@lru_cache(maxsize=None)
def model_steps(name):
    """STEP_N transitions from injected draws on the model (checkpoint form): a namespace with p0, logp0, cov, depth, e, extras,
    steps [(draws, coords, logp, trace, a_sum)] and the record of every decision's margin."""
    d, kernel, cov, depth, eps, ex = step_case(name)
    prob = ms.problem(d, kernel)
    seed = case_seed("step", d, kernel, name if isinstance(name, str) else "grid")
    tgt = hc.target_of(prob, ex)
    coords = _start(prob, W_STEP, seed, name)
    logp = tgt(coords)
    grad = tgt.value_grad(coords)[1]
    C, _ = hm.gm.scale_factor(cov, d)
    p0, lp0, steps, rec = coords, logp, [], {}
    for it in range(STEP_N):
        dr = injected_draws(W_STEP, d, 1000 * seed, it, eps, depth)
        coords, logp, grad, trace, a = nn.nuts_step_arrays(tgt, coords, logp, grad, C, dr.e, dr.z, dr.dirw, dr.u_leaf, dr.u_tree, depth, rec=rec)
        steps.append((dr, coords, logp, trace, a))
    return SimpleNamespace(prob=prob, p0=p0, lp0=lp0, cov=cov, depth=depth, e=eps, ex=ex, steps=steps, rec=rec, seed=seed)


# ---- production runs with the counter-based draws
# name -> (d, kernel, W, E, moves as (cov form, step size factor, max_depth, jitter, weight), N or None for ms.problem's)
CHAIN_CASES = {
    "w1": (2, "Matern52", 1, 1, (("vector", 1.0, 3, 1.5, 1.0),), None),
    "d1": (1, "ExpSquared", 6, 1, (("scalar", 1.0, 3, None, 1.0),), None),
    "matrix": (5, "Matern52", 6, 1, (("matrix", 1.0, 3, None, 1.0),), None),
    "two": (5, "ExpSquared", 4, 3, (("vector", 1.0, 2, 1.5, 0.5), ("scalar", 0.7, 3, 1.3, 0.5)), None),
    "tiled": (5, "ExpSquared", 4, 1, (("vector", 1.0, 3, None, 1.0),), 520),
}


def case_problem(name):
    d, kernel, W, E, moves, N = CHAIN_CASES[name]
    return ms.problem(d, kernel) if N is None else hc.gc.big_problem(d, N)


def case_moves(name):
    """The model's move list [(cov, step size, max_depth, jitter, weight)] of a chain case."""
    d = CHAIN_CASES[name][0]
    return [(hc.cov_of(m[0], d), m[1] * step_size(d), m[2], m[3], m[4]) for m in CHAIN_CASES[name][4]]


def moves_objects(spec):
    from alabi_amd.moves import NUTSMove
    return [(NUTSMove(m[0], step_size=m[1], max_depth=m[2], jitter=m[3]), m[4]) for m in spec]


def _run(tgt, spec, p0, seed, id0=0, nsteps=CHAIN_STEPS, cont=CONT_STEPS):
    lp0 = tgt(p0)
    rec, counts = {}, {}
    chain, lp, nacc, c_end, lp_end, cnt, a_sum = nn.run_nuts(tgt, p0, nsteps, seed, spec, logp0=lp0, id0=id0, count_moves=counts, rec=rec)
    chain2, _, nacc2, _, _, cnt2, a_sum2 = nn.run_nuts(tgt, c_end, cont, seed, spec, step0=nsteps, logp0=lp_end, id0=id0, rec=rec)
    return SimpleNamespace(chain=chain, logp=lp, nacc=nacc, cont=chain2, nacc_cont=nacc2, counts=cnt, a_sum=a_sum, counts_cont=cnt2,
                           a_sum_cont=a_sum2, move_counts=counts, rec=rec)


@lru_cache(maxsize=None)
def model_chain(name):
    """The model's side of a chain case: E single-ensemble runs (id0 = e W) laid side by side as the device lays its ensembles."""
    d, kernel, W, E, moves, N = CHAIN_CASES[name]
    prob = case_problem(name)
    ex = hc.extras(d)
    tgt = hc.target_of(prob, ex)
    seed = case_seed("chain", d, name)
    spec = case_moves(name)
    p0 = hc.start(prob, W * E, seed)
    runs = [_run(tgt, spec, p0[e * W:(e + 1) * W], seed, id0=e * W) for e in range(E)]
    cat = lambda key, axis: np.concatenate([getattr(r, key) for r in runs], axis=axis)   # noqa: E731
    return SimpleNamespace(W=W, E=E, prob=prob, ex=ex, p0=p0, seed=seed, spec=spec, chain=cat("chain", 1), logp=cat("logp", 1),
                           nacc=cat("nacc", 0), cont=cat("cont", 1), nacc_cont=cat("nacc_cont", 0), counts=cat("counts", 0),
                           a_sum=cat("a_sum", 0), counts_cont=cat("counts_cont", 0), a_sum_cont=cat("a_sum_cont", 0),
                           recs=[r.rec for r in runs], move_counts=[r.move_counts for r in runs])


STEP_NAMES = tuple(GRID) + tuple(EXTRA_STEP_CASES)


def all_model_runs():
    """(name, record) of every model run a GPU test compares against."""
    for name in STEP_NAMES:
        yield ("step", name), model_steps(name).rec
    for name in CHAIN_CASES:
        for e, rec in enumerate(model_chain(name).recs):
            yield ("chain", name, e), rec
