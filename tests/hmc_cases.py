"""Cases and NumPy model runs shared by tests/test_hmc_move_host.py (which checks on the CPU that every run is honest: no near
tie, all three outcomes, a surrogate that varies) and tests/test_gpu_hmc_move.py (which compares the device with them).  No GPU is
touched here.  A model run is computed once per process and shared: the results are not to be modified."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import gaussian_move_cases as gc
import hmc_numpy as hm
import moves_shapes_common as ms

HALF_WIDTH = 2.9            # walkers start in uniform(-2.9, 2.9) about the centre of the box [-3, 3]^d: some sit at the walls
W_STEP, STEP_N = 16, 20
CHAIN_STEPS, CONT_STEPS, THIN = 60, 10, 3

DIMS = (1, 2, 3, 7, 10, 16, 17, 33, 64)
GRID = tuple((d, k) for d in DIMS for k in ("ExpSquared", "Matern52")) + tuple((d, k) for d in (3, 17, 64)
                                                                               for k in ("Matern32", "RationalQuadratic"))
STEP_CASES = tuple((d, k, L) for d, k in GRID for L in (1, 3))

# Seeds.  A case's seed is 100 + d unless it is listed here; NOTES.md ("HMC move") records the search.
SEEDS = {}


def case_seed(*key):
    return SEEDS.get(key, 100 + key[1])


def extras(d):
    """What makes a problem of moves_shapes_common reject inside the box under HMC: up to d = 3 the bare surrogate does; from
    d = 4 to 10 the log-probability is sharpened by logp_affine = ms.AFFINE (scale 2.5); from d = 16 on the surrogate is too flat
    for either, and a normal prior N(0, 0.5^2) on the coordinates 0 ... d - 3 (the last two left free) does it."""
    if d <= 3:
        return dict(affine=(1.0, 0.0), prior=None)
    if d <= 10:
        return dict(affine=ms.AFFINE, prior=None)
    pm, ps = np.full(d, np.nan), np.full(d, np.nan)
    pm[:d - 2], ps[:d - 2] = 0.0, 0.5
    return dict(affine=(1.0, 0.0), prior=(pm, ps))


def sampler_kw(ex):
    """EnsembleSampler keywords of an ``extras`` dict (also those of EXTRA_TARGETS)."""
    kw = {}
    if ex.get("affine", (1.0, 0.0)) != (1.0, 0.0):
        kw["logp_affine"] = ex["affine"]
    if ex.get("prior") is not None:
        kw["normal_prior"] = ex["prior"]
    if ex.get("ymap") is not None:
        kw["logp_map"] = ex["ymap"]
    return kw


def step_size(d, L):
    """1.6 / sqrt(d) where the bare or sharpened surrogate is the target; under the N(0, 0.5^2) prior 0.3 for MALA, 0.2 for
    longer trajectories."""
    if d <= 10:
        return 1.6 / np.sqrt(d)
    return 0.3 if L == 1 else 0.2


def cov_of(form, d):
    """A covariance of the given form: a scalar, a vector of unequal variances, or a matrix with correlation 0.3^|i - j|."""
    if form == "scalar":
        return 0.8
    var = 0.5 + 0.5 * (np.arange(d) % 3)
    if form == "vector":
        return var
    sd = np.sqrt(var)
    return sd[:, None] * 0.3 ** np.abs(np.arange(d)[:, None] - np.arange(d)[None, :]) * sd[None, :]


def start(prob, W, seed):
    return prob.off + np.random.RandomState(seed).uniform(-HALF_WIDTH, HALF_WIDTH, (W, prob.d))


def target_of(prob, ex):
    return hm.GPTarget(prob, affine=ex.get("affine", (1.0, 0.0)), ymap=ex.get("ymap"), prior=ex.get("prior"))


# ---- log_prob_grad: 32 points per problem, some outside the box, one on a training point
LPG_EXTRAS = ("tiled", "nlog", "log", "prior", "offset")


@lru_cache(maxsize=None)
def lpg_problem(name):
    """(problem, extras) of a log_prob_grad case: a (d, kernel) pair of GRID or one of LPG_EXTRAS."""
    if isinstance(name, tuple):
        return ms.problem(*name), dict(affine=(1.0, 0.0), prior=None)
    if name == "tiled":
        return gc.big_problem(5, 520), dict()
    if name in ("nlog", "log"):
        return ms.problem(5, "ExpSquared", ymap=name), dict(ymap=name)
    if name == "prior":
        return ms.problem(17, "Matern52"), dict(affine=ms.AFFINE, prior=ms.normal_prior(17))
    return ms.problem(5, "ExpSquared", offset=True), dict()


def lpg_points(prob, seed=7):
    rs = np.random.RandomState(seed + prob.d)
    pts = prob.off + rs.uniform(-2.9, 2.9, (32, prob.d))
    pts[0] = prob.X[3]                                             # on a training point
    pts[1, 0] = prob.off[0] + 3.5                                  # outside, one coordinate
    pts[2] = prob.off - 3.2                                        # outside, every coordinate
    pts[3, prob.d - 1] = prob.off[prob.d - 1] + 3.0                # on the wall: the box is open
    return pts


# ---- single steps from injected draws
def injected_draws(W, d, seed, it, eps):
    rs = np.random.RandomState(seed + it)
    return SimpleNamespace(z=rs.randn(W, d), u_acc=rs.rand(W), e=float(eps) * (1.0 if it % 2 == 0 else 1.2))


@lru_cache(maxsize=None)
def model_steps(d, kernel, L):
    """STEP_N steps from injected draws on the model: (p0, logp0, cov, extras, [(draws, coords, logp, accepted)], stats)."""
    prob = ms.problem(d, kernel)
    seed = case_seed("step", d, kernel, L)
    ex = extras(d)
    tgt = target_of(prob, ex)
    coords = start(prob, W_STEP, seed)
    logp = tgt(coords)
    grad = tgt.value_grad(coords)[1]
    cov = cov_of("vector", d)
    C, _ = hm.gm.scale_factor(cov, d)
    eps = step_size(d, L)
    p0, lp0, steps, rec = coords, logp, [], {}
    for it in range(STEP_N):
        dr = injected_draws(W_STEP, d, 1000 * seed, it, eps)
        coords, logp, grad, acc = hm.hmc_step_arrays(tgt, coords, logp, grad, C, dr.e, dr.z, L, dr.u_acc, rec)
        steps.append((dr, coords, logp, acc))
    return p0, lp0, cov, ex, steps, hm.stats(rec, tgt)


# ---- production runs with the counter-based draws
# name -> (d, kernel, W, E, moves as (cov form, step size factor, n_leapfrog, jitter, weight), N or None for ms.problem's)
# The step size of a move is factor * step_size(d, n_leapfrog).
CHAIN_CASES = {
    "d1": (1, "ExpSquared", 12, 1, (("scalar", 1.0, 3, None, 1.0),), None),
    "d2": (2, "Matern32", 12, 1, (("vector", 1.0, 1, None, 1.0),), None),
    "d5jitter": (5, "ExpSquared", 12, 1, (("vector", 1.0, 1, 1.5, 1.0),), None),
    "d17": (17, "ExpSquared", 12, 1, (("vector", 1.0, 2, None, 1.0),), None),
    "d33": (33, "RationalQuadratic", 12, 1, (("vector", 1.0, 2, None, 1.0),), None),
    "d64": (64, "ExpSquared", 12, 1, (("vector", 1.0, 2, None, 1.0),), None),
    "d64mala": (64, "Matern52", 12, 1, (("scalar", 1.0, 1, None, 1.0),), None),
    "matrix": (5, "Matern52", 12, 1, (("matrix", 1.0, 3, None, 1.0),), None),
    "two": (5, "ExpSquared", 12, 1, (("vector", 1.0, 1, None, 0.5), ("scalar", 0.7, 3, 1.3, 0.5)), None),
    "tiled": (5, "ExpSquared", 8, 1, (("vector", 1.0, 2, None, 1.0),), 520),
    "ens3": (5, "ExpSquared", 6, 3, (("vector", 1.0, 2, 1.5, 1.0),), None),
    "w1": (2, "Matern52", 1, 1, (("vector", 1.0, 2, 1.5, 1.0),), None),
}


def case_problem(name):
    d, kernel, W, E, moves, N = CHAIN_CASES[name]
    return ms.problem(d, kernel) if N is None else gc.big_problem(d, N)


def case_moves(name):
    """The model's move list [(cov, step size, n_leapfrog, jitter, weight)] of a chain case."""
    d = CHAIN_CASES[name][0]
    return [(cov_of(m[0], d), m[1] * step_size(d, m[2]), m[2], m[3], m[4]) for m in CHAIN_CASES[name][4]]


def moves_objects(spec):
    from alabi_amd.moves import HMCMove
    return [(HMCMove(m[0], step_size=m[1], n_leapfrog=m[2], jitter=m[3]), m[4]) for m in spec]


def _run(tgt, spec, p0, seed, id0=0):
    lp0 = tgt(p0)
    rec, counts = {}, {}
    chain, lp, nacc, c_end, lp_end = hm.run_hmc(tgt, p0, CHAIN_STEPS, seed, spec, logp0=lp0, id0=id0, count_moves=counts, record=rec)
    chain2, _, nacc2, _, _ = hm.run_hmc(tgt, c_end, CONT_STEPS, seed, spec, step0=CHAIN_STEPS, logp0=lp_end, id0=id0, record=rec)
    return SimpleNamespace(chain=chain, logp=lp, nacc=nacc, cont=chain2, nacc_cont=nacc2, counts=counts, stats=hm.stats(rec, tgt))


@lru_cache(maxsize=None)
def model_chain(name):
    """The model's side of a chain case: E single-ensemble runs (id0 = e W) laid side by side as the device lays its ensembles."""
    d, kernel, W, E, moves, N = CHAIN_CASES[name]
    prob = case_problem(name)
    ex = extras(d)
    tgt = target_of(prob, ex)
    seed = case_seed("chain", d, name)
    spec = case_moves(name)
    p0 = start(prob, W * E, seed)
    runs = [_run(tgt, spec, p0[e * W:(e + 1) * W], seed, id0=e * W) for e in range(E)]
    cat = lambda key, axis: np.concatenate([getattr(r, key) for r in runs], axis=axis)   # noqa: E731
    return SimpleNamespace(W=W, E=E, prob=prob, ex=ex, p0=p0, seed=seed, spec=spec, chain=cat("chain", 1), logp=cat("logp", 1),
                           nacc=cat("nacc", 0), cont=cat("cont", 1), nacc_cont=cat("nacc_cont", 0), stats=[r.stats for r in runs],
                           counts=[r.counts for r in runs])


def all_model_runs():
    """(name, stats) of every model run a GPU test compares against."""
    for c in STEP_CASES:
        yield ("step",) + c, model_steps(*c)[5]
    for name in CHAIN_CASES:
        for e, st in enumerate(model_chain(name).stats):
            yield ("chain", name, e), st
