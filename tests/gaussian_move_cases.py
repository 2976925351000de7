"""Cases and NumPy model runs shared by tests/test_gaussian_move_host.py (which checks on the CPU that every run is honest: no
near tie, all three outcomes, a surrogate that varies) and tests/test_gpu_gaussian_move.py (which compares the device with them).
No GPU is touched here.  A model run is computed once per process and shared: the results are not to be modified."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import gaussian_move_numpy as gm
import moves_shapes_common as ms
from conftest import make_problem
from oracle.gp_oracle import OracleGP

HALF_WIDTH = 2.9            # walkers start in uniform(-2.9, 2.9) about the centre of the box [-3, 3]^d: some sit at the walls

# Seeds.  A case's seed is 100 + d unless it is listed here; NOTES.md ("Gaussian and MH moves") records the search.
SEEDS = {("step", 2, 1, "vector", "random", "Matern52"): 104}     # one walker, 20 proposals: 102 rejects nothing inside the box, 103 never leaves it


def case_seed(*key):
    return SEEDS.get(key, 100 + key[1])


def sigma(d, mode):
    """Proposal scale per coordinate: a whole-vector move shrinks with the dimension, a one-coordinate move does not."""
    return 0.9 / np.sqrt(d) if mode == "vector" else 0.9


def cov_of(form, d, mode):
    """A covariance of the given form: a scalar, a vector of unequal variances, or a matrix with correlation 0.3^|i - j|."""
    s2 = sigma(d, mode) ** 2
    if form == "scalar":
        return s2
    var = s2 * (0.5 + 0.5 * (np.arange(d) % 3))
    if form == "vector":
        return var
    sd = np.sqrt(var)
    return sd[:, None] * 0.3 ** np.abs(np.arange(d)[:, None] - np.arange(d)[None, :]) * sd[None, :]


def start(prob, W, seed):
    return prob.off + np.random.RandomState(seed).uniform(-HALF_WIDTH, HALF_WIDTH, (W, prob.d))


# ---- item 1: single steps from injected draws: (d, W, cov form, mode, kernel)
STEP_N = 20
STEP_CASES = ((1, 4, "scalar", "vector", "ExpSquared"), (2, 1, "vector", "random", "Matern52"),
              (5, 12, "matrix", "vector", "ExpSquared"), (5, 12, "vector", "sequential", "Matern32"),
              (5, 4, "scalar", "random", "Matern52"), (5, 33, "vector", "vector", "RationalQuadratic"),
              (16, 33, "matrix", "vector", "ExpSquared"),
              (17, 12, "matrix", "vector", "ExpSquared"), (17, 12, "vector", "random", "Matern32"),
              (17, 4, "scalar", "sequential", "Matern52"), (17, 33, "vector", "vector", "RationalQuadratic"),
              (33, 12, "vector", "sequential", "ExpSquared"),
              (64, 33, "matrix", "vector", "Matern52"), (64, 4, "scalar", "random", "ExpSquared"))


def injected_draws(W, d, mode, seed, it):
    rs = np.random.RandomState(seed + it)
    inds = np.arange(W) % 2; rs.shuffle(inds)
    ids = np.arange(W)
    order = np.concatenate([ids[inds == 0], ids[inds == 1]]).astype(np.int32); n0 = int((inds == 0).sum())
    u_acc = rs.rand(W)
    z = rs.randn(W, d)
    coord = {"vector": np.full(W, -1), "random": rs.randint(0, d, size=W), "sequential": np.full(W, it % d)}[mode].astype(np.int32)
    return SimpleNamespace(order=order, n0=n0, u_acc=u_acc, z=z, coord=coord, f=1.0 if it % 2 == 0 else 1.3)


@lru_cache(maxsize=None)
def model_steps(d, W, form, mode, kernel):
    """STEP_N steps from injected draws on the model: (p0, logp0, cov, [(draws, coords, logp, accepted)], stats)."""
    prob = ms.problem(d, kernel)
    seed = case_seed("step", d, W, form, mode, kernel)
    model = ms.BoxModel(prob)
    coords = start(prob, W, seed)
    logp = model(coords)
    model.reset()
    cov = cov_of(form, d, mode)
    C, diagonal = gm.scale_factor(cov, d)
    p0, lp0, steps, margins = coords, logp, [], []
    for it in range(STEP_N):
        dr = injected_draws(W, d, mode, 1000 * seed, it)
        coords, logp, acc, _ = gm.gaussian_step_arrays(coords, logp, dr.order, dr.n0, C, dr.f, dr.coord, dr.z, dr.u_acc, model,
                                                       margin_out=margins, diagonal=diagonal)
        steps.append((dr, coords, logp, acc))
    return p0, lp0, cov, steps, ms.stats(margins, model)


# ---- items 2 to 6: production runs with the counter-based draws
CHAIN_STEPS, CONT_STEPS, THIN = 60, 10, 3


def spec_of(d, *moves):
    """Model move list from (form, mode, factor, weight) items (Gaussian) or ready model items (red-blue moves)."""
    return tuple(("gauss", cov_of(m[0], d, m[1]), m[1], m[2], m[3]) if m[0] in ("scalar", "vector", "matrix") else m for m in moves)


def moves_objects(spec):
    """A model move list as alabi_amd.moves objects."""
    from alabi_amd.moves import GaussianMove
    out = []
    for m in spec:
        if m[0] == "gauss":
            out.append((GaussianMove(m[1], mode=m[2], factor=m[3]), m[4]))
        else:
            out.extend(ms.moves_objects([m]))
    return out


def _run(prob, spec, p0, nsteps, seed, post=None, cont=0, id0=0):
    model = ms.BoxModel(prob, post)
    lp0 = model(p0)
    model.reset()
    margins, counts = [], {}
    chain, lp, nacc, c_end, lp_end = gm.run_ensemble_moves(p0, nsteps, model, seed=seed, moves=list(spec), logp0=lp0, id0=id0,
                                                           count_moves=counts, margin_out=margins)
    chain2 = nacc2 = None
    if cont:
        chain2, _, nacc2, _, _ = gm.run_ensemble_moves(c_end, cont, model, seed=seed, moves=list(spec), step0=nsteps, logp0=lp_end,
                                                       id0=id0, margin_out=margins)
    return SimpleNamespace(p0=p0, seed=seed, chain=chain, logp=lp, nacc=nacc, cont=chain2, nacc_cont=nacc2, counts=counts,
                           stats=ms.stats(margins, model), prob=prob, spec=spec)


@lru_cache(maxsize=None)
def big_problem(d, N):
    """ms.problem with N training points: the training set that does not fit the workgroup's registers."""
    X, y, h = make_problem(N, d, 1000 + d, log_wn=-9.0, ell2=4.0 * d)
    o = OracleGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel="ExpSquaredKernel", log_alpha=1.0).compute(X)
    return SimpleNamespace(d=d, N=N, X=X, y=y, h=h, off=np.zeros(d), bounds=np.stack([np.full(d, -3.0), np.full(d, 3.0)], axis=1),
                           oracle=o, kernel_name="ExpSquaredKernel", log_alpha=1.0)


# name -> (d, kernel, W, moves as (form, mode, factor, weight), N or None for ms.problem's)
# The workgroup has 256 lanes for every dimension bucket (alabi_ens::threads at Npad / 2 <= 1024), a lane keeps one pair of
# points, so Npad = 512 is the resident limit: N = 520 (Npad = 576) streams a second tile, in the <= 16 buckets (d = 5) and
# above them (d = 17).  alabi_ens_mh_plan reports the tiled route and the GPU test asserts it.
CHAIN_CASES = {
    "d1": (1, "ExpSquared", 4, (("scalar", "vector", None, 1.0),), None),
    "d2": (2, "Matern32", 7, (("vector", "random", None, 1.0),), None),
    "d17": (17, "ExpSquared", 12, (("matrix", "vector", None, 1.0),), None),
    "d33": (33, "RationalQuadratic", 12, (("vector", "sequential", None, 1.0),), None),
    "d64": (64, "Matern52", 6, (("matrix", "vector", None, 1.0),), None),
    "two": (5, "ExpSquared", 12, (("matrix", "vector", None, 0.6), ("vector", "random", None, 0.4)), None),
    "factor": (5, "Matern52", 12, (("scalar", "vector", 2.0, 1.0),), None),
    "d64two": (64, "ExpSquared", 4, (("vector", "vector", None, 0.5), ("scalar", "random", None, 0.5)), None),   # 64 KB of factors in LDS
    "w1": (2, "Matern52", 1, (("vector", "vector", 1.5, 1.0),), None),        # one walker: alabi_ens_create_metropolis
    "w300": (2, "ExpSquared", 300, (("vector", "vector", None, 1.0),), None),
    "tiled5": (5, "ExpSquared", 8, (("matrix", "vector", None, 1.0),), 520),
    "tiled17": (17, "ExpSquared", 8, (("vector", "vector", None, 1.0),), 520),
}
ENS_CASE = (5, "ExpSquared", 6, 3, (("vector", "vector", 1.5, 0.5), ("scalar", "sequential", None, 0.5)))   # d, kernel, W, E, moves


def case_problem(name):
    d, kernel, W, moves, N = CHAIN_CASES[name]
    return ms.problem(d, kernel) if N is None else big_problem(d, N)


@lru_cache(maxsize=None)
def model_chain(name):
    d, kernel, W, moves, N = CHAIN_CASES[name]
    prob = case_problem(name)
    seed = case_seed("chain", d, name)
    return _run(prob, spec_of(d, *moves), start(prob, W, seed), CHAIN_STEPS, seed, cont=CONT_STEPS)


@lru_cache(maxsize=None)
def model_ensembles():
    """E single-ensemble model runs (id0 = e W) of the n_ensembles case."""
    d, kernel, W, E, moves = ENS_CASE
    prob = ms.problem(d, kernel)
    seed = case_seed("ens", d)
    p0 = start(prob, W * E, seed)
    return p0, seed, [_run(prob, spec_of(d, *moves), p0[e * W:(e + 1) * W], CHAIN_STEPS, seed, cont=CONT_STEPS, id0=e * W)
                      for e in range(E)]


EXTRAS = ((4, "prior"), (17, "prior"), (5, "nlog"), (5, "log"), (5, "offset"))


@lru_cache(maxsize=None)
def model_extras(d, which):
    """A Gaussian run under a fused extra, as ms.model_extras has them for the red-blue moves: "prior" (normal prior on
    ms.PRIOR_DIMS plus logp_affine), "nlog" / "log" (the non-affine y maps), "offset" (inputs far from the origin)."""
    from scipy.stats import norm
    W = 12
    seed = case_seed("extra", d, which)
    if which == "prior":
        prob = ms.problem(d, "ExpSquared")
        pm, ps = ms.normal_prior(d)

        def post(mu, q):
            v = ms.AFFINE[0] * mu + ms.AFFINE[1]
            for k in ms.PRIOR_DIMS[d]:
                v = v + norm.logpdf(q[:, k], pm[k], ps[k])
            return v
    elif which == "offset":
        prob, post = ms.problem(d, "ExpSquared", offset=True), None
    else:
        prob = ms.problem(d, "ExpSquared", ymap=which)
        sign = -1.0 if which == "nlog" else 1.0
        post = lambda mu, q: sign * 10.0 ** mu  # noqa: E731
    return _run(prob, spec_of(d, ("matrix", "vector", None, 1.0)), start(prob, W, seed), CHAIN_STEPS, seed, post=post)


MIX = (("vector", "vector", None, 0.5), ("stretch", 2.0, 0.3), ("de", 1e-5, None, 0.2))
MIX_DIMS = (5, 17)


@lru_cache(maxsize=None)
def model_mixture(d):
    prob = ms.problem(d, "ExpSquared")
    seed = case_seed("mix", d)
    return _run(prob, spec_of(d, *MIX), start(prob, 12, seed), CHAIN_STEPS, seed)


def all_model_runs():
    """(name, stats) of every model run a GPU test compares against."""
    for c in STEP_CASES:
        yield ("step",) + c, model_steps(*c)[4]
    for name in CHAIN_CASES:
        yield ("chain", name), model_chain(name).stats
    for e, r in enumerate(model_ensembles()[2]):
        yield ("ens", e), r.stats
    for d, which in EXTRAS:
        yield ("extra", d, which), model_extras(d, which).stats
    for d in MIX_DIMS:
        yield ("mix", d), model_mixture(d).stats
