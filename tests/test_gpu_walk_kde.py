"""GPU parity of the walk and KDE moves (alabi_amd.moves.WalkMove / KDEMove: wk_proposal, ens_kde_prepass_kernel and the whole-half
instantiations of the half-step and propose kernels) against tests/walk_kde_numpy.py, on the problems of
tests/moves_shapes_common.py (N = 65 / 130, length scale growing with d).  Tolerances are those of tests/test_gpu_snooker.py:
proposals bit for bit, log-probabilities and the KDE log factor to 1e-8 (1 + max|logp|), production chains to 1e-7 with
identical acceptance counts.  Every model run is asserted to be no near tie (|margin| > 1e-6) before a chain is compared with it;
a seed in SEEDS was chosen where the default one was."""
import ctypes as C
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import moves_shapes_common as ms
import snooker_numpy as sn
import walk_kde_numpy as wk

pytestmark = pytest.mark.gpu

WALK, WALK3, KDE = (("walk", None, 1.0),), (("walk", 3, 1.0),), (("kde", None, 1.0),)
MIX = (("de", 1e-5, None, .5), ("walk", None, .2), ("kde", None, .2), ("snooker", 1.7, .1))
SEEDS = {}


def _moves(spec):
    from alabi_amd.moves import KDEMove, WalkMove
    out = []
    for m in spec:
        if m[0] == "walk":
            out.append((WalkMove(m[1]), m[2]))
        elif m[0] == "kde":
            out.append((KDEMove(m[1]), m[2]))
        else:
            out.extend(ms.moves_objects([m]))
    return out


def _start(prob, W, seed, half_width):
    return prob.off + np.random.RandomState(seed).uniform(-half_width, half_width, (W, prob.d))


# ------------------------------------------------------------------------------------------------ injected randoms
# (d, W, s0 of a walk step | decades of a KDE step's accept uniforms, kernel, move): W = 2 d + 2, 33 (Nc 16 / 17), 257 (Nc 128 / 129);
# s0 = 2, 3 (< d) and Nc.
# KDE: the log factor is compared to the ABSOLUTE 1e-8 (1 + max|logp|), which an fp64 evaluation can meet only while |lnfac| stays
# below about 1e7 (one ulp of 1e9 is 1e-7).  With Nc = d + 1 rows the KDE's bandwidth matrix is nearly singular in some directions
# and the model's own log factors reach 1e6 at d = 17 (kept: 2e-10 of error) and 1.5e9 at d = 64, W = 130 (not a KDE step case:
# the d = 64 case has W = 257, where they stay below 250; W = 130 is in the production runs, which compare chains).  Far from
# the kernels the factor is tens to hundreds below zero, so where u' ~ U(0, 1) accepts nothing the uniforms spread over the given
# number of decades: some proposals are accepted, and show their bits, in every case.
STEP_CASES = [(1, 4, 2, "ExpSquared", "walk"), (5, 12, 2, "ExpSquared", "walk"), (5, 12, 3, "Matern52", "walk"),
              (5, 33, 16, "ExpSquared", "walk"), (17, 36, 3, "ExpSquared", "walk"), (17, 257, 128, "ExpSquared", "walk"),
              (64, 130, 3, "ExpSquared", "walk"),
              (1, 4, 0, "ExpSquared", "kde"), (5, 12, 0, "ExpSquared", "kde"), (5, 12, 0, "Matern52", "kde"), (5, 33, 0, "ExpSquared", "kde"),
              (17, 36, 10, "ExpSquared", "kde"), (17, 257, 0, "ExpSquared", "kde"), (64, 257, 40, "ExpSquared", "kde")]
STEP_N = 30


def _injected(W, d, s0, seed, it, move="walk"):
    """Labels as emcee shuffles them; per walker a subset of s0 distinct rows in RANDOM order (the sums follow the caller's
    order), or a row, and normals.  The normals are scaled by 1 / sqrt(d) so that proposals stay near the box in every dimension."""
    rs = np.random.RandomState(seed + it)
    inds = np.arange(W) % 2; rs.shuffle(inds)
    ids = np.arange(W)
    order = np.concatenate([ids[inds == 0], ids[inds == 1]]).astype(np.int32); n0 = int((inds == 0).sum())
    ncmin = W - n0
    zs = 1.0 / np.sqrt(d)
    if move == "walk":
        subset = np.array([rs.permutation(ncmin)[:s0] for _ in range(W)], dtype=np.int32)
        return SimpleNamespace(order=order, n0=n0, subset=subset, z_walk=zs * rs.randn(W, s0), u_acc=rs.rand(W))
    row, z = rs.randint(0, ncmin, W).astype(np.int32), zs * rs.randn(W, d)
    return SimpleNamespace(order=order, n0=n0, row=row, z_kde=z, u_acc=10.0 ** (-rs.uniform(0.0, s0, W)) if s0 else rs.rand(W))


@lru_cache(maxsize=None)
def model_steps(d, W, s0, kernel, move):
    prob = ms.problem(d, kernel)
    seed = SEEDS.get(("step", d, W, s0, move), 100 + d)
    model = ms.BoxModel(prob)
    coords = _start(prob, W, seed, 2.9)                       # close to the walls: some proposals leave the box
    logp = model(coords)
    model.reset()
    p0, lp0, steps, margins = coords, logp, [], []
    factor = wk.kde_factor(None, W // 2, d)
    for it in range(STEP_N):
        dr = _injected(W, d, s0, 1000 * seed, it, move)
        if move == "walk":
            coords, logp, acc, q = wk.walk_step_arrays(coords, logp, dr.order, dr.n0, dr.subset, dr.z_walk, dr.u_acc, model,
                                                       margin_out=margins)
            lnfac = None
        else:
            coords, logp, acc, q, lnfac = wk.kde_step_arrays(coords, logp, dr.order, dr.n0, factor, dr.row, dr.z_kde, dr.u_acc, model,
                                                             margin_out=margins)
        steps.append((dr, coords, logp, acc, lnfac))
    return p0, lp0, steps, ms.stats(margins, model), factor


def _dev(torch, *arrays):
    return [torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in arrays]


@pytest.mark.parametrize("d,W,s0,kernel,move", STEP_CASES)
def test_step_with_injected_randoms(d, W, s0, kernel, move):
    """Same draws -> bit-identical accepted proposals, identical accept mask, log-probabilities and the KDE log factor within
    1e-8 (1 + max|logp|), over 30 steps."""
    import torch
    from alabi_amd import _lib
    p0, lp0, steps, st, factor = model_steps(d, W, s0, kernel, move)
    assert st["min_margin"] > ms.MIN_MARGIN and st["n_acc"] >= 1 and st["n_out"] >= 1, st
    if move == "kde":                                         # the absolute tolerance is one an fp64 evaluation can meet (see STEP_CASES)
        assert max(np.max(np.abs(f)) for _, _, _, _, f in steps) < 2e7
    prob = ms.problem(d, kernel)
    s = ms.sampler(prob, W, 1)
    c_dev = torch.as_tensor(p0, device="cuda").clone()
    lp_dev = s.compute_log_prob(c_dev)
    assert np.max(np.abs(lp_dev.cpu().numpy() - lp0)) < 1e-8 * (1 + np.max(np.abs(lp0)))
    nacc = torch.zeros(W, dtype=torch.int64, device="cuda")
    lnf = torch.zeros(W, dtype=torch.float64, device="cuda")
    lib, stream = _lib.lib(), _lib.current_stream()
    coords = p0
    for it, (dr, c_o, l_o, a_o, lnfac_o) in enumerate(steps):
        if move == "walk":
            dev = _dev(torch, dr.order, dr.subset, dr.z_walk, dr.u_acc)
            rc = lib.alabi_ens_step_with_randoms_walk(s._ens, _lib.ptr(c_dev), _lib.ptr(lp_dev), _lib.ptr(dev[0]), dr.n0, s0,
                                                      _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]), _lib.ptr(nacc), stream)
        else:
            dev = _dev(torch, dr.order, dr.row, dr.z_kde, dr.u_acc)
            rc = lib.alabi_ens_step_with_randoms_kde(s._ens, _lib.ptr(c_dev), _lib.ptr(lp_dev), _lib.ptr(dev[0]), dr.n0, factor,
                                                     _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]), _lib.ptr(lnf),
                                                     _lib.ptr(nacc), stream)
        _lib.check(rc, "step_with_randoms_" + move)
        torch.cuda.synchronize()
        c_g, l_g = c_dev.cpu().numpy(), lp_dev.cpu().numpy()
        a_g = np.any(c_g != coords, axis=1)
        scale = 1 + np.max(np.abs(l_o[np.isfinite(l_o)]))
        assert np.array_equal(a_g, a_o), f"accept mask differs at iteration {it}"
        assert np.array_equal(c_g, c_o), f"proposals differ at iteration {it}"
        assert np.max(np.abs(l_g - l_o)) < 1e-8 * scale
        if move == "kde":
            assert np.max(np.abs(lnf.cpu().numpy() - lnfac_o)) < 1e-8 * scale
        coords = c_o
        lp_dev.copy_(torch.as_tensor(l_o, device="cuda"))
    assert int(nacc.sum()) == sum(int(a.sum()) for _, _, _, a, _ in steps) > 0
    assert s.kde_singular_half_steps == 0


def test_bad_subsets_and_rows_are_no_ops():
    import torch
    from alabi_amd import _lib
    d, W, s0 = 5, 12, 3
    prob = ms.problem(d, "ExpSquared")
    s = ms.sampler(prob, W, 1)
    p0 = _start(prob, W, 3, 2.0)
    c_dev = torch.as_tensor(p0, device="cuda").clone()
    lp_dev = s.compute_log_prob(c_dev)
    lp0 = lp_dev.cpu().numpy().copy()
    nacc = torch.zeros(W, dtype=torch.int64, device="cuda")
    dr = _injected(W, d, s0, 5, 0)
    dk = _injected(W, d, 0, 5, 0, "kde")
    ids = np.arange(W)
    bad = dr.subset.copy()
    bad[ids % 3 == 0, 2] = bad[ids % 3 == 0, 0]               # repeated
    bad[ids % 3 == 1, 1] = W // 2                             # beyond the complementary list
    bad[ids % 3 == 2, 0] = -1                                 # negative
    lib, stream = _lib.lib(), _lib.current_stream()
    dev = _dev(torch, dr.order, bad, dr.z_walk, np.full(W, 1e-300))
    _lib.check(lib.alabi_ens_step_with_randoms_walk(s._ens, _lib.ptr(c_dev), _lib.ptr(lp_dev), _lib.ptr(dev[0]), dr.n0, s0, _lib.ptr(dev[1]),
                                                    _lib.ptr(dev[2]), _lib.ptr(dev[3]), _lib.ptr(nacc), stream), "walk")
    rows = np.where(ids % 2 == 0, W // 2, -1).astype(np.int32)
    dev2 = _dev(torch, dr.order, rows, dk.z_kde, np.full(W, 1e-300))
    _lib.check(lib.alabi_ens_step_with_randoms_kde(s._ens, _lib.ptr(c_dev), _lib.ptr(lp_dev), _lib.ptr(dev2[0]), dr.n0, 0.7, _lib.ptr(dev2[1]),
                                                   _lib.ptr(dev2[2]), _lib.ptr(dev2[3]), None, _lib.ptr(nacc), stream), "kde")
    torch.cuda.synchronize()
    assert np.array_equal(c_dev.cpu().numpy(), p0) and np.array_equal(lp_dev.cpu().numpy(), lp0) and int(nacc.sum()) == 0


def test_library_refuses_what_the_header_says():
    import torch
    from alabi_amd import _lib
    d = 5
    prob = ms.problem(d, "ExpSquared")
    lib = _lib.lib()

    def set_moves(s, kind, p0, p1=0.0):
        return lib.alabi_ens_set_moves(s._ens, 1, (C.c_int * 1)(kind), _lib.host_doubles([1.0]), _lib.host_doubles([p0]),
                                       _lib.host_doubles([p1]))
    s = ms.sampler(prob, 11, 1); s._ensure_ens()              # halves of 6 and 5
    for p0 in (1.0, 2.5, 6.0, -2.0, np.nan):
        assert set_moves(s, 3, p0) == _lib.BAD_ARG, p0
    assert set_moves(s, 3, 5.0) == _lib.OK and set_moves(s, 3, 0.0) == _lib.OK and set_moves(s, 3, 2.0) == _lib.OK
    assert set_moves(s, 4, 0.5, 0.5) == _lib.BAD_ARG         # 5 complementary walkers in 5-D
    assert set_moves(s, 5, 1.0) == _lib.BAD_ARG
    t = ms.sampler(prob, 12, 1); t._ensure_ens()
    assert set_moves(t, 4, 0.5, 0.6) == _lib.OK
    for p0, p1 in ((0.0, 0.5), (0.5, 0.0), (np.nan, 0.5), (0.5, np.inf), (-0.5, 0.5)):
        assert set_moves(t, 4, p0, p1) == _lib.BAD_ARG, (p0, p1)
    small = ms.sampler(prob, 3, 1); small._ensure_ens()
    assert set_moves(small, 3, 0.0) == _lib.BAD_ARG          # a half of one walker
    # the test entries
    W = 12
    c = torch.zeros((W, d), dtype=torch.float64, device="cuda"); lp = torch.zeros(W, dtype=torch.float64, device="cuda")
    order = torch.arange(W, dtype=torch.int32, device="cuda")
    idx = torch.zeros((W, 8), dtype=torch.int32, device="cuda"); z = torch.zeros((W, 8), dtype=torch.float64, device="cuda")
    u = torch.full((W,), 0.5, dtype=torch.float64, device="cuda")
    walk = lambda n0, s0: lib.alabi_ens_step_with_randoms_walk(t._ens, _lib.ptr(c), _lib.ptr(lp), _lib.ptr(order), n0, s0, _lib.ptr(idx),   # noqa: E731
                                                               _lib.ptr(z), _lib.ptr(u), None, _lib.current_stream())
    kde = lambda n0, f: lib.alabi_ens_step_with_randoms_kde(t._ens, _lib.ptr(c), _lib.ptr(lp), _lib.ptr(order), n0, f, _lib.ptr(idx),        # noqa: E731
                                                            _lib.ptr(z), _lib.ptr(u), None, None, _lib.current_stream())
    assert walk(6, 1) == _lib.BAD_ARG and walk(6, 7) == _lib.BAD_ARG and walk(8, 5) == _lib.BAD_ARG and walk(13, 2) == _lib.BAD_ARG
    assert kde(6, 0.0) == _lib.BAD_ARG and kde(6, np.nan) == _lib.BAD_ARG and kde(7, 0.5) == _lib.BAD_ARG and kde(5, 0.5) == _lib.BAD_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- production runs
def _post_prior_nlog(d):
    from scipy.stats import norm
    pm, ps = ms.normal_prior(d)

    def post(mu, q):
        v = -(10.0 ** mu)
        for k in ms.PRIOR_DIMS[d]:
            v = v + norm.logpdf(q[:, k], pm[k], ps[k])
        return v
    return post


@lru_cache(maxsize=None)
def model_run(d, kernel, W, spec, nsteps, half_width, extra=None, id0=0, W_total=None):
    """The model's run at thin_by = 1 (a thinned chain is every thin-th row) and its continuation by 9 steps."""
    prob = ms.problem(d, kernel, ymap="nlog" if extra else None)
    seed = SEEDS.get(("run", d, kernel, W, spec, id0), 300 + d + W)
    post = _post_prior_nlog(d) if extra else None
    p_all = _start(prob, W_total or W, seed, half_width)
    p0 = p_all[id0:id0 + W]
    model = ms.BoxModel(prob, post)
    lp0 = model(p0)
    model.reset()
    margins, counts, sing = [], {}, []
    chain, lp, nacc, c_end, lp_end = wk.run_ensemble_moves(p0, nsteps, model, seed=seed, moves=list(spec), logp0=lp0, id0=id0,
                                                           count_moves=counts, margin_out=margins, singular_out=sing)
    cont = wk.run_ensemble_moves(c_end, 9, model, seed=seed, moves=list(spec), step0=nsteps, logp0=lp_end, id0=id0, margin_out=margins,
                                 singular_out=sing)[0]
    return SimpleNamespace(p0=p0, p_all=p_all, seed=seed, chain=chain, logp=lp, nacc=nacc, cont=cont, counts=counts, sing=sing,
                           stats=ms.stats(margins, model), prob=prob)


def _honest(run, spec):
    st = run.stats
    assert st["min_margin"] > ms.MIN_MARGIN, st
    assert st["n_acc"] >= 1 and st["n_rej_in"] + st["n_out"] >= 1, st
    assert len(run.counts) == len(spec), run.counts          # every move of the set ran
    assert run.sing == []


RUN_CASES = [  # d, kernel, W, spec, nsteps, thin, start half width
    (1, "ExpSquared", 4, WALK, 60, 1, 2.5), (1, "ExpSquared", 4, KDE, 60, 3, 2.5), (1, "ExpSquared", 6, MIX, 100, 1, 2.5),
    (5, "ExpSquared", 12, WALK, 60, 1, 2.5), (5, "ExpSquared", 12, WALK3, 60, 3, 2.5), (5, "ExpSquared", 12, KDE, 60, 1, 2.5),
    (5, "Matern32", 33, MIX, 100, 1, 2.5), (5, "ExpSquared", 33, KDE, 60, 3, 2.5), (5, "ExpSquared", 33, WALK, 60, 1, 2.5),
    (17, "ExpSquared", 36, MIX, 100, 3, 1.0), (17, "ExpSquared", 257, MIX, 40, 1, 1.0), (17, "ExpSquared", 257, WALK3, 20, 1, 1.0),
    (64, "ExpSquared", 130, MIX, 60, 1, 0.5),
]


@pytest.mark.parametrize("d,kernel,W,spec,nsteps,thin,hw", RUN_CASES,
                         ids=[f"d{c[0]}-{c[1]}-W{c[2]}-{'+'.join(m[0] + ('3' if m[1] == 3 else '') for m in c[3])}-thin{c[5]}" for c in RUN_CASES])
def test_production_run_matches_numpy_chain(d, kernel, W, spec, nsteps, thin, hw):
    """Counter-based draws (streams 6-8 where the proposal is formed) + pre-pass + whole-half kernels ==
    walk_kde_numpy.run_ensemble_moves, step for step; run_mcmc(None, n) continues the counter."""
    run = model_run(d, kernel, W, spec, nsteps, hw)
    _honest(run, spec)
    s = ms.sampler(run.prob, W, run.seed, moves=_moves(spec))
    s.run_mcmc(run.p0, nsteps, thin_by=thin)
    assert s.last_path == "launch-per-half-step"
    chain = s.get_chain()
    ref, ref_lp = run.chain[thin - 1::thin], run.logp[thin - 1::thin]
    assert chain.shape == ref.shape
    assert np.max(np.abs(chain - ref)) < 1e-7
    assert np.max(np.abs(s.get_log_prob() - ref_lp)) < 1e-7
    assert np.array_equal(s._naccept.cpu().numpy(), run.nacc)
    assert s.kde_singular_half_steps == 0
    s.run_mcmc(None, 9, thin_by=1)
    assert np.max(np.abs(s.get_chain()[-9:] - run.cont)) < 1e-7


def test_independent_ensembles():
    """n_ensembles = 3: rows [eW, (e+1)W) evolve like a stand-alone ensemble whose walker ids start at eW -- the pre-pass has one
    workgroup per ensemble, the move is chosen per ensemble."""
    d, W, E, nsteps = 5, 14, 3, 60
    runs = [model_run(d, "ExpSquared", W, MIX, nsteps, 2.5, id0=e * W, W_total=W * E) for e in range(E)]
    for r in runs:
        _honest(r, MIX)
    s = ms.sampler(runs[0].prob, W, runs[0].seed, n_ensembles=E, moves=_moves(MIX))
    s.run_mcmc(runs[0].p_all, nsteps)
    chain = s.get_chain()
    for e, r in enumerate(runs):
        assert np.max(np.abs(chain[:, e * W:(e + 1) * W] - r.chain)) < 1e-7
        assert np.array_equal(s._naccept.cpu().numpy()[e * W:(e + 1) * W], r.nacc)


def test_fused_normal_prior_and_nlog_map():
    d, W, nsteps = 4, 12, 60
    run = model_run(d, "ExpSquared", W, MIX, nsteps, 2.5, extra="prior+nlog")
    _honest(run, MIX)
    s = ms.sampler(run.prob, W, run.seed, moves=_moves(MIX), normal_prior=ms.normal_prior(d), logp_map="nlog")
    s.run_mcmc(run.p0, nsteps)
    assert np.max(np.abs(s.get_chain() - run.chain)) < 1e-7
    assert np.max(np.abs(s.get_log_prob() - run.logp)) < 1e-7 * (1 + np.max(np.abs(run.logp)))
    assert np.array_equal(s._naccept.cpu().numpy(), run.nacc)


def test_graph_and_eager_paths_agree(monkeypatch):
    prob = ms.problem(5, "ExpSquared")
    p0 = _start(prob, 24, 2, 2.0)
    monkeypatch.setenv("ALABI_ENS_GRAPH_STEPS", "16")
    a = ms.sampler(prob, 24, 5, moves=_moves(MIX)); a.run_mcmc(p0, 50)
    monkeypatch.setenv("ALABI_ENS_GRAPH", "0")
    b = ms.sampler(prob, 24, 5, moves=_moves(MIX)); b.run_mcmc(p0, 50)
    assert np.array_equal(a.get_chain(), b.get_chain())
    assert np.array_equal(a.get_log_prob(), b.get_log_prob())
    assert np.array_equal(a.acceptance_fraction, b.acceptance_fraction)
    assert 0.0 < a.acceptance_fraction.mean() < 1.0


def test_host_prior_callback_equals_fused_chain():
    """A Python prior_fn equal to the box: pre-pass -> propose kernel (which leaves the log factor in the record) -> host ->
    accept kernel gives the chain of the fused kernels."""
    from oracle.stretch_oracle import box_lnprior_batch
    prob = ms.problem(5, "ExpSquared")
    W = 24
    p0 = _start(prob, W, 12, 2.5)
    fused = ms.sampler(prob, W, 3, moves=_moves(MIX)); fused.run_mcmc(p0, 60)
    host = ms.sampler(prob, W, 3, moves=_moves(MIX), prior_fn=lambda q: box_lnprior_batch(q, prob.bounds), gate_box=False)
    host.run_mcmc(p0, 60)
    assert host.last_path == "host-callback" and fused.last_path == "launch-per-half-step"
    assert np.max(np.abs(host.get_chain() - fused.get_chain())) < 1e-7
    assert np.array_equal(host._naccept.cpu().numpy(), fused._naccept.cpu().numpy())
    assert 0 < int(fused._naccept.sum()) < W * 60


@pytest.mark.parametrize("spec", [ms.STRETCH, (("de", 1e-5, None, 0.8), ("snooker", 1.7, 0.2))], ids=["stretch", "de+snooker"])
def test_older_move_sets_keep_their_chains(spec, monkeypatch):
    """Sets without a new move against the model they were documented with (snooker_numpy, which knows nothing of streams 6-8):
    the same chain as before, on the launch-per-half-step path where the changed draw kernel and HalfArgs are."""
    monkeypatch.setenv("ALABI_ENS_STREAM", "0")
    run = ms.model_chain(5, "ExpSquared", 12, spec=tuple(spec), tag="older", nsteps=60, cont=0)
    ms.assert_honest(run.stats)
    s = ms.sampler(run.prob, 12, run.seed, moves=ms.moves_objects(spec))
    s.run_mcmc(run.p0, 60)
    assert s.last_path == "launch-per-half-step"
    assert np.max(np.abs(s.get_chain() - run.chain)) < 1e-7
    assert np.array_equal(s._naccept.cpu().numpy(), run.nacc)


def test_planted_singular_half_is_rejected_and_counted():
    """All complementary walkers of step 0, split 0 on one point: every proposal of that half step is rejected, the counter reads
    1, and the run goes on as the model's does."""
    d, W, seed = 3, 16, 41
    prob = ms.problem(d, "ExpSquared")
    dr = sn.draw_steps_batched(seed, 0, 1, W, np.array([1.0]))
    order, n0 = dr["order"][0], dr["n0"]
    p0 = _start(prob, W, seed, 2.0)
    p0[order[n0:]] = p0[order[n0]]
    model = ms.BoxModel(prob)
    sing, margins = [], []
    chain_o, lp_o, nacc_o, _, _ = wk.run_ensemble_moves(p0, 4, model, seed=seed, moves=list(KDE), singular_out=sing, margin_out=margins)
    assert sing == [(0, 0)]
    assert np.array_equal(chain_o[0][order[:n0]], p0[order[:n0]])
    live = np.concatenate(margins[1:])
    assert np.min(np.abs(live[np.isfinite(live)])) > ms.MIN_MARGIN and nacc_o.sum() > 0
    s = ms.sampler(prob, W, seed, moves=_moves(KDE))
    s.run_mcmc(p0, 4, skip_initial_state_check=True)
    assert s.kde_singular_half_steps == 1
    chain = s.get_chain()
    assert np.array_equal(chain[0][order[:n0]], p0[order[:n0]])
    assert np.max(np.abs(chain - chain_o)) < 1e-7
    assert np.array_equal(s._naccept.cpu().numpy(), nacc_o)


def test_bounds_on_the_walkers_and_no_sharding():
    from alabi_amd.moves import KDEMove, WalkMove
    prob = ms.problem(5, "ExpSquared")
    with pytest.raises(ValueError, match="nwalkers // 2"):
        ms.sampler(prob, 12, 1, moves=WalkMove(s=7))
    with pytest.raises(ValueError, match="2 ndim"):
        ms.sampler(prob, 11, 1, moves=KDEMove())
    for mv in (WalkMove(), [(KDEMove(), 0.5), (WalkMove(), 0.5)]):
        with pytest.raises(ValueError, match="shard"):
            ms.sampler(prob, 48, 1, shard=True, moves=mv)
    with pytest.warns(RuntimeWarning, match="KDEMove"):
        s = ms.sampler(prob, 12, 1, moves=KDEMove())
    s._ensure_ens()                                           # 2 d + 2 walkers are enough for the library as well
    assert [type(m).__name__ for m, _ in s.moves] == ["KDEMove"]


def test_run_emcee_takes_a_kde_mixture(tmp_path):
    from alabi_amd import SurrogateModel
    from alabi_amd.benchmarks import gaussian_2d
    from alabi_amd.moves import DEMove, KDEMove
    sm = SurrogateModel(lnlike_fn=gaussian_2d["fn"], bounds=gaussian_2d["bounds"], savedir=str(tmp_path), verbose=False,
                        random_state=2, cache=False)
    sm.init_samples(ntrain=60)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1, optimizer_kwargs={"maxiter": 10})
    mv = [(KDEMove(), 0.3), (DEMove(), 0.7)]
    sm.run_emcee(nwalkers=24, nsteps=300, min_ess=50, sampler_kwargs={"moves": mv})
    assert sm.emcee_sampler.last_path == "launch-per-half-step"
    assert [type(m).__name__ for m, _ in sm.emcee_sampler.moves] == ["KDEMove", "DEMove"]
    assert sm.emcee_sampler.kde_singular_half_steps == 0
    b = np.asarray(gaussian_2d["bounds"], dtype=float)
    assert sm.emcee_samples.shape[1] == 2 and sm.emcee_samples.shape[0] >= 50
    assert np.all(sm.emcee_samples > b[:, 0]) and np.all(sm.emcee_samples < b[:, 1])
    assert 0.05 < sm.acc_frac < 0.95
