"""GPU parity of the ensemble sampler's moves -- emcee's DEMove and weighted mixtures of StretchMove / DEMove
(alabi_amd/moves.py, ens_draw_kernel and the two-partner half-step kernels) -- against tests/de_move_numpy.py."""
import ctypes as C

import numpy as np
import pytest

import de_move_numpy as dm
from conftest import make_problem
from de_move_numpy import TWO_MODE_MOVES, mode_share_and_crossings, two_mode_lnprob, two_mode_start

pytestmark = pytest.mark.gpu

DE_ALONE = [("de", 1e-5, None, 1.0)]
DE_STRETCH = [("de", 1e-5, None, 0.5), ("stretch", 2.0, 0.5)]


def _moves(spec):
    """The numpy statement's move list as alabi_amd.moves objects."""
    from alabi_amd.moves import DEMove, StretchMove
    return [(StretchMove(m[1]), m[2]) if m[0] == "stretch" else (DEMove(sigma=m[1], gamma0=m[2]), m[3]) for m in spec]


@pytest.fixture(scope="module")
def setup():
    import torch
    from alabi_amd import HipGP
    from oracle.gp_oracle import OracleGP
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    X, y, h = make_problem(500, 5, 31)
    g = HipGP(5, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"]); g.compute(X)
    o = OracleGP(5, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"]).compute(X)
    bounds = np.array([[-3.0, 3.0]] * 5)
    return torch, g, o, y, bounds


@pytest.fixture(scope="module")
def small():
    """The 260 x 4 problem of the multi-proposal test."""
    from alabi_amd import HipGP
    X, y, h = make_problem(260, 4, 21, log_wn=-9.0)
    g = HipGP(4, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"]); g.compute(X)
    return g, y, np.array([[-3.0, 3.0]] * 4)


def _lnp(o, y, bounds, counter=None):
    from oracle.stretch_oracle import box_lnprior_batch

    def f(q):
        lp = box_lnprior_batch(q, bounds)
        inside = np.isfinite(lp)
        if counter is not None:
            counter[0] += int(np.sum(~inside))
        out = np.full(len(q), -np.inf)
        if inside.any():
            out[inside] = o.predict(y, q[inside])
        return out
    return f


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("W", [4, 10, 33, 257])
def test_device_move_draws_match_numpy(setup, W, E):
    """Move index, j1 and j2 bit for bit (j1 != j2), streams 0-2 still bit for bit whichever move the step takes, gamma within
    8 * 2^-52 * g0 * (1 + |sigma n|): n carries at most ~5 ulp (log 1 ulp, halved by the correctly rounded sqrt; cos 2 ulp in HIP
    and 0.5 in libm; two multiplications), the rest is the roundings of g0 * (1 + sigma * n) itself."""
    torch, g, o, y, bounds = setup
    from alabi_amd import EnsembleSampler, _lib
    from alabi_amd.moves import DEMove, StretchMove
    from oracle.stretch_oracle import draw_step_randoms
    seed, a, WT = 0xDEADBEEFCAFE1234, 2.5, W * E
    cum = np.cumsum(np.array([0.8, 0.2]) / 1.0)
    # the listed steps, and the first later one at which ensemble 0 takes the stretch move: both kinds of record are seen
    later = dm.draw_steps_batched(seed, 2, 64, W, cum)["move"]
    steps = (0, 1, 12345678901, 2 + int(np.argmax(later == 1)))
    seen = set()
    for sigma in (1e-5, 0.3):
        g0 = 2.38 / np.sqrt(2 * 5)
        s = EnsembleSampler(W, 5, g, y, bounds, seed=seed, live_dangerously=True, n_ensembles=E,
                            moves=[(DEMove(sigma=sigma), 0.8), (StretchMove(a), 0.2)])
        s._ensure_ens()
        for step in steps:
            order = torch.empty(WT, dtype=torch.int32, device="cuda"); partner = torch.empty_like(order)
            cw = torch.empty_like(order); j2 = torch.empty_like(order)
            move = torch.empty(E, dtype=torch.int32, device="cuda")
            u_z = torch.empty(WT, dtype=torch.float64, device="cuda"); u_acc = torch.empty_like(u_z)
            zz = torch.empty_like(u_z); gam = torch.empty_like(u_z)
            n0 = C.c_int(0)
            _lib.check(_lib.lib().alabi_ens_export_draws(s._ens, step, 2.0, _lib.ptr(order), C.byref(n0), _lib.ptr(u_z),
                                                         _lib.ptr(partner), _lib.ptr(u_acc), _lib.ptr(cw), _lib.ptr(zz),
                                                         _lib.current_stream()), "export_draws")
            _lib.check(_lib.lib().alabi_ens_export_move_draws(s._ens, _lib.ptr(move), _lib.ptr(j2), _lib.ptr(gam),
                                                              _lib.current_stream()), "export_move_draws")
            torch.cuda.synchronize()
            for e in range(E):
                ro, rn0, ruz, rp, rua = draw_step_randoms(seed, step, W, id0=e * W)
                mi, rj1, rj2, rn, rgam = dm.draw_move_randoms(seed, step, W, cum, g0=g0, sigma=sigma, id0=e * W)
                sl = slice(e * W, (e + 1) * W)
                assert n0.value == rn0 and int(move.cpu()[e]) == mi
                assert np.array_equal(order.cpu().numpy()[sl], ro + e * W)
                assert np.array_equal(partner.cpu().numpy()[sl], rp[ro])
                assert np.array_equal(u_z.cpu().numpy()[sl], ruz[ro])
                assert np.array_equal(u_acc.cpu().numpy()[sl], rua[ro])
                comp = lambda j: np.where(np.arange(W) < rn0, ro[rn0:][np.minimum(j, W - rn0 - 1)], ro[:rn0][np.minimum(j, rn0 - 1)])  # noqa: E731
                assert np.array_equal(cw.cpu().numpy()[sl], comp(rp[ro]) + e * W)
                seen.add(mi)
                if mi == 1:                                   # a stretch step: the record of the stretch move with ITS a
                    assert np.array_equal(zz.cpu().numpy()[sl], ((a - 1.0) * ruz[ro] + 1.0) ** 2.0 / a)
                    assert np.all(j2.cpu().numpy()[sl] == -1)
                    continue
                dj2 = j2.cpu().numpy()[sl]
                assert np.array_equal(dj2, rj2[ro]) and np.all(dj2 != partner.cpu().numpy()[sl])
                err = np.abs(gam.cpu().numpy()[sl] - rgam[ro])
                bound = 8 * 2.0 ** -52 * g0 * (1 + np.abs(sigma * rn[ro]))
                print(f"W={W} E={E} step={step} sigma={sigma}: max gamma err / bound = {np.max(err / bound):.3f}")
                assert np.all(err <= bound)
                assert np.array_equal(zz.cpu().numpy()[sl], gam.cpu().numpy()[sl])   # gamma sits in the stretch factor's slot
    assert seen == {0, 1}


def test_de_step_with_injected_randoms(setup):
    """Same (order, j1, j2, gamma, u_acc) -> bit-identical proposals, identical accept mask."""
    torch, g, o, y, bounds = setup
    from alabi_amd import EnsembleSampler, _lib
    W, d = 48, 5
    rng = np.random.RandomState(4)
    s = EnsembleSampler(W, d, g, y, bounds, seed=1)
    coords = rng.uniform(-2.9, 2.9, (W, d))               # close to the walls: some proposals leave the box
    n_out = [0]
    lnp = _lnp(o, y, bounds, n_out)
    logp_o = lnp(coords)
    n_out[0] = 0
    c_dev = torch.as_tensor(coords, device="cuda").clone()
    lp_dev = s.compute_log_prob(c_dev)
    nacc = torch.zeros(W, dtype=torch.int64, device="cuda")
    g0 = 2.38 / np.sqrt(2 * d)
    for it in range(30):
        rs = np.random.RandomState(100 + it)
        inds = np.arange(W) % 2; rs.shuffle(inds)
        ids = np.arange(W)
        order = np.concatenate([ids[inds == 0], ids[inds == 1]]).astype(np.int32); n0 = int((inds == 0).sum())
        j1 = rs.randint(W // 2, size=W).astype(np.int32)
        j2 = rs.randint(W // 2 - 1, size=W).astype(np.int32); j2 += (j2 >= j1)
        gamma = g0 * (1 + (0.3 if it % 2 else 1e-5) * rs.randn(W)); u_acc = rs.rand(W)
        c_o, l_o, a_o = dm.de_step_arrays(coords, logp_o, order, n0, j1, j2, gamma, u_acc, lnp)
        before = c_dev.cpu().numpy().copy()
        dev = [torch.as_tensor(a, device="cuda") for a in (order, j1, j2, gamma, u_acc)]   # alive until the kernels have run
        st = _lib.lib().alabi_ens_step_with_randoms_de(s._ens, _lib.ptr(c_dev), _lib.ptr(lp_dev), _lib.ptr(dev[0]), n0,
                                                       _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]), _lib.ptr(dev[4]),
                                                       _lib.ptr(nacc), _lib.current_stream())
        _lib.check(st, "step_with_randoms_de")
        torch.cuda.synchronize()
        c_g = c_dev.cpu().numpy(); l_g = lp_dev.cpu().numpy()
        a_g = np.any(c_g != before, axis=1)
        assert np.array_equal(a_g, a_o), f"accept mask differs at iteration {it}"
        assert np.array_equal(c_g, c_o)                  # proposals are bit-identical (multiply, then add: no FMA)
        assert np.max(np.abs(l_g - l_o)) < 1e-8 * (1 + np.max(np.abs(l_o[np.isfinite(l_o)])))
        coords, logp_o = c_o, l_o
        lp_dev.copy_(torch.as_tensor(l_o, device="cuda"))
    assert int(nacc.sum()) > 0 and n_out[0] > 0          # accepts and out-of-box rejections both occurred


@pytest.mark.parametrize("spec", [DE_ALONE, DE_STRETCH], ids=["de", "de+stretch"])
@pytest.mark.parametrize("W,nsteps,thin", [(32, 300, 1), (64, 257, 3), (33, 64, 1)])
def test_production_run_matches_numpy_chain(setup, W, nsteps, thin, spec):
    """Counter-based draws + kernel sequence (graph replay + eager tail) == run_ensemble_moves, step for step."""
    torch, g, o, y, bounds = setup
    from alabi_amd import EnsembleSampler
    p0 = np.random.RandomState(W).uniform(-2, 2, (W, 5))
    s = EnsembleSampler(W, 5, g, y, bounds, seed=77, moves=_moves(spec))
    s.run_mcmc(p0, nsteps, thin_by=thin)
    assert s.last_path == "launch-per-half-step"
    lnp = _lnp(o, y, bounds)
    counts = {}
    chain_o, lp_o, nacc_o, c_end, lp_end = dm.run_ensemble_moves(p0, nsteps, lnp, seed=77, moves=spec, thin_by=thin, count_moves=counts)
    assert len(counts) == len(spec)                      # every move of the set ran
    chain = s.get_chain()
    assert chain.shape == chain_o.shape
    assert np.max(np.abs(chain - chain_o)) < 1e-7
    assert np.max(np.abs(s.get_log_prob() - lp_o)) < 1e-7
    assert np.array_equal(s._naccept.cpu().numpy(), nacc_o)
    assert 0 < nacc_o.sum() < W * nsteps
    # continuing the run continues the counter (emcee: run_mcmc(None, n) resumes)
    s.run_mcmc(None, 10 * thin, thin_by=thin)
    chain_o2 = dm.run_ensemble_moves(c_end, 10 * thin, lnp, seed=77, moves=spec, thin_by=thin, step0=nsteps, logp0=lp_end)[0]
    assert np.max(np.abs(s.get_chain()[-10:] - chain_o2)) < 1e-7


def test_de_graph_and_eager_paths_agree(setup, monkeypatch):
    torch, g, o, y, bounds = setup
    from alabi_amd import EnsembleSampler
    p0 = np.random.RandomState(2).uniform(-2, 2, (40, 5))
    monkeypatch.setenv("ALABI_ENS_GRAPH_STEPS", "64")
    a = EnsembleSampler(40, 5, g, y, bounds, seed=5, moves=_moves(DE_STRETCH)); a.run_mcmc(p0, 200)
    monkeypatch.setenv("ALABI_ENS_GRAPH", "0")
    b = EnsembleSampler(40, 5, g, y, bounds, seed=5, moves=_moves(DE_STRETCH)); b.run_mcmc(p0, 200)
    assert np.array_equal(a.get_chain(), b.get_chain())
    assert np.array_equal(a.get_log_prob(), b.get_log_prob())
    assert np.array_equal(a.acceptance_fraction, b.acceptance_fraction)


@pytest.mark.parametrize("W,E", [(40, 16), (700, 1)])
def test_de_multi_proposal_half_step_bit_identical(small, W, E, monkeypatch):
    """The two-partner instantiation of ens_half_multi_kernel against that of ens_half_kernel (ragged last workgroup included)."""
    from alabi_amd import EnsembleSampler
    g, y, bounds = small
    p0 = np.random.RandomState(5).uniform(-2, 2, (W * E, 4))
    out = {}
    for multi in ("0", "1"):
        monkeypatch.setenv("ALABI_ENS_MULTI", multi)
        s = EnsembleSampler(W, 4, g, y, bounds, seed=8, n_ensembles=E, moves=_moves(DE_STRETCH))
        s.run_mcmc(p0, 40)
        assert s.last_path == "launch-per-half-step"
        out[multi] = (s.get_chain(), s.get_log_prob(), s.acceptance_fraction)
    for a, b in zip(out["0"], out["1"]):
        np.testing.assert_array_equal(a, b)
    assert 0.0 < out["0"][2].mean() < 1.0


def test_de_independent_ensembles(setup):
    """n_ensembles = 3: rows [eW, (e+1)W) evolve like a stand-alone ensemble whose walker ids start at eW, the move choice
    included (stream 3 at the ensemble's walker 0)."""
    torch, g, o, y, bounds = setup
    from alabi_amd import EnsembleSampler
    W, E, nsteps = 24, 3, 120
    p0 = np.random.RandomState(21).uniform(-2, 2, (W * E, 5))
    s = EnsembleSampler(W, 5, g, y, bounds, seed=1234, n_ensembles=E, moves=_moves(DE_STRETCH))
    s.run_mcmc(p0, nsteps)
    chain = s.get_chain()
    lnp = _lnp(o, y, bounds)
    for e in range(E):
        ref, _, nacc, _, _ = dm.run_ensemble_moves(p0[e * W:(e + 1) * W], nsteps, lnp, seed=1234, moves=DE_STRETCH, id0=e * W)
        assert np.max(np.abs(chain[:, e * W:(e + 1) * W] - ref)) < 1e-7
        assert np.array_equal(s._naccept.cpu().numpy()[e * W:(e + 1) * W], nacc)


def test_stretch_only_move_sets_keep_their_chain_and_their_kernel(setup):
    """moves=None, moves=StretchMove() and a=2.0 give bit-identical chains on the persistent kernel; so does a mixture of two
    equal stretch moves (the move choice touches nothing else), and a mixture of two different ones follows the numpy run."""
    torch, g, o, y, bounds = setup
    from alabi_amd import EnsembleSampler
    from alabi_amd.moves import StretchMove
    p0 = np.random.RandomState(40).uniform(-2, 2, (40, 5))
    runs = []
    for kw in ({}, {"moves": None}, {"moves": StretchMove()}, {"a": 2.0}, {"moves": [StretchMove(2.0), StretchMove(2.0)]}):
        s = EnsembleSampler(40, 5, g, y, bounds, seed=5, **kw)
        s.run_mcmc(p0, 300, thin_by=2)
        assert s.last_path == "stream" and getattr(s, "stream_fallbacks", 0) == 0
        runs.append((s.get_chain(), s.get_log_prob(), s._naccept.cpu().numpy().copy()))
    for r in runs[1:]:
        for x, x0 in zip(r, runs[0]):
            assert np.array_equal(x, x0)
    spec = [("stretch", 2.0, 0.5), ("stretch", 3.5, 0.5)]
    s = EnsembleSampler(40, 5, g, y, bounds, seed=5, moves=_moves(spec))
    s.run_mcmc(p0, 1100)                                 # more than one chunk: the second one is drawn ahead, on the side stream
    assert s.last_path == "stream" and len(s.moves) == 2
    counts = {}
    ref, lp, nacc, _, _ = dm.run_ensemble_moves(p0, 1100, _lnp(o, y, bounds), seed=5, moves=spec, count_moves=counts)
    assert min(counts.get(0, 0), counts.get(1, 0)) > 400
    assert np.max(np.abs(s.get_chain() - ref)) < 1e-7 and np.array_equal(s._naccept.cpu().numpy(), nacc)


def test_host_prior_callback_equals_fused_de_chain(setup):
    """A Python prior_fn equal to the box: propose kernel (two-partner instantiation) -> host -> accept kernel gives the chain
    of the fused kernels."""
    torch, g, o, y, bounds = setup
    from alabi_amd import EnsembleSampler
    from oracle.stretch_oracle import box_lnprior_batch
    W = 32
    p0 = np.random.RandomState(12).uniform(-2.5, 2.5, (W, 5))
    fused = EnsembleSampler(W, 5, g, y, bounds, seed=3, moves=_moves(DE_STRETCH)); fused.run_mcmc(p0, 150)
    host = EnsembleSampler(W, 5, g, y, bounds, seed=3, moves=_moves(DE_STRETCH), prior_fn=lambda q: box_lnprior_batch(q, bounds),
                           gate_box=False)
    host.run_mcmc(p0, 150)
    assert host.last_path == "host-callback" and fused.last_path == "launch-per-half-step"
    assert np.max(np.abs(host.get_chain() - fused.get_chain())) < 1e-7
    assert np.array_equal(host._naccept.cpu().numpy(), fused._naccept.cpu().numpy())


def test_host_likelihood_two_modes_are_equalised(setup):
    """The two-mode target as a host like_fn, ensemble and start of tests/test_moves_host.py: after 300 of 1500 steps with the
    ter Braak mixture the + mode, where 4 of the 32 walkers started, holds its half of the samples."""
    torch, g, o, y, _ = setup
    from alabi_amd import EnsembleSampler
    bounds = np.array([[-15.0, 15.0]] * 5)
    s = EnsembleSampler(32, 5, g, y, bounds, seed=11, moves=_moves(TWO_MODE_MOVES), like_fn=two_mode_lnprob)
    s.run_mcmc(two_mode_start(), 1500)
    share, crossings = mode_share_and_crossings(s.get_chain()[300:])
    print("share of the + mode", share, "crossings", crossings)
    assert 0.4 <= share <= 0.6


def test_de_needs_four_walkers_and_cannot_be_sharded(setup):
    torch, g, o, y, bounds = setup
    from alabi_amd import EnsembleSampler
    from alabi_amd.moves import DEMove, StretchMove
    with pytest.raises(ValueError, match="nwalkers"):
        EnsembleSampler(3, 5, g, y, bounds, seed=1, live_dangerously=True, moves=DEMove())
    with pytest.raises(ValueError, match="shard"):
        EnsembleSampler(16, 5, g, y, bounds, seed=1, shard=True, moves=[(DEMove(), 0.5), (StretchMove(), 0.5)])
    EnsembleSampler(16, 5, g, y, bounds, seed=1, shard=True, moves=StretchMove())      # a stretch-only set may be sharded


def test_run_emcee_takes_moves(tmp_path):
    from alabi_amd import SurrogateModel
    from alabi_amd.benchmarks import gaussian_2d
    from alabi_amd.moves import DEMove, StretchMove
    sm = SurrogateModel(lnlike_fn=gaussian_2d["fn"], bounds=gaussian_2d["bounds"], savedir=str(tmp_path), verbose=False,
                        random_state=2, cache=False)
    sm.init_samples(ntrain=60)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1, optimizer_kwargs={"maxiter": 10})
    mv = [(DEMove(), 0.8), (StretchMove(), 0.2)]
    with pytest.raises(ValueError, match="shard"):        # before anything is launched
        sm.run_emcee(nwalkers=12, nsteps=300, min_ess=50, sampler_kwargs={"moves": mv, "shard": True})
    with pytest.raises(NotImplementedError, match="DESnookerMove"):
        sm.run_emcee(nwalkers=12, nsteps=300, min_ess=50, sampler_kwargs={"moves": type("DESnookerMove", (), {})()})
    sm.run_emcee(nwalkers=12, nsteps=300, min_ess=50, sampler_kwargs={"moves": mv})
    assert len(sm.emcee_sampler.moves) == 2 and sm.emcee_sampler.last_path == "launch-per-half-step"
    assert [w for _, w in sm.emcee_sampler.moves] == [0.8, 0.2]
    b = np.asarray(gaussian_2d["bounds"], dtype=float)
    assert sm.emcee_samples.shape[1] == 2 and sm.emcee_samples.shape[0] >= 50
    assert np.all(sm.emcee_samples > b[:, 0]) and np.all(sm.emcee_samples < b[:, 1])
    assert 0.05 < sm.acc_frac < 0.95 and sm.emcee_mode == "single"
