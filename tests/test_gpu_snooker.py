"""GPU parity of the snooker move (alabi_amd.moves.SnookerMove: ens_draw_kernel's snooker record, snooker_coord and the
three-partner instantiations of the half-step and propose kernels) against tests/snooker_numpy.py, on the 500 x 5 problem of
tests/test_gpu_moves.py.  Tolerances are that file's: proposals bit for bit, log-probabilities to 1e-8 relative (device log /
exp against NumPy's), production chains to 1e-7 with identical acceptance counts."""
import ctypes as C

import numpy as np
import pytest

import snooker_numpy as sn
from conftest import make_problem

pytestmark = pytest.mark.gpu

SNOOKER = [("snooker", 1.7, 1.0)]
DE_SNOOKER = [("de", 1e-5, None, 0.8), ("snooker", 1.7, 0.2)]
ALL_THREE = [("stretch", 2.0, 0.3), ("de", 1e-5, None, 0.4), ("snooker", 1.4, 0.3)]


def _moves(spec):
    """The numpy statement's move list as alabi_amd.moves objects."""
    from alabi_amd.moves import DEMove, SnookerMove, StretchMove
    make = {"stretch": lambda m: (StretchMove(m[1]), m[2]), "de": lambda m: (DEMove(sigma=m[1], gamma0=m[2]), m[3]),
            "snooker": lambda m: (SnookerMove(m[1]), m[2])}
    return [make[m[0]](m) for m in spec]


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
@pytest.mark.parametrize("W", [6, 7, 33, 257])
def test_device_snooker_draws_match_numpy(setup, W, E):
    """Move index, j1, j2, j3 and the partners' global ids bit for bit (pairwise distinct), whichever move the step takes; a
    stretch record carries -1 in the second- and third-partner slots, a DE record in the third-partner slots.  Steps 0, 1, one
    beyond 2^32, and the first later step at which ensemble 0 takes each kind."""
    torch, g, o, y, bounds = setup
    from alabi_amd import EnsembleSampler, _lib
    from oracle.stretch_oracle import draw_step_randoms
    seed, WT = 0xDEADBEEFCAFE1234, W * E
    spec = [("de", 1e-5, None, 0.4), ("snooker", 1.7, 0.35), ("stretch", 2.5, 0.25)]
    kinds, cum, tp0, _ = sn.move_table(spec, 5)
    later = sn.draw_steps_batched(seed, 2, 64, W, cum)["move"]
    steps = (0, 1, 12345678901) + tuple(2 + int(np.argmax(later == k)) for k in range(3))
    s = EnsembleSampler(W, 5, g, y, bounds, seed=seed, live_dangerously=True, n_ensembles=E, moves=_moves(spec))
    s._ensure_ens()
    seen = set()
    lib = _lib.lib()
    for step in steps:
        ints = {k: torch.empty(WT, dtype=torch.int32, device="cuda") for k in ("order", "partner", "cw", "j2", "j3", "cw2", "cw3")}
        dbl = {k: torch.empty(WT, dtype=torch.float64, device="cuda") for k in ("u_z", "u_acc", "zz", "gam")}
        move = torch.empty(E, dtype=torch.int32, device="cuda")
        n0 = C.c_int(0)
        st = _lib.current_stream()
        _lib.check(lib.alabi_ens_export_draws(s._ens, step, 2.0, _lib.ptr(ints["order"]), C.byref(n0), _lib.ptr(dbl["u_z"]),
                                              _lib.ptr(ints["partner"]), _lib.ptr(dbl["u_acc"]), _lib.ptr(ints["cw"]),
                                              _lib.ptr(dbl["zz"]), st), "export_draws")
        _lib.check(lib.alabi_ens_export_move_draws(s._ens, _lib.ptr(move), _lib.ptr(ints["j2"]), _lib.ptr(dbl["gam"]), st),
                   "export_move_draws")
        _lib.check(lib.alabi_ens_export_snooker_draws(s._ens, _lib.ptr(ints["j3"]), st), "export_snooker_draws")
        _lib.check(lib.alabi_ens_export_partner_ids(s._ens, _lib.ptr(ints["cw2"]), _lib.ptr(ints["cw3"]), st), "export_partner_ids")
        torch.cuda.synchronize()
        host = {k: v.cpu().numpy() for k, v in {**ints, **dbl}.items()}
        for e in range(E):
            ro, rn0, ruz, rp, rua = draw_step_randoms(seed, step, W, id0=e * W)
            mi, rj1, rj2, rj3 = sn.draw_snooker_randoms(seed, step, W, cum, id0=e * W)
            sl = slice(e * W, (e + 1) * W)
            assert n0.value == rn0 and int(move.cpu()[e]) == mi
            assert np.array_equal(host["order"][sl], ro + e * W)
            assert np.array_equal(host["partner"][sl], rj1[ro]) and np.array_equal(rj1, rp)
            assert np.array_equal(host["u_z"][sl], ruz[ro]) and np.array_equal(host["u_acc"][sl], rua[ro])
            # global id of the walker at index j of the complementary list, by list position
            comp = lambda j: np.where(np.arange(W) < rn0, ro[rn0:][np.minimum(j, W - rn0 - 1)], ro[:rn0][np.minimum(j, rn0 - 1)]) + e * W  # noqa: E731
            assert np.array_equal(host["cw"][sl], comp(rj1[ro]))
            seen.add(int(kinds[mi]))
            if kinds[mi] == 0:
                for k in ("j2", "j3", "cw2", "cw3"):
                    assert np.all(host[k][sl] == -1), k
                continue
            assert np.array_equal(host["j2"][sl], rj2[ro]) and np.array_equal(host["cw2"][sl], comp(rj2[ro]))
            if kinds[mi] == 1:
                assert np.all(host["j3"][sl] == -1) and np.all(host["cw3"][sl] == -1)
                continue
            dj = [host[k][sl] for k in ("partner", "j2", "j3")]
            assert np.array_equal(dj[2], rj3[ro]) and np.array_equal(host["cw3"][sl], comp(rj3[ro]))
            assert np.all(dj[0] != dj[1]) and np.all(dj[0] != dj[2]) and np.all(dj[1] != dj[2])
            assert np.all(host["zz"][sl] == tp0[mi])                 # gammas sits in the stretch factor's slot
    assert seen == {0, 1, 2}


def test_snooker_step_with_injected_randoms(setup):
    """Same (order, j1, j2, j3, gamma, u_acc) -> bit-identical proposals, identical accept mask; non-distinct or out-of-range
    indices make the proposal a no-op."""
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

    def step(order, n0, j1, j2, j3, gamma, u_acc):
        dev = [torch.as_tensor(a, device="cuda") for a in (order, j1, j2, j3, u_acc)]   # alive until the kernels have run
        st = _lib.lib().alabi_ens_step_with_randoms_snooker(s._ens, _lib.ptr(c_dev), _lib.ptr(lp_dev), _lib.ptr(dev[0]), n0,
                                                            _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]), gamma,
                                                            _lib.ptr(dev[4]), _lib.ptr(nacc), _lib.current_stream())
        _lib.check(st, "step_with_randoms_snooker")
        torch.cuda.synchronize()
        return c_dev.cpu().numpy(), lp_dev.cpu().numpy()

    for it in range(30):
        rs = np.random.RandomState(100 + it)
        inds = np.arange(W) % 2; rs.shuffle(inds)
        ids = np.arange(W)
        order = np.concatenate([ids[inds == 0], ids[inds == 1]]).astype(np.int32); n0 = int((inds == 0).sum())
        trip = np.array([rs.permutation(W // 2)[:3] for _ in range(W)], dtype=np.int32)
        j1, j2, j3 = (np.ascontiguousarray(trip[:, k]) for k in range(3))
        gamma = 1.7 if it % 2 else 0.9
        u_acc = rs.rand(W)
        c_o, l_o, a_o, _ = sn.snooker_step_arrays(coords, logp_o, order, n0, j1, j2, j3, gamma, u_acc, lnp)
        before = c_dev.cpu().numpy().copy()
        c_g, l_g = step(order, n0, j1, j2, j3, gamma, u_acc)
        a_g = np.any(c_g != before, axis=1)
        assert np.array_equal(a_g, a_o), f"accept mask differs at iteration {it}"
        assert np.array_equal(c_g, c_o)                  # proposals are bit-identical (products rounded, sums in coordinate order)
        assert np.max(np.abs(l_g - l_o)) < 1e-8 * (1 + np.max(np.abs(l_o[np.isfinite(l_o)])))
        coords, logp_o = c_o, l_o
        lp_dev.copy_(torch.as_tensor(l_o, device="cuda"))
    assert int(nacc.sum()) > 0 and n_out[0] > 0          # accepts and out-of-box rejections both occurred
    # no-ops: j3 == j1, j2 == j1, an index beyond the complementary list, a negative one -- every walker has one of them
    bad2 = np.where(ids % 4 == 1, j1, j2).astype(np.int32)
    bad3 = np.where(ids % 4 == 0, j1, np.where(ids % 4 == 2, W // 2, np.where(ids % 4 == 3, -1, j3))).astype(np.int32)
    taken = int(nacc.sum())
    c_g, l_g = step(order, n0, j1, bad2, bad3, 1.7, np.full(W, 1e-300))
    assert np.array_equal(c_g, coords) and np.array_equal(l_g, logp_o) and int(nacc.sum()) == taken


@pytest.mark.parametrize("spec", [SNOOKER, DE_SNOOKER, ALL_THREE], ids=["snooker", "de+snooker", "stretch+de+snooker"])
@pytest.mark.parametrize("W,nsteps,thin", [(32, 300, 1), (33, 64, 1), (6, 100, 3)])
def test_production_run_matches_numpy_chain(setup, W, nsteps, thin, spec):
    """Counter-based draws + kernel sequence == snooker_numpy.run_ensemble_moves, step for step."""
    torch, g, o, y, bounds = setup
    from alabi_amd import EnsembleSampler
    p0 = np.random.RandomState(W).uniform(-2, 2, (W, 5))
    s = EnsembleSampler(W, 5, g, y, bounds, seed=77, moves=_moves(spec), live_dangerously=True)
    s.run_mcmc(p0, nsteps, thin_by=thin)
    assert s.last_path == "launch-per-half-step"
    lnp = _lnp(o, y, bounds)
    counts = {}
    chain_o, lp_o, nacc_o, c_end, lp_end = sn.run_ensemble_moves(p0, nsteps, lnp, seed=77, moves=spec, thin_by=thin, count_moves=counts)
    assert len(counts) == len(spec)                      # every move of the set ran
    chain = s.get_chain()
    assert chain.shape == chain_o.shape
    assert np.max(np.abs(chain - chain_o)) < 1e-7
    assert np.max(np.abs(s.get_log_prob() - lp_o)) < 1e-7
    assert np.array_equal(s._naccept.cpu().numpy(), nacc_o)
    assert 0 < nacc_o.sum() < W * nsteps
    # continuing the run continues the counter
    s.run_mcmc(None, 10 * thin, thin_by=thin)
    chain_o2 = sn.run_ensemble_moves(c_end, 10 * thin, lnp, seed=77, moves=spec, thin_by=thin, step0=nsteps, logp0=lp_end)[0]
    assert np.max(np.abs(s.get_chain()[-10:] - chain_o2)) < 1e-7


def test_snooker_graph_and_eager_paths_agree(setup, monkeypatch):
    torch, g, o, y, bounds = setup
    from alabi_amd import EnsembleSampler
    p0 = np.random.RandomState(2).uniform(-2, 2, (40, 5))
    monkeypatch.setenv("ALABI_ENS_GRAPH_STEPS", "64")
    a = EnsembleSampler(40, 5, g, y, bounds, seed=5, moves=_moves(ALL_THREE)); a.run_mcmc(p0, 200)
    monkeypatch.setenv("ALABI_ENS_GRAPH", "0")
    b = EnsembleSampler(40, 5, g, y, bounds, seed=5, moves=_moves(ALL_THREE)); b.run_mcmc(p0, 200)
    assert np.array_equal(a.get_chain(), b.get_chain())
    assert np.array_equal(a.get_log_prob(), b.get_log_prob())
    assert np.array_equal(a.acceptance_fraction, b.acceptance_fraction)
    assert 0.0 < a.acceptance_fraction.mean() < 1.0


def test_snooker_independent_ensembles(setup):
    """n_ensembles = 3: rows [eW, (e+1)W) evolve like a stand-alone ensemble whose walker ids start at eW, the move choice
    and the third partner (stream 5 at the global walker id) included."""
    torch, g, o, y, bounds = setup
    from alabi_amd import EnsembleSampler
    W, E, nsteps = 24, 3, 120
    p0 = np.random.RandomState(21).uniform(-2, 2, (W * E, 5))
    s = EnsembleSampler(W, 5, g, y, bounds, seed=1234, n_ensembles=E, moves=_moves(DE_SNOOKER))
    s.run_mcmc(p0, nsteps)
    chain = s.get_chain()
    lnp = _lnp(o, y, bounds)
    for e in range(E):
        ref, _, nacc, _, _ = sn.run_ensemble_moves(p0[e * W:(e + 1) * W], nsteps, lnp, seed=1234, moves=DE_SNOOKER, id0=e * W)
        assert np.max(np.abs(chain[:, e * W:(e + 1) * W] - ref)) < 1e-7
        assert np.array_equal(s._naccept.cpu().numpy()[e * W:(e + 1) * W], nacc)


def test_host_prior_callback_equals_fused_snooker_chain(setup):
    """A Python prior_fn equal to the box: propose kernel (three-partner instantiation, which leaves the log factor in the
    record) -> host -> accept kernel gives the chain of the fused kernels."""
    torch, g, o, y, bounds = setup
    from alabi_amd import EnsembleSampler
    from oracle.stretch_oracle import box_lnprior_batch
    W = 32
    p0 = np.random.RandomState(12).uniform(-2.5, 2.5, (W, 5))
    fused = EnsembleSampler(W, 5, g, y, bounds, seed=3, moves=_moves(ALL_THREE)); fused.run_mcmc(p0, 150)
    host = EnsembleSampler(W, 5, g, y, bounds, seed=3, moves=_moves(ALL_THREE), prior_fn=lambda q: box_lnprior_batch(q, bounds),
                           gate_box=False)
    host.run_mcmc(p0, 150)
    assert host.last_path == "host-callback" and fused.last_path == "launch-per-half-step"
    assert np.max(np.abs(host.get_chain() - fused.get_chain())) < 1e-7
    assert np.array_equal(host._naccept.cpu().numpy(), fused._naccept.cpu().numpy())
    assert 0 < int(fused._naccept.sum()) < W * 150


def test_snooker_needs_six_walkers_and_cannot_be_sharded(setup):
    torch, g, o, y, bounds = setup
    from alabi_amd import EnsembleSampler
    from alabi_amd.moves import DEMove, SnookerMove
    with pytest.raises(ValueError, match="nwalkers"):
        EnsembleSampler(5, 5, g, y, bounds, seed=1, live_dangerously=True, moves=SnookerMove())
    with pytest.raises(ValueError, match="nwalkers"):
        EnsembleSampler(5, 5, g, y, bounds, seed=1, live_dangerously=True, moves=[(DEMove(), 0.8), (SnookerMove(), 0.2)])
    with pytest.raises(ValueError, match="shard"):
        EnsembleSampler(16, 5, g, y, bounds, seed=1, shard=True, moves=[(DEMove(), 0.8), (SnookerMove(), 0.2)])
    s = EnsembleSampler(6, 5, g, y, bounds, seed=1, live_dangerously=True, moves=SnookerMove())
    s._ensure_ens()                                        # six walkers are enough for the library as well
    assert [type(m).__name__ for m, _ in s.moves] == ["SnookerMove"]


def test_run_emcee_takes_a_snooker_mixture(tmp_path):
    from alabi_amd import SurrogateModel
    from alabi_amd.benchmarks import gaussian_2d
    from alabi_amd.moves import DEMove, SnookerMove
    sm = SurrogateModel(lnlike_fn=gaussian_2d["fn"], bounds=gaussian_2d["bounds"], savedir=str(tmp_path), verbose=False,
                        random_state=2, cache=False)
    sm.init_samples(ntrain=60)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1, optimizer_kwargs={"maxiter": 10})
    mv = [(DEMove(), 0.8), (SnookerMove(), 0.2)]
    with pytest.raises(ValueError, match="shard"):        # before anything is launched
        sm.run_emcee(nwalkers=12, nsteps=300, min_ess=50, sampler_kwargs={"moves": mv, "shard": True})
    sm.run_emcee(nwalkers=12, nsteps=300, min_ess=50, sampler_kwargs={"moves": mv})
    assert len(sm.emcee_sampler.moves) == 2 and sm.emcee_sampler.last_path == "launch-per-half-step"
    assert [type(m).__name__ for m, _ in sm.emcee_sampler.moves] == ["DEMove", "SnookerMove"]
    assert [w for _, w in sm.emcee_sampler.moves] == [0.8, 0.2]
    b = np.asarray(gaussian_2d["bounds"], dtype=float)
    assert sm.emcee_samples.shape[1] == 2 and sm.emcee_samples.shape[0] >= 50
    assert np.all(sm.emcee_samples > b[:, 0]) and np.all(sm.emcee_samples < b[:, 1])
    assert 0.05 < sm.acc_frac < 0.95
