"""The launch-per-half-step ensemble kernels, one step at a time, at every dimension bucket and in both kernel families: the
stretch, DE and snooker steps from injected draws (ens_half_kernel, ens_half_de_kernel, ens_half_snooker_kernel and
ens_lnprob_kernel at D = 1 .. 64, squared-exponential and generic) against oracle/stretch_oracle.py, tests/de_move_numpy.py and
tests/snooker_numpy.py, and the degenerate geometries of the snooker move, which must leave a walker where it is without a NaN.
Production runs of the same shapes are in tests/test_gpu_moves_chains.py; problems and model runs in tests/moves_shapes_common.py.

Tolerances are those of tests/test_gpu_snooker.py: accepted coordinates bit for bit, log-probabilities to 1e-8 relative, the accept
mask identical -- after the model run has been shown to have no accept test within 1e-6 of a tie."""
import numpy as np
import pytest

import moves_shapes_common as mc
import snooker_numpy as sn

pytestmark = pytest.mark.gpu

MOVES = ("stretch", "de", "snooker")


@pytest.fixture(autouse=True)
def half_step_path(monkeypatch):
    """The kernels under test are the ones that run: no persistent kernel, the library's own choice of proposals per workgroup."""
    monkeypatch.setenv("ALABI_ENS_STREAM", "0")
    monkeypatch.setenv("ALABI_ENS_GROUP", "0")
    monkeypatch.delenv("ALABI_ENS_MULTI", raising=False)


def _step(s, move, c_dev, lp_dev, nacc, dr):
    """One injected step on the device; the draws' device copies live until the kernels have run."""
    import torch
    from alabi_amd import _lib
    lib, P, st = _lib.lib(), _lib.ptr, _lib.current_stream()
    if move == "stretch":
        dev = [torch.as_tensor(a, device="cuda") for a in (dr.order, dr.u_z, dr.j1, dr.u_acc)]
        rc = lib.alabi_ens_step_with_randoms(s._ens, P(c_dev), P(lp_dev), P(dev[0]), dr.n0, P(dev[1]), P(dev[2]), P(dev[3]), 2.0, P(nacc), st)
    elif move == "de":
        dev = [torch.as_tensor(a, device="cuda") for a in (dr.order, dr.j1, dr.j2, dr.gamma_de, dr.u_acc)]
        rc = lib.alabi_ens_step_with_randoms_de(s._ens, P(c_dev), P(lp_dev), P(dev[0]), dr.n0, P(dev[1]), P(dev[2]), P(dev[3]), P(dev[4]),
                                                P(nacc), st)
    else:
        dev = [torch.as_tensor(a, device="cuda") for a in (dr.order, dr.j1, dr.j2, dr.j3, dr.u_acc)]
        rc = lib.alabi_ens_step_with_randoms_snooker(s._ens, P(c_dev), P(lp_dev), P(dev[0]), dr.n0, P(dev[1]), P(dev[2]), P(dev[3]),
                                                     float(dr.gamma_snk), P(dev[4]), P(nacc), st)
    _lib.check(rc, "step_with_randoms " + move)
    torch.cuda.synchronize()
    return c_dev.cpu().numpy(), lp_dev.cpu().numpy()


@pytest.mark.parametrize("d,kernel", mc.STEP_CASES, ids=[f"d{d}-{k}" for d, k in mc.STEP_CASES])
def test_one_step_from_injected_draws(d, kernel):
    """20 steps of each move, W = 16: same draws -> bit-identical rows, identical accept mask, logp to 1e-8; the device's logp is
    reset to the model's after every step."""
    import torch
    models = {mv: mc.model_steps(d, kernel, mv) for mv in MOVES}
    for mv in MOVES:
        print(f"d={d} {kernel} {mv}: {models[mv][3]}")
        mc.assert_honest(models[mv][3], mv)
    prob = mc.problem(d, kernel)
    s = mc.sampler(prob, mc.STEP_W, 1)
    for mv in MOVES:
        p0, lp0, steps, _ = models[mv]
        c_dev = torch.as_tensor(p0, device="cuda").clone()
        lp_dev = s.compute_log_prob(c_dev)
        err0 = np.max(np.abs(lp_dev.cpu().numpy() - lp0)) / (1 + np.max(np.abs(lp0)))
        assert err0 < 1e-8, (mv, err0)                       # ens_lnprob_kernel at this bucket
        nacc = torch.zeros(mc.STEP_W, dtype=torch.int64, device="cuda")
        before, worst = p0, 0.0
        for it, (dr, c_o, l_o, a_o) in enumerate(steps):
            c_g, l_g = _step(s, mv, c_dev, lp_dev, nacc, dr)
            assert np.array_equal(np.any(c_g != before, axis=1), a_o), f"{mv}: accept mask differs at step {it}"
            assert np.array_equal(c_g, c_o), f"{mv}: rows differ at step {it}"
            err = np.max(np.abs(l_g - l_o)) / (1 + np.max(np.abs(l_o)))
            worst = max(worst, err)
            assert err < 1e-8, (mv, it, err)
            lp_dev.copy_(torch.as_tensor(l_o, device="cuda"))
            before = c_o
        print(f"d={d} {kernel} {mv}: start logp err {err0:.2e}, worst step logp err {worst:.2e}")
        assert int(nacc.sum()) == sum(int(a.sum()) for _, _, _, a in steps)


# ---- degenerate snooker geometry, exact by construction.  Walker 0 is active in the first half step and takes walkers 8, 9, 10 as
# z, z1, z2; every other walker's record is inert (j2 == j1), so the whole ensemble must come back as it went in.
DEG_W = 16


def _degenerate(d, case):
    rng = np.random.RandomState(7 * d + len(case))
    c = rng.uniform(-2.5, 2.5, (DEG_W, d))
    e0 = np.zeros(d); e0[0] = 1.0
    if case == "s==z":
        c[0] = c[8]
    elif case == "q==z":
        c[0], c[8], c[9], c[10] = e0, 0.0, 0.0, 0.5 * e0
    else:
        c[10] = c[9]
    q, n, nq = sn.snooker_proposal(c[0:1], c[8:9], c[9:10], c[10:11], 2.0)
    return c, q[0], float(n[0]), float(nq[0])


def _degenerate_step(s, c, u):
    import torch
    from alabi_amd import _lib
    order = np.arange(DEG_W, dtype=np.int32)
    j1 = np.zeros(DEG_W, dtype=np.int32); j2 = np.zeros(DEG_W, dtype=np.int32); j3 = np.full(DEG_W, 2, dtype=np.int32)
    j2[0] = 1
    c_dev = torch.as_tensor(c, device="cuda").clone()
    lp_dev = s.compute_log_prob(c_dev)
    lp0 = lp_dev.cpu().numpy().copy()
    nacc = torch.zeros(DEG_W, dtype=torch.int64, device="cuda")
    dev = [torch.as_tensor(a, device="cuda") for a in (order, j1, j2, j3, np.full(DEG_W, u))]
    P = _lib.ptr
    rc = _lib.lib().alabi_ens_step_with_randoms_snooker(s._ens, P(c_dev), P(lp_dev), P(dev[0]), DEG_W // 2, P(dev[1]), P(dev[2]), P(dev[3]),
                                                        2.0, P(dev[4]), P(nacc), _lib.current_stream())
    _lib.check(rc, "step_with_randoms_snooker")
    torch.cuda.synchronize()
    return lp0, c_dev.cpu().numpy(), lp_dev.cpu().numpy(), nacc.cpu().numpy()


@pytest.mark.parametrize("case", ["s==z", "q==z"])
@pytest.mark.parametrize("d", [1, 2, 17])
def test_degenerate_snooker_step_is_a_no_op_without_nan(d, case):
    """s == z: n = 0 and q is NaN.  q == z (s = e_0, z = z1 = 0, z2 = e_0 / 2, gamma = 2): |q - z| = 0, the log factor is -inf and,
    at d = 1, 0 * (-inf) = NaN.  With u' = 1e-300 anything but a false accept test would move the walker."""
    c, q, n, nq = _degenerate(d, case)
    if case == "s==z":
        assert n == 0.0 and np.all(np.isnan(q))
    else:
        assert n == 1.0 and nq == 0.0 and np.array_equal(q, np.zeros(d))
        with np.errstate(divide="ignore", invalid="ignore"):
            lnfac = (d - 1.0) * (np.log(nq) - np.log(n))
        assert np.isnan(lnfac) if d == 1 else lnfac == -np.inf
    s = mc.sampler(mc.problem(d, "ExpSquared"), DEG_W, 1)
    lp0, c_g, l_g, nacc = _degenerate_step(s, c, 1e-300)
    assert np.array_equal(c_g, c) and np.array_equal(l_g, lp0) and not nacc.any()
    assert not np.isnan(c_g).any() and not np.isnan(l_g).any()


@pytest.mark.parametrize("d", [1, 2, 17])
def test_snooker_step_with_equal_projections_keeps_the_row(d):
    """z1 == z2: p = 0, q = s bit for bit and the log factor is 0; the row is the same whichever way the accept test falls (u' = 0.5:
    taken, u' = 1: the kernel's own value of logp(s) decides)."""
    c, q, n, nq = _degenerate(d, "z1==z2")
    assert np.array_equal(q, c[0]) and n == nq
    s = mc.sampler(mc.problem(d, "ExpSquared"), DEG_W, 1)
    for u in (0.5, 1.0):
        lp0, c_g, l_g, nacc = _degenerate_step(s, c, u)
        assert np.array_equal(c_g, c) and not nacc[1:].any() and np.array_equal(l_g[1:], lp0[1:])
        assert abs(l_g[0] - lp0[0]) < 1e-8 * (1 + abs(lp0[0])) and not np.isnan(l_g).any()
        assert nacc[0] == 1 if u == 0.5 else nacc[0] in (0, 1)


@pytest.mark.parametrize("case", ["s==z", "q==z"])
@pytest.mark.parametrize("d", [1, 2, 17])
def test_degenerate_snooker_proposal_on_the_host_callback_path(d, case):
    """The same two geometries through ens_propose_snooker_kernel and ens_accept_kernel: a production run draws its own partners, so
    the model's draws of step 0 say which rows the first active walker takes, and those rows are made the coincident ones.  The
    prior is the box on the host over the box-gated surrogate (gate_box=True: a NaN proposal is -inf, not a NaN log-probability,
    which run_mcmc would refuse as emcee does)."""
    from oracle.stretch_oracle import box_lnprior_batch
    W, seed = 12, 5
    prob = mc.problem(d, "ExpSquared")
    dr = sn.draw_steps_batched(seed, 0, 1, W, np.array([1.0]))
    order, n0 = dr["order"][0], dr["n0"]
    a = int(order[0])
    z, z1, z2 = (int(order[n0:][dr[k][0][a]]) for k in ("partner", "j2", "j3"))
    assert len({a, z, z1, z2}) == 4
    p0 = mc.start(prob, W, 3)
    e0 = np.zeros(d); e0[0] = 1.0
    if case == "s==z":
        p0[a] = p0[z]
    else:
        p0[a], p0[z], p0[z1], p0[z2] = e0, 0.0, 0.0, 0.5 * e0
    spec = [("snooker", 2.0, 1.0)]
    model = mc.BoxModel(prob)
    ref = sn.run_ensemble_moves(p0, 9, model, seed=seed, moves=spec)
    assert np.array_equal(ref[0][0][a], p0[a]) and 0 < ref[2].sum() and ref[2][a] < 9      # the model keeps the walker at step 0; others move
    s = mc.sampler(prob, W, seed, moves=mc.moves_objects(spec), prior_fn=lambda q: box_lnprior_batch(q, prob.bounds))
    lp0 = s.compute_log_prob(p0).cpu().numpy()
    st = s.run_mcmc(p0, 1, skip_initial_state_check=True)
    assert s.last_path == "host-callback"
    assert np.array_equal(st.coords[a], p0[a]) and st.log_prob[a] == lp0[a] and int(s._naccept[a]) == 0
    s.run_mcmc(None, 8)
    assert s.last_path == "host-callback" and int(s._naccept.sum()) > 0
    assert not np.isnan(s.get_chain()).any() and not np.isnan(s.get_log_prob()).any()
    assert not np.isnan(s.get_last_sample().coords).any()
