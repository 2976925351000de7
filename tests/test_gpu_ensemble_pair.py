"""Pair variant of the persistent ensemble kernel (ens_pair_kernel: two workgroups per list position, which evaluate both
outcomes of a pending update): chain, chain log-probability, final walkers, log-probability and acceptance counters equal
those of one launch per half step byte for byte, for every shape and option at which the kernel takes another path; the
per-class counters equal what the draws say; the variant is chosen, refused and switched off as documented."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu

NSTEPS = 300


@pytest.fixture(scope="module")
def problems():
    """(d, N, kernel) -> (gp, y); built once, never changed."""
    import torch
    from alabi_amd import HipGP
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    cache = {}

    def get(d, N=150, kernel="ExpSquaredKernel"):
        key = (d, N, kernel)
        if key not in cache:
            X, y, h = make_problem(N, d, 11 + d, log_wn=-9.0)
            g = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel)
            g.compute(X)
            cache[key] = (g, y)
        return cache[key]
    return get


def _sampler(problem, monkeypatch, stream, W, d, half_width=3.0, seed=4, **kw):
    from alabi_amd import EnsembleSampler
    g, y = problem
    monkeypatch.setenv("ALABI_ENS_STREAM", stream)       # read when the sampler's handle is created (first run)
    return EnsembleSampler(W, d, g, y, np.array([[-half_width, half_width]] * d), seed=seed, live_dangerously=True, **kw)


def _result(s):
    return (s.get_chain(), s.get_log_prob(), s._coords.cpu().numpy().copy(), s._logp.cpu().numpy().copy(),
            s._naccept.cpu().numpy().copy())


def _assert_same(a, b, what):
    for name, x, y in zip(("chain", "chain_logp", "walkers", "logp", "n_accept"), a, b):
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), (what, name)


def _compare(problem, monkeypatch, W, d, nsteps=NSTEPS, thin=1, variant="pair", p0_width=2.0, **kw):
    E = kw.get("n_ensembles", 1)
    p0 = np.random.RandomState(W + d).uniform(-p0_width, p0_width, (W * E, d))
    s = _sampler(problem, monkeypatch, "1", W, d, **kw)
    s.run_mcmc(p0, nsteps, thin_by=thin)
    assert s.last_path == "stream" and s.last_stream_kernel == "ens_stream_kernel"
    assert s.last_stream_variant == variant and getattr(s, "stream_fallbacks", 0) == 0
    ref = _sampler(problem, monkeypatch, "0", W, d, **kw)
    ref.run_mcmc(p0, nsteps, thin_by=thin)
    assert ref.last_path == "launch-per-half-step" and ref.last_stream_variant is None
    _assert_same(_result(s), _result(ref), (W, d, kw))
    return s


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("W", [4, 5, 16, 24])
def test_shapes(problems, monkeypatch, W, d):
    """The smallest pair grid, an odd W (n0 != n1: the last pair has no item in the second half step), several pairs."""
    _compare(problems(d), monkeypatch, W, d)


def test_headline_dimension_bucket(problems, monkeypatch):
    _compare(problems(10), monkeypatch, 16, 10)


def test_one_point_pair_per_lane_with_padded_lanes(problems, monkeypatch):
    _compare(problems(3, N=70), monkeypatch, 16, 3)


def test_two_ensembles(problems, monkeypatch):
    _compare(problems(3), monkeypatch, 16, 3, n_ensembles=2)


def test_two_chunks_thinned(problems, monkeypatch):
    """1024 + 37 steps: prop is refilled for the second chunk, row K of the first is row 0 of the second."""
    s = _compare(problems(3), monkeypatch, 16, 3, nsteps=1024 + 37, thin=3)
    assert s.get_chain().shape[0] == (1024 + 37) // 3


def test_matern_kernel(problems, monkeypatch):
    """The GENERIC instantiation."""
    _compare(problems(3, kernel="Matern32Kernel"), monkeypatch, 16, 3)


def test_normal_prior_and_logp_affine(problems, monkeypatch):
    pm, ps = np.array([0.3, np.nan, -0.2]), np.array([1.5, np.nan, 0.8])
    _compare(problems(3), monkeypatch, 16, 3, logp_affine=(0.7, -1.25), normal_prior=(pm, ps))


def test_out_of_bounds_proposals(problems, monkeypatch):
    """A box so tight in ten dimensions that most proposals leave it: they are still published, and the workgroup that
    assumes "accepted" always loses on them."""
    _compare(problems(10), monkeypatch, 16, 10, half_width=0.25, p0_width=0.25)


# (compute lanes, training points) -> point pairs per lane = ceil(Npad / 2 / lanes), Npad = N rounded up to 64
LADDER_ROWS = [(256, 150, 1), (256, 600, 2), (256, 1100, 3), (256, 1600, 4), (512, 150, 1), (512, 1100, 2)]


@pytest.mark.parametrize("lanes,N,ppt", LADDER_ROWS)
def test_every_row_of_the_launch_table(problems, monkeypatch, lanes, N, ppt):
    """One configuration per (compute lanes, point pairs per lane) row of the persistent kernels' launch table: the pair kernel
    and the single kernel of that row run, and their chains are those of one launch per half step with the same lanes."""
    npad = -(-N // 64) * 64
    assert -(-(npad // 2) // lanes) == ppt
    W, d, nsteps = 8, 3, 4
    monkeypatch.setenv("ALABI_ENS_THREADS", str(lanes))  # read, like ALABI_ENS_STREAM, when the sampler's handle is created
    s = _compare(problems(d, N=N), monkeypatch, W, d, nsteps=nsteps)
    monkeypatch.setenv("ALABI_ENS_PAIR", "0")
    single = _sampler(problems(d, N=N), monkeypatch, "1", W, d)
    single.run_mcmc(np.random.RandomState(W + d).uniform(-2.0, 2.0, (W, d)), nsteps)
    assert single.last_path == "stream" and single.last_stream_variant == "single" and getattr(single, "stream_fallbacks", 0) == 0
    _assert_same(_result(single), _result(s), (lanes, N, ppt))


def _host_class_counts(s, W, nsteps):
    """Items per class from the exported draws (labels of consecutive steps): class = number of input rows of a proposal that
    the immediately preceding half step produced."""
    import torch
    from alabi_amd import _lib
    counts = [0, 0, 0]
    prev_second = None
    for t in range(nsteps):
        order = torch.empty(W, dtype=torch.int32, device="cuda"); partner = torch.empty_like(order); cw = torch.empty_like(order)
        u_z = torch.empty(W, dtype=torch.float64, device="cuda"); u_acc = torch.empty_like(u_z); zz = torch.empty_like(u_z)
        n0 = C.c_int(0)
        _lib.check(_lib.lib().alabi_ens_export_draws(s._ens, t, 2.0, _lib.ptr(order), C.byref(n0), _lib.ptr(u_z), _lib.ptr(partner),
                                                     _lib.ptr(u_acc), _lib.ptr(cw), _lib.ptr(zz), _lib.current_stream()), "export")
        torch.cuda.synchronize()
        order, cw = order.cpu().numpy(), cw.cpu().numpy()
        for pos in range(n0.value):                   # first half step: fresh iff the walker was in the second list of step t - 1
            fresh = 0 if prev_second is None else int(order[pos] in prev_second) + int(cw[pos] in prev_second)
            counts[fresh] += 1
        counts[1] += W - n0.value                     # second half step: the partner row is fresh, the own row is not
        prev_second = set(order[n0.value:].tolist())
    return counts


def test_class_counts_match_the_draws(problems, monkeypatch):
    from alabi_amd import _lib
    W, d, nsteps = 16, 3, 200
    s = _sampler(problems(d), monkeypatch, "1", W, d)
    s._ensure_ens()
    out = (C.c_longlong * 9)()
    _lib.check(_lib.lib().alabi_ens_pair_stats(s._ens, out, 1), "alabi_ens_pair_stats")      # switches counting on
    s.run_mcmc(np.random.RandomState(2).uniform(-2, 2, (W, d)), nsteps)
    assert s.last_stream_variant == "pair"
    _lib.check(_lib.lib().alabi_ens_pair_stats(s._ens, out, 1), "alabi_ens_pair_stats")
    got = np.array(list(out)).reshape(3, 3)           # class x (items, rows stored by R, rows stored by A)
    print(got)
    want = _host_class_counts(s, W, nsteps)
    assert got[:, 0].tolist() == want and min(want) > 0
    assert got[0].tolist() == [want[0], want[0], 0] and got[2].tolist() == [want[2], want[2], 0]
    assert got[1, 1] + got[1, 2] == want[1] and got[1, 1] > 0 and got[1, 2] > 0


def test_variant_switched_off(problems, monkeypatch):
    monkeypatch.setenv("ALABI_ENS_PAIR", "0")
    _compare(problems(3), monkeypatch, 16, 3, variant="single")


def test_more_pairs_than_compute_units(problems, monkeypatch):
    """W = 300: 2 ceil(W / 2) = 300 workgroups do not fit one per CU, the single kernel runs."""
    _compare(problems(3), monkeypatch, 300, 3, nsteps=60, variant="single")


def test_forced_time_out(problems, monkeypatch):
    """A spin limit of one poll in the middle call: the pair variant and the retry on the single kernel both time out, the call
    falls back to one launch per half step once, and the handle has turned the pair variant off."""
    from alabi_amd import _lib
    W, d, n = 16, 3, 120
    p0 = np.random.RandomState(2).uniform(-2, 2, (W, d))
    ref = _sampler(problems(d), monkeypatch, "0", W, d)
    ref.run_mcmc(p0, n); ref.run_mcmc(None, n); ref.run_mcmc(None, n)
    s = _sampler(problems(d), monkeypatch, "1", W, d)
    s.run_mcmc(p0, n)
    assert s.last_path == "stream" and s.last_stream_variant == "pair"
    monkeypatch.setenv("ALABI_ENS_SPIN_LIMIT", "1")
    s.run_mcmc(None, n)
    monkeypatch.delenv("ALABI_ENS_SPIN_LIMIT")
    assert getattr(s, "stream_fallbacks", 0) == 1 and s.last_path == "launch-per-half-step"
    _lib.check(_lib.lib().alabi_ens_set_stream(s._ens, 1), "alabi_ens_set_stream")
    s.run_mcmc(None, n)
    assert s.last_path == "stream" and s.last_stream_variant == "single" and s.stream_fallbacks == 1
    _assert_same(_result(s), _result(ref), "after a time-out")
