"""Fetch-ahead of the pair kernel's hand-off wave (ens_pair_kernel: the next item's input words are loaded in the idle window
of the current item and the poll is skipped when none of them is the sentinel): chain, chain log-probability, final walkers,
log-probability and acceptance counters equal those of one launch per half step byte for byte at the shapes where the
fetched words are most often not there yet, where the next item is absent or belongs to the next launch, and after a forced
time-out; the fetch-ahead counters of alabi_ens_pair_stats2 are consistent with the items the draws prescribe."""
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


def _compare(problem, monkeypatch, W, d, nsteps=NSTEPS, thin=1, p0_width=2.0, **kw):
    """The pair kernel against one launch per half step (ALABI_ENS_STREAM=0), no fallback on the way."""
    E = kw.get("n_ensembles", 1)
    p0 = np.random.RandomState(W + d).uniform(-p0_width, p0_width, (W * E, d))
    s = _sampler(problem, monkeypatch, "1", W, d, **kw)
    s.run_mcmc(p0, nsteps, thin_by=thin)
    assert s.last_path == "stream" and s.last_stream_variant == "pair" and getattr(s, "stream_fallbacks", 0) == 0
    ref = _sampler(problem, monkeypatch, "0", W, d, **kw)
    ref.run_mcmc(p0, nsteps, thin_by=thin)
    assert ref.last_path == "launch-per-half-step" and ref.last_stream_variant is None
    _assert_same(_result(s), _result(ref), (W, d, kw))
    return s


@pytest.mark.parametrize("d", [1, 3])
def test_two_pairs_inputs_stored_one_item_earlier(problems, monkeypatch, d):
    """W = 4: an item's inputs are very often the row its own pair stored one item earlier, so the fetched words are the
    sentinel and the wave falls back to the poll."""
    _compare(problems(d), monkeypatch, 4, d)


@pytest.mark.parametrize("W", [5, 7])
def test_odd_walkers_next_item_absent(problems, monkeypatch, W):
    """The last pair has no item in the second half step: its fetch-ahead targets the next step's item."""
    _compare(problems(3), monkeypatch, W, 3)


def test_headline_dimension_bucket(problems, monkeypatch):
    _compare(problems(10), monkeypatch, 16, 10)


def test_two_ensembles(problems, monkeypatch):
    _compare(problems(3), monkeypatch, 24, 3, n_ensembles=2)


def test_two_chunks_thinned(problems, monkeypatch):
    """1024 + 37 steps: the last item of a launch fetches row 0, prop is refilled, row K of the first chunk is row 0 of the second."""
    s = _compare(problems(3), monkeypatch, 16, 3, nsteps=1024 + 37, thin=3)
    assert s.get_chain().shape[0] == (1024 + 37) // 3


def test_out_of_bounds_proposals(problems, monkeypatch):
    """A box so tight in ten dimensions that most proposals leave it: they are still published (a reader that waited for an
    unpublished proposal would time out: _compare asserts that nothing fell back)."""
    _compare(problems(10), monkeypatch, 16, 10, half_width=0.25, p0_width=0.25)


def test_matern_kernel(problems, monkeypatch):
    """The GENERIC instantiation."""
    _compare(problems(3, kernel="Matern32Kernel"), monkeypatch, 16, 3)


def test_normal_prior_and_logp_affine(problems, monkeypatch):
    pm, ps = np.array([0.3, np.nan, -0.2]), np.array([1.5, np.nan, 0.8])
    _compare(problems(3), monkeypatch, 16, 3, logp_affine=(0.7, -1.25), normal_prior=(pm, ps))


def test_forced_time_out(problems, monkeypatch):
    """W = 5, a spin limit of one poll in the middle call: the kernel's own bounded exit (with fetched words in registers) and
    the fallback; the three calls together equal the reference."""
    from alabi_amd import _lib
    W, d, n = 5, 3, 120
    p0 = np.random.RandomState(2).uniform(-2, 2, (W, d))
    ref = _sampler(problems(d), monkeypatch, "0", W, d)
    ref.run_mcmc(p0, n); ref.run_mcmc(None, n); ref.run_mcmc(None, n)
    s = _sampler(problems(d), monkeypatch, "1", W, d)
    s.run_mcmc(p0, n)
    assert s.last_path == "stream" and s.last_stream_variant == "pair"
    monkeypatch.setenv("ALABI_ENS_SPIN_LIMIT", "1")
    s.run_mcmc(None, n)
    monkeypatch.delenv("ALABI_ENS_SPIN_LIMIT")
    print("stream_fallbacks", getattr(s, "stream_fallbacks", 0), "path", s.last_path)
    assert getattr(s, "stream_fallbacks", 0) == 1 and s.last_path == "launch-per-half-step"
    _lib.check(_lib.lib().alabi_ens_set_stream(s._ens, 1), "alabi_ens_set_stream")
    s.run_mcmc(None, n)
    assert s.last_path == "stream" and s.stream_fallbacks == 1
    _assert_same(_result(s), _result(ref), "after a time-out")


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


def test_fetch_ahead_counters(problems, monkeypatch):
    """alabi_ens_pair_stats2 (six words; the two slot counters are kept for a two-slot proposal array and stay 0): both workgroups of a pair step through every item; the workgroup that assumes "rejected" reads rows
    that are at least one verdict old, so the fetch-ahead finds some of them complete, never more than there are items (item 0
    of a launch has no fetch-ahead).  alabi_ens_pair_stats keeps its meaning beside it."""
    from alabi_amd import _lib
    W, d, nsteps = 16, 3, 200
    s = _sampler(problems(d), monkeypatch, "1", W, d)
    s._ensure_ens()
    out = (C.c_longlong * 9)()
    out2 = (C.c_longlong * 6)()
    _lib.check(_lib.lib().alabi_ens_pair_stats(s._ens, out, 1), "alabi_ens_pair_stats")      # switches counting on
    _lib.check(_lib.lib().alabi_ens_pair_stats2(s._ens, out2, 1), "alabi_ens_pair_stats2")
    assert list(out2) == [0] * 6
    s.run_mcmc(np.random.RandomState(2).uniform(-2, 2, (W, d)), nsteps)
    assert s.last_stream_variant == "pair"
    _lib.check(_lib.lib().alabi_ens_pair_stats(s._ens, out, 1), "alabi_ens_pair_stats")
    _lib.check(_lib.lib().alabi_ens_pair_stats2(s._ens, out2, 1), "alabi_ens_pair_stats2")
    got = np.array(list(out)).reshape(3, 3)           # class x (items, rows stored by R, rows stored by A)
    r_items, r_ahead, a_items, a_ahead, slot_r, slot_a = list(out2)
    print(got, list(out2))
    want = _host_class_counts(s, W, nsteps)
    assert r_items == sum(want) and a_items == sum(want)
    assert 0 < r_ahead <= r_items - W // 2            # the first item of each of the W / 2 pairs polls
    assert 0 <= a_ahead <= a_items - W // 2
    assert slot_r == 0 and slot_a == 0                # kept for a two-slot proposal array: prop has one slot
    assert got[:, 0].tolist() == want and min(want) > 0
    assert got[0].tolist() == [want[0], want[0], 0] and got[2].tolist() == [want[2], want[2], 0]
    assert got[1, 1] + got[1, 2] == want[1] and got[1, 1] > 0 and got[1, 2] > 0
    _lib.check(_lib.lib().alabi_ens_pair_stats2(s._ens, out2, 0), "alabi_ens_pair_stats2")
    assert list(out2) == [0] * 6                 # read and cleared
