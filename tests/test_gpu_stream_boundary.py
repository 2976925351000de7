"""Chunk boundaries of the persistent ensemble kernel: the fused epilogue (chain, counters, walkers, row K -> row 0, sentinel
put back, step counters) must leave exactly what one launch per half step leaves, however a run is cut into calls and
chunks, also after a time-out and with several samplers alive."""
import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu

W, D = 16, 3
CHUNK = 1024                      # alabi_ens_create: chunk_cap = min(1024, 4 Mi / walkers)
NSTEPS = 2 * CHUNK + 37


@pytest.fixture(scope="module")
def setup():
    import torch
    from alabi_amd import HipGP
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    X, y, h = make_problem(150, D, 11, log_wn=-9.0)
    g = HipGP(D, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"]); g.compute(X)
    bounds = np.array([[-3.0, 3.0]] * D)
    return g, y, bounds


def _sampler(setup, monkeypatch, stream, seed=4, walkers=W):
    from alabi_amd import EnsembleSampler
    g, y, bounds = setup
    monkeypatch.setenv("ALABI_ENS_STREAM", stream)       # read when the sampler's handle is created (first run)
    return EnsembleSampler(walkers, D, g, y, bounds, seed=seed)


def _result(s):
    return (s.get_chain(), s.get_log_prob(), s._coords.cpu().numpy().copy(), s._logp.cpu().numpy().copy(),
            s._naccept.cpu().numpy().copy())


def _assert_same(a, b, what):
    for name, x, y in zip(("chain", "chain_logp", "walkers", "logp", "n_accept"), a, b):
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        assert np.array_equal(x, y), (what, name)


@pytest.mark.parametrize("thin", [1, 3])
def test_chunked_run_equals_single_chunk_calls_and_half_steps(setup, monkeypatch, thin):
    """2 chunk_cap + 37 steps in one call (three chunks, two carried rows) == the same steps as calls of at most one chunk ==
    one launch per half step: chain, chain_logp, final walkers, n_accept, bit for bit."""
    p0 = np.random.RandomState(1).uniform(-2, 2, (W, D))
    one = _sampler(setup, monkeypatch, "1")
    one.run_mcmc(p0, NSTEPS, thin_by=thin)
    assert one.last_path == "stream" and getattr(one, "stream_fallbacks", 0) == 0
    # single-chunk calls whose lengths are multiples of thin_by, so that the calls store the same steps as the one call
    first = CHUNK - CHUNK % thin
    parts = [first, first, NSTEPS - 2 * first]
    assert all(0 < n <= CHUNK and (n % thin == 0 or n == parts[-1]) for n in parts)
    cut = _sampler(setup, monkeypatch, "1")
    cut.run_mcmc(p0, parts[0], thin_by=thin)
    for n in parts[1:]:
        cut.run_mcmc(None, n, thin_by=thin)
        assert cut.last_path == "stream"
    half = _sampler(setup, monkeypatch, "0")
    half.run_mcmc(p0, NSTEPS, thin_by=thin)
    assert half.last_path == "launch-per-half-step"
    assert one.get_chain().shape[0] == NSTEPS // thin
    _assert_same(_result(one), _result(half), "one call / half steps")
    _assert_same(_result(cut), _result(half), "single-chunk calls / half steps")


def test_history_is_refilled_after_a_time_out(setup, monkeypatch):
    """A forced time-out in the middle call leaves the history half written: the next call on the persistent kernel must
    refill it instead of trusting the previous epilogue."""
    from alabi_amd import _lib
    p0 = np.random.RandomState(2).uniform(-2, 2, (W, D))
    n = CHUNK + 6                                          # two chunks per call
    ref = _sampler(setup, monkeypatch, "0")
    ref.run_mcmc(p0, n); ref.run_mcmc(None, n); ref.run_mcmc(None, n)
    s = _sampler(setup, monkeypatch, "1")
    s.run_mcmc(p0, n)
    assert s.last_path == "stream"
    monkeypatch.setenv("ALABI_ENS_SPIN_LIMIT", "1")        # the second half step can never be ready after one poll
    s.run_mcmc(None, n)
    monkeypatch.delenv("ALABI_ENS_SPIN_LIMIT")
    assert getattr(s, "stream_fallbacks", 0) == 1 and s.last_path == "launch-per-half-step"
    _lib.check(_lib.lib().alabi_ens_set_stream(s._ens, 1), "alabi_ens_set_stream")   # back to the persistent kernel
    s.run_mcmc(None, n)
    assert s.last_path == "stream" and s.stream_fallbacks == 1
    _assert_same(_result(s), _result(ref), "after a time-out")


def test_two_samplers_alive_at_once(setup, monkeypatch):
    """Each handle owns its history and its clean / dirty state: interleaved calls of two samplers do not disturb each other."""
    pa = np.random.RandomState(3).uniform(-2, 2, (W, D))
    pb = np.random.RandomState(4).uniform(-2, 2, (24, D))
    n = CHUNK + 11
    a = _sampler(setup, monkeypatch, "1", seed=7)
    b = _sampler(setup, monkeypatch, "1", seed=8, walkers=24)
    a.run_mcmc(pa, n); b.run_mcmc(pb, 50, thin_by=2); a.run_mcmc(None, 300); b.run_mcmc(None, n, thin_by=2); a.run_mcmc(None, n)
    assert a.last_path == "stream" and b.last_path == "stream"
    ra = _sampler(setup, monkeypatch, "0", seed=7)
    rb = _sampler(setup, monkeypatch, "0", seed=8, walkers=24)
    ra.run_mcmc(pa, n); ra.run_mcmc(None, 300); ra.run_mcmc(None, n)
    rb.run_mcmc(pb, 50, thin_by=2); rb.run_mcmc(None, n, thin_by=2)
    _assert_same(_result(a), _result(ra), "sampler a")
    _assert_same(_result(b), _result(rb), "sampler b")
