"""The boundary between two calls of the persistent ensemble path: one prologue launch (native save, row 0, flag), the proposal
buffer kept clean by the epilogue, the next call's first chunk of draws made ahead on the side stream, one read-back of flag and
walkers.  Whatever the call boundary does, a sampler must leave exactly what one launch per half step leaves (ALABI_ENS_STREAM=0,
same calls): chain, chain log-probabilities, final walkers, log-probabilities and acceptance counts, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu

W, D = 16, 3
CHUNK = 1024                      # alabi_ens_create: chunk_cap = min(1024, 4 Mi / walkers)
NOT_COMPUTED = 4                  # ALABI_NOT_COMPUTED


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


def _sampler(setup, monkeypatch, stream, seed=4, walkers=W, **kw):
    from alabi_amd import EnsembleSampler
    g, y, bounds = setup
    monkeypatch.setenv("ALABI_ENS_STREAM", stream)       # read when the sampler's handle is created: here, not at its first run
    s = EnsembleSampler(walkers, D, g, y, bounds, seed=seed, **kw)
    s._ensure_ens()
    return s


def _result(s):
    return (s.get_chain(), s.get_log_prob(), s._coords.cpu().numpy().copy(), s._logp.cpu().numpy().copy(),
            s._naccept.cpu().numpy().copy())


def _assert_same(a, b, what):
    for name, x, y in zip(("chain", "chain_logp", "walkers", "logp", "n_accept"), a, b):
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        assert np.array_equal(x, y), (what, name)


def _stats(s):
    """(draw-ahead hits, misses, prop fills, hist fills) of the sampler's handle."""
    from alabi_amd import _lib
    out = (C.c_longlong * 4)()
    _lib.check(_lib.lib().alabi_ens_boundary_stats(s._ens, out), "alabi_ens_boundary_stats")
    return tuple(int(v) for v in out)


def _both(s, ref, what, *args, **kw):
    """The same run_mcmc call on the sampler under test and on the reference; everything equal afterwards."""
    st = s.run_mcmc(*args, **kw)
    ref.run_mcmc(*args, **kw)
    _assert_same(_result(s), _result(ref), what)
    return st


def _set_stretch_table(s, a):
    from alabi_amd import _lib
    _lib.check(_lib.lib().alabi_ens_set_moves(s._ens, 1, (C.c_int * 1)(0), _lib.host_doubles([1.0]), _lib.host_doubles([a]),
                                              _lib.host_doubles([0.0])), "alabi_ens_set_moves")


def test_draw_ahead_hit_and_miss(setup, monkeypatch):
    """Calls of one, two and three chunks, first chunks shorter than and equal to the cap: every call after the first finds its
    first chunk drawn ahead; a changed `a`, a changed move table miss; a restart that keeps the draw counter hits; a draw entry
    point between two calls does no harm.  Equal to the reference after every call."""
    from alabi_amd import _lib
    p0 = np.random.RandomState(1).uniform(-2, 2, (W, D))
    s, ref = _sampler(setup, monkeypatch, "1"), _sampler(setup, monkeypatch, "0")
    _both(s, ref, "call 0", p0, 40)
    assert s.last_path == "stream" and ref.last_path == "launch-per-half-step"
    for i, n in enumerate((1030, 7, 1024, 2085)):
        _both(s, ref, "call %d" % (i + 1), None, n)
        assert s.last_path == "stream"
    hits, misses = _stats(s)[:2]
    assert hits >= 4 and misses == 1
    s.a = ref.a = 2.5                                       # the records made ahead carry a = 2: drawn again
    _both(s, ref, "changed a", None, 50)
    assert _stats(s)[:2] == (hits, misses + 1)
    _both(s, ref, "same a again", None, 50)
    assert _stats(s)[:2] == (hits + 1, misses + 1)
    for x in (s, ref):
        _set_stretch_table(x, 1.7)                          # another stretch-only table: still the persistent path, other records
    _both(s, ref, "changed move table", None, 50)
    assert s.last_path == "stream" and _stats(s)[:2] == (hits + 1, misses + 2)
    p1 = np.random.RandomState(5).uniform(-2, 2, (W, D))
    _both(s, ref, "restart", p1, 60)                        # new walkers, the draw counter goes on: the records are still the right ones
    assert _stats(s)[:2] == (hits + 2, misses + 2)
    for x in (s, ref):                                      # a draw entry point between two calls (it writes the first buffer set)
        _lib.check(_lib.lib().alabi_ens_draw(x._ens, 3, 20, 2.0, _lib.current_stream()), "alabi_ens_draw")
    import torch
    torch.cuda.synchronize()
    _both(s, ref, "after alabi_ens_draw", None, CHUNK + 3)
    assert s.last_path == "stream" and getattr(s, "stream_fallbacks", 0) == 0
    assert sum(_stats(s)[:2]) == 10                         # whichever way it counted


def test_prop_clean_and_dirty(setup, monkeypatch):
    """Pair variant: the proposal buffer is filled once, on first use; afterwards the epilogue keeps it clean.  A time-out of the
    middle call (pair, retried on the single variant, then the launch-per-half-step fallback) leaves both buffers dirty.  A
    time-out turns the pair variant off for the handle, so the next persistent call runs on ens_stream_kernel: it refills the
    history (one fill launch), and the proposal buffer is not used again (its fill count stays at the one of first use)."""
    from alabi_amd import _lib
    p0 = np.random.RandomState(2).uniform(-2, 2, (W, D))
    s, ref = _sampler(setup, monkeypatch, "1"), _sampler(setup, monkeypatch, "0")
    _both(s, ref, "call 0", p0, 1030)
    assert s.last_stream_variant == "pair"
    assert _stats(s)[2:] == (1, 1)
    _both(s, ref, "call 1", None, 40)
    _both(s, ref, "call 2", None, 1030)
    assert s.last_stream_variant == "pair"
    assert _stats(s)[2:] == (1, 1)                          # no fill of either buffer after the first call
    t, tref = _sampler(setup, monkeypatch, "1", seed=9), _sampler(setup, monkeypatch, "0", seed=9)
    _both(t, tref, "t call 0", p0, 1030)
    assert t.last_stream_variant == "pair" and _stats(t)[2:] == (1, 1)
    monkeypatch.setenv("ALABI_ENS_SPIN_LIMIT", "1")         # the second half step can never be ready after one poll
    _both(t, tref, "t timed out", None, 40)
    monkeypatch.delenv("ALABI_ENS_SPIN_LIMIT")
    assert t.stream_fallbacks == 1 and t.last_path == "launch-per-half-step"
    before = _stats(t)
    _lib.check(_lib.lib().alabi_ens_set_stream(t._ens, 1), "alabi_ens_set_stream")
    _both(t, tref, "t after the time-out", None, 1030)
    assert t.last_path == "stream" and t.last_stream_variant == "single"
    after = _stats(t)
    assert after[3] - before[3] == 1 and after[2] == 1
    _both(t, tref, "t clean again", None, 1030)
    assert _stats(t)[2:] == after[2:]


@pytest.mark.parametrize("pair,ensembles", [("0", 1), (None, 1), (None, 2)])
def test_native_save_and_restore(setup, monkeypatch, pair, ensembles):
    """A forced time-out: the single variant goes straight to the Python fallback (ALABI_ENS_PAIR=0), the pair variant goes to the
    single variant first; also with two ensembles.  The walkers, log-probabilities and counters the fallback starts from are those
    the call saved natively."""
    if pair is None:
        monkeypatch.delenv("ALABI_ENS_PAIR", raising=False)
    else:
        monkeypatch.setenv("ALABI_ENS_PAIR", pair)
    p0 = np.random.RandomState(3).uniform(-2, 2, (W * ensembles, D))
    s = _sampler(setup, monkeypatch, "1", n_ensembles=ensembles)
    ref = _sampler(setup, monkeypatch, "0", n_ensembles=ensembles)
    _both(s, ref, "call 0", p0, 30)
    assert s.last_path == "stream" and s.last_stream_variant == ("single" if pair == "0" else "pair")
    monkeypatch.setenv("ALABI_ENS_SPIN_LIMIT", "1")
    st = _both(s, ref, "timed-out call", None, CHUNK + 5)
    monkeypatch.delenv("ALABI_ENS_SPIN_LIMIT")
    assert s.stream_fallbacks == 1 and s.last_path == "launch-per-half-step"
    assert np.array_equal(st.coords, s._coords.cpu().numpy()) and np.array_equal(st.log_prob, s._logp.cpu().numpy())


def _last_state(s):
    from alabi_amd import _lib
    c = np.empty((s.total_walkers, s.ndim)); lp = np.empty(s.total_walkers)
    return _lib.lib().alabi_ens_last_state(s._ens, C.c_void_p(c.ctypes.data), C.c_void_p(lp.ctypes.data)), c, lp


def _state_is_walkers(st, s, what):
    assert np.array_equal(st.coords, s._coords.cpu().numpy()), what
    assert np.array_equal(st.log_prob, s._logp.cpu().numpy()), what
    assert st.coords.shape == (s.total_walkers, s.ndim) and st.log_prob.shape == (s.total_walkers,)


def test_returned_state(setup, monkeypatch):
    """The State run_mcmc returns is the walkers on the device, bit for bit: persistent path with one, two and three chunks, two
    ensembles, after a fallback, and on the launch-per-half-step path of a DE move.  alabi_ens_last_state refuses before any call
    and after a timed-out one."""
    from alabi_amd import _lib
    from alabi_amd.moves import DEMove
    p0 = np.random.RandomState(6).uniform(-2, 2, (W, D))
    s = _sampler(setup, monkeypatch, "1")
    s._ensure_ens()
    assert _last_state(s)[0] == NOT_COMPUTED
    st = s.run_mcmc(p0, 20)
    for n in (CHUNK, CHUNK + 9, 2 * CHUNK + 9):
        st = s.run_mcmc(None, n)
        assert s.last_path == "stream"
        _state_is_walkers(st, s, n)
        rc, c, lp = _last_state(s)
        assert rc == _lib.OK and np.array_equal(c, st.coords) and np.array_equal(lp, st.log_prob)
    monkeypatch.setenv("ALABI_ENS_SPIN_LIMIT", "1")
    st = s.run_mcmc(None, 33)
    monkeypatch.delenv("ALABI_ENS_SPIN_LIMIT")
    assert s.stream_fallbacks == 1
    _state_is_walkers(st, s, "after a fallback")
    assert _last_state(s)[0] == NOT_COMPUTED
    two = _sampler(setup, monkeypatch, "1", n_ensembles=2)
    st = two.run_mcmc(np.random.RandomState(7).uniform(-2, 2, (2 * W, D)), CHUNK + 2)
    assert two.last_path == "stream"
    _state_is_walkers(st, two, "two ensembles")
    de = _sampler(setup, monkeypatch, "1", moves=DEMove())
    st = de.run_mcmc(p0, 25)
    assert de.last_path == "launch-per-half-step"
    _state_is_walkers(st, de, "DE move")
    assert _last_state(de)[0] == NOT_COMPUTED


def test_two_handles_alive(setup, monkeypatch):
    """Interleaved calls of two samplers: each handle keeps its own ahead-draws, save area and clean counts."""
    pa = np.random.RandomState(3).uniform(-2, 2, (W, D))
    pb = np.random.RandomState(4).uniform(-2, 2, (24, D))
    a, ra = _sampler(setup, monkeypatch, "1", seed=7), _sampler(setup, monkeypatch, "0", seed=7)
    b, rb = _sampler(setup, monkeypatch, "1", seed=8, walkers=24), _sampler(setup, monkeypatch, "0", seed=8, walkers=24)
    _both(a, ra, "a0", pa, CHUNK + 11)
    _both(b, rb, "b0", pb, 50)
    _both(a, ra, "a1", None, 300)
    _both(b, rb, "b1", None, CHUNK + 11)
    _both(a, ra, "a2", None, CHUNK + 11)
    _both(b, rb, "b2", None, 7)
    assert a.last_path == "stream" and b.last_path == "stream"
    assert _stats(a)[:2] == (2, 1) and _stats(b)[:2] == (2, 1)
    assert _stats(a)[2:] == (1, 1)                          # first use
    assert _stats(b)[2:] == (2, 2)                          # first use (50 rows), then the first call that polls more rows than that
