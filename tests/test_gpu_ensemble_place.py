"""Placement of the pair ensemble kernel's items by XCD class (ens_place_kernel, the XCD map of ens_pair_kernel): results are
byte-equal with placement on, off and on the single kernel; the pair of every item, the permuted records and the counters
are those of the NumPy model (tests/place_numpy.py); placement stays off where it does not apply."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_problem
from place_numpy import place_chunk

pytestmark = pytest.mark.gpu

D, N, NSTEPS, CHUNK = 2, 64, 202, 128      # two chunks: 128 + 74 steps, the second with a short last segment


@pytest.fixture(scope="module")
def setup():
    import torch
    from alabi_amd import HipGP
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    X, y, h = make_problem(N, D, 13, log_wn=-9.0)
    g = HipGP(D, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"]); g.compute(X)
    return g, y, np.array([[-3.0, 3.0]] * D)


def _sampler(setup, monkeypatch, W, place="1", pair="1", stream="1", chunk=CHUNK, **kw):
    from alabi_amd import EnsembleSampler
    g, y, bounds = setup
    monkeypatch.setenv("ALABI_ENS_STREAM", stream)       # all four are read by the handle: at its creation or at its first run
    monkeypatch.setenv("ALABI_ENS_PAIR", pair)
    monkeypatch.setenv("ALABI_ENS_PLACE", place)
    monkeypatch.setenv("ALABI_ENS_CHUNK", str(chunk))
    return EnsembleSampler(W, D, g, y, bounds, seed=5, **kw)


def _result(s):
    return (s.get_chain(), s.get_log_prob(), s._coords.cpu().numpy().copy(), s._logp.cpu().numpy().copy(),
            s._naccept.cpu().numpy().copy())


def _assert_same(a, b, what):
    for name, x, y in zip(("chain", "chain_logp", "walkers", "logp", "n_accept"), a, b):
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), (what, name)


def _stats(s, reset=0):
    from alabi_amd import _lib
    out = (C.c_longlong * 3)()
    _lib.check(_lib.lib().alabi_ens_place_stats(s._ens, out, reset), "alabi_ens_place_stats")
    return list(out)


def _export(s, step0, n, WT):
    """(place [n, WT], packed [n, WT, 4], packed_x [n, WT, 4]) of steps step0 .. step0 + n - 1 placed as one chunk."""
    import torch
    from alabi_amd import _lib
    place = torch.zeros(n * WT, dtype=torch.int32, device="cuda")
    packed = torch.zeros(n * WT * 4, dtype=torch.int64, device="cuda")
    packed_x = torch.zeros_like(packed)
    _lib.check(_lib.lib().alabi_ens_export_placement(s._ens, step0, n, s.a, _lib.ptr(place), _lib.ptr(packed), _lib.ptr(packed_x),
                                                     _lib.current_stream()), "alabi_ens_export_placement")
    torch.cuda.synchronize()
    return (place.cpu().numpy().reshape(n, WT), packed.cpu().numpy().view(np.uint64).reshape(n, WT, 4),
            packed_x.cpu().numpy().view(np.uint64).reshape(n, WT, 4))


def _run_three(setup, monkeypatch, W, calls, **kw):
    """The same calls with placement on, off, and on the single kernel; returns the sampler with placement on."""
    p0 = np.random.RandomState(W).uniform(-2, 2, (W * kw.get("n_ensembles", 1), D))
    out = []
    for place, pair in (("1", "1"), ("0", "1"), ("1", "0")):
        s = _sampler(setup, monkeypatch, W, place=place, pair=pair, **kw)
        s.run_mcmc(p0, calls[0])
        for n in calls[1:]:
            s.run_mcmc(None, n)
        assert s.last_path == "stream" and getattr(s, "stream_fallbacks", 0) == 0
        assert s.last_stream_variant == ("pair" if pair == "1" else "single")
        out.append(s)
    _assert_same(_result(out[0]), _result(out[1]), "placement on / off")
    _assert_same(_result(out[0]), _result(out[2]), "placement on / single kernel")
    assert _stats(out[1])[0] == 0 and _stats(out[2]) == [0, 0, 0]
    return out[0]


@pytest.mark.parametrize("W", [16, 64])
def test_placement_equals_model_and_changes_no_result(setup, monkeypatch, W):
    """W = 16: one pair per class, capacity 1, every conflict path.  202 steps in two chunks."""
    s = _run_three(setup, monkeypatch, W, [NSTEPS])
    on, n_pref, n_hit = _stats(s)
    assert on == 1
    n0 = W // 2
    model_pref = model_hit = 0
    for step0, n in ((0, CHUNK), (CHUNK, NSTEPS - CHUNK)):
        place, packed, packed_x = _export(s, step0, n, W)
        order = (packed[:, :, 0] & np.uint64(0xffffffff)).astype(np.int64)
        cw = (packed[:, :, 0] >> np.uint64(32)).astype(np.int64)
        m_place, a, b = place_chunk(order, cw)
        assert np.array_equal(place, m_place), (W, step0)
        model_pref += a; model_hit += b
        for lo in (0, n0):                                # the permuted records: position = pair, within every (step, half)
            idx = lo + place[:, lo:lo + n0]
            moved = np.take_along_axis(packed_x, idx[:, :, None], axis=1)
            assert np.array_equal(moved, packed[:, lo:lo + n0]), (W, step0, lo)
            assert all(sorted(r.tolist()) == list(range(n0)) for r in place[:, lo:lo + n0])
    assert (n_pref, n_hit) == (model_pref, model_hit) and 0 < n_hit <= n_pref
    assert _stats(s)[1:] == [n_pref, n_hit]               # the exports count nothing


def test_placement_is_off_where_the_lists_have_no_whole_classes(setup, monkeypatch):
    s = _run_three(setup, monkeypatch, 20, [NSTEPS])      # n0 = 10
    assert _stats(s) == [0, 0, 0]


def test_second_call_and_reset(setup, monkeypatch):
    """The second call finds its first chunk drawn and placed ahead; reset() forgets the chain, not the draw counter."""
    p0 = np.random.RandomState(3).uniform(-2, 2, (16, D))
    res = []
    for place in ("1", "0"):
        s = _sampler(setup, monkeypatch, 16, place=place)
        s.run_mcmc(p0, 150)
        s.run_mcmc(None, 40)
        s.reset()
        s.run_mcmc(None, 150)
        assert s.last_stream_variant == "pair" and _stats(s)[0] == int(place)
        res.append(_result(s))
    _assert_same(res[0], res[1], "second call and reset")


def test_after_a_time_out(setup, monkeypatch):
    """A forced time-out: the second run of the call is on the single kernel and reads the records as drawn; so does every
    later call of the handle."""
    from alabi_amd import _lib
    p0 = np.random.RandomState(4).uniform(-2, 2, (16, D))
    ref = _sampler(setup, monkeypatch, 16, stream="0")
    ref.run_mcmc(p0, 150); ref.run_mcmc(None, 150); ref.run_mcmc(None, 150)
    s = _sampler(setup, monkeypatch, 16)
    s.run_mcmc(p0, 150)
    assert s.last_stream_variant == "pair" and _stats(s)[0] == 1
    monkeypatch.setenv("ALABI_ENS_SPIN_LIMIT", "1")
    s.run_mcmc(None, 150)
    monkeypatch.delenv("ALABI_ENS_SPIN_LIMIT")
    assert getattr(s, "stream_fallbacks", 0) == 1
    _lib.check(_lib.lib().alabi_ens_set_stream(s._ens, 1), "alabi_ens_set_stream")
    s.run_mcmc(None, 150)
    assert s.last_path == "stream" and s.last_stream_variant == "single"
    _assert_same(_result(s), _result(ref), "after a time-out")


def test_two_ensembles(setup, monkeypatch):
    """Two ensembles of 16 walkers: each is placed by itself (its own walker ids, its own lists)."""
    s = _run_three(setup, monkeypatch, 16, [NSTEPS], n_ensembles=2)
    on, n_pref, n_hit = _stats(s)
    place, packed, _ = _export(s, 0, CHUNK, 32)
    tot = [0, 0]
    for e in range(2):
        sl = slice(16 * e, 16 * e + 16)
        order = (packed[:, sl, 0] & np.uint64(0xffffffff)).astype(np.int64) - 16 * e
        cw = (packed[:, sl, 0] >> np.uint64(32)).astype(np.int64) - 16 * e
        m_place, a, b = place_chunk(order, cw)
        assert np.array_equal(place[:, sl], m_place), e
        tot[0] += a; tot[1] += b
    assert on == 1 and 0 < tot[1] <= tot[0] < n_pref
