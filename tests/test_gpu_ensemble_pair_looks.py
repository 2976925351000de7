"""Look counters of the pair kernel's hand-off wave (ens_pair_kernel; alabi_ens_pair_stats3 counts the looks of the verdict poll
and of the input poll): with the counting code in the kernel the chain still equals one launch per half step byte for byte over
three chunks, the counters are consistent with the items the draws prescribe, and a time-out at W = 16 falls back."""
import ctypes as C

import numpy as np

from test_gpu_ensemble_pair_pipeline import (  # noqa: F401  (`problems` is the fixture of that file: one GP per shape)
    _assert_same, _compare, _host_class_counts, _result, _sampler, problems, pytestmark)


def test_three_chunks_headline_dimension(problems, monkeypatch):
    """3000 steps at W = 16, d = 10: 47 000 class-1 verdict polls, two chunk boundaries."""
    _compare(problems(10), monkeypatch, 16, 10, nsteps=3000)


def test_look_counters(problems, monkeypatch):
    """alabi_ens_pair_stats3: both workgroups of a pair poll the verdict of every class-1 item; every poll has at least one
    look and falls into exactly one bin; the input-poll counters cover only items that loaded, so at most every item."""
    from alabi_amd import _lib
    W, d, nsteps = 16, 3, 200
    s = _sampler(problems(d), monkeypatch, "1", W, d)
    s._ensure_ens()
    out = (C.c_longlong * 20)()
    _lib.check(_lib.lib().alabi_ens_pair_stats3(s._ens, out, 1), "alabi_ens_pair_stats3")    # switches counting on
    assert list(out) == [0] * 20
    s.run_mcmc(np.random.RandomState(2).uniform(-2, 2, (W, d)), nsteps)
    assert s.last_stream_variant == "pair" and getattr(s, "stream_fallbacks", 0) == 0
    _lib.check(_lib.lib().alabi_ens_pair_stats3(s._ens, out, 0), "alabi_ens_pair_stats3")    # enable = 0: read and clear
    got = np.array(list(out)).reshape(2, 2, 5)        # role x (verdict poll, input poll) x (items, looks, look 1, look 2, look >= 3)
    print(got)
    want = _host_class_counts(s, W, nsteps)
    for role in range(2):
        items, looks, b1, b2, b3 = got[role, 0].tolist()
        assert items == want[1] and min(want) > 0
        assert looks >= items and b1 + b2 + b3 == items
        assert looks >= b1 + 2 * b2 + 3 * b3
        items, looks, b1, b2, b3 = got[role, 1].tolist()
        assert 0 < items <= sum(want)
        assert looks >= items and b1 + b2 + b3 == items
    _lib.check(_lib.lib().alabi_ens_pair_stats3(s._ens, out, 0), "alabi_ens_pair_stats3")
    assert list(out) == [0] * 20                      # cleared by the read before; counting stays on
    s.run_mcmc(None, 10)
    _lib.check(_lib.lib().alabi_ens_pair_stats3(s._ens, out, 0), "alabi_ens_pair_stats3")
    assert out[0] > 0 and out[10] == out[0]


def test_time_out_at_sixteen_walkers(problems, monkeypatch):
    """W = 16, a spin limit of one look in the middle call: a poll gives up, the call
    falls back, and the three calls together equal the reference."""
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
    print("stream_fallbacks", getattr(s, "stream_fallbacks", 0), "path", s.last_path)
    assert getattr(s, "stream_fallbacks", 0) == 1
    _lib.check(_lib.lib().alabi_ens_set_stream(s._ens, 1), "alabi_ens_set_stream")
    s.run_mcmc(None, n)
    assert s.stream_fallbacks == 1
    _assert_same(_result(s), _result(ref), "after a time-out")
