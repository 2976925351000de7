"""The plan of an all-NUTS move table (alabi_amd/csrc/ens_plan.hip: ens_nuts_chunk, the path-6 route, ALABI_ENS_NUTS_CHUNK) through
the host-only hook alabi_debug_ens_plan, against the rule restated here.  No GPU."""
import ctypes
import os

import pytest

FIELDS = ("W", "E", "d", "Npad", "generic", "ymap", "threads", "chunk_cap", "stream_grid", "has_hist", "stream_ok", "mh_ok", "has_de",
          "all_gauss", "all_hmc", "factors", "n_moves", "lmax", "mh_lds", "hmc_lds", "has_stream", "all_nuts", "nuts_lds")
PATH, CHUNK, HMC_CHUNK = 17, 18, 14
VAR = "ALABI_ENS_NUTS_CHUNK"


@pytest.fixture(scope="module")
def plan():
    from alabi_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    fn = ctypes.CDLL(_lib.LIB_PATH).alabi_debug_ens_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    buf = (ctypes.c_longlong * 27)()

    def call(n_cu=256, **kw):
        h = dict.fromkeys(FIELDS, 0)
        h.update(W=256, E=1, d=10, Npad=2048, stream_ok=1, mh_ok=1, has_stream=1, all_nuts=1, factors=1, n_moves=1, lmax=8)
        h.update(kw)
        h["mh_lds"] = h["n_moves"] * h["d"] * h["d"] * 8
        h["hmc_lds"] = (h["n_moves"] * h["d"] * (h["d"] | 1) + h["Npad"]) * 8
        h["nuts_lds"] = h["hmc_lds"] + 2 * 10 * 64 * 8
        arr = (ctypes.c_int * len(FIELDS))(*[h[k] for k in FIELDS])
        assert fn(arr, len(FIELDS), n_cu, buf, 27) == 27
        return list(buf)
    return call


@pytest.fixture
def env():
    saved = os.environ.pop(VAR, None)
    yield os.environ
    os.environ.pop(VAR, None)
    if saved is not None:
        os.environ[VAR] = saved


def _rule(W, E, Npad, depth, n_cu, threads=256, cap=0):
    """ens_hmc_chunk's estimate with 2^depth - 1 leaves in place of n_leapfrog, between 4 and 16384."""
    T = min(threads, 512)
    rounds = (W * E + 2 * n_cu - 1) // (2 * n_cu)
    tiles = max(((Npad >> 1) + T - 1) // T, 1)
    chunk = min(max(100000 // (9 * rounds * tiles * ((1 << depth) - 1)), 4), 16384)
    return cap if 1 <= cap < chunk else chunk


@pytest.mark.parametrize("depth", [1, 3, 8, 10])
@pytest.mark.parametrize("W,E,n_cu", [(256, 1, 256), (1, 1, 256), (1024, 3, 256), (8192, 300, 64)])
def test_the_chunk_rule_and_the_route(plan, env, depth, W, E, n_cu):
    r = plan(n_cu=n_cu, W=W, E=E, lmax=depth)
    assert r[PATH] == 6 and r[CHUNK] == _rule(W, E, 2048, depth, n_cu) and r[HMC_CHUNK] == 0
    assert 4 <= r[CHUNK] <= 16384


def test_known_values(plan, env):
    assert plan(lmax=8)[CHUNK] == 100000 // (9 * 4 * 255) == 10          # the headline shape, max_depth 8
    assert plan(lmax=10)[CHUNK] == 4                                      # the lower limit
    assert plan(lmax=1, Npad=64)[CHUNK] == 11111


def test_the_switch_caps_the_chunk_and_nothing_else(plan, env):
    env[VAR] = "3"
    assert plan(lmax=8)[CHUNK] == 3 and plan(lmax=8)[PATH] == 6
    env[VAR] = "1000"
    assert plan(lmax=8)[CHUNK] == 10
    for bad in ("0", "-3", "x", ""):
        env[VAR] = bad
        assert plan(lmax=8)[CHUNK] == 10
    env[VAR] = "3"
    hmc = plan(all_nuts=0, all_hmc=1)                                     # nor does the NUTS switch reach an HMC table
    assert hmc[PATH] == 5 and hmc[CHUNK] == hmc[HMC_CHUNK] == 100000 // (9 * 4 * 8)
    os.environ["ALABI_ENS_HMC_CHUNK"] = "2"
    try:
        assert plan(lmax=8)[CHUNK] == 3                                   # the HMC switch does not reach a NUTS table
    finally:
        os.environ.pop("ALABI_ENS_HMC_CHUNK")


def test_refusals(plan, env):
    assert plan(factors=0)[PATH] == -1                                    # no factor on the device
    assert plan(d=64, n_moves=5, Npad=192)[PATH] == -1                    # five full factors at d = 64: 162 KB
    assert plan(d=64, n_moves=3, Npad=192)[PATH] == 6
    # the checkpoints count: factors and weights alone would fit 128 KB, with the 10 KB of checkpoints they do not
    npad = (128 * 1024 - 3 * 64 * 65 * 8) // 8 - 64
    assert (3 * 64 * 65 + npad) * 8 <= 128 * 1024 < (3 * 64 * 65 + npad + 1280) * 8
    assert plan(d=64, n_moves=3, Npad=npad)[PATH] == -1
    assert plan(lmax=11)[PATH] == -1 and plan(lmax=0)[PATH] == -1         # a depth the kernel's checkpoints do not hold
    assert plan(W=1)[PATH] == 6                                           # one walker is a chain
    assert plan(stream_ok=0, mh_ok=0)[PATH] == 6                          # alabi_ens_set_stream does not move it
