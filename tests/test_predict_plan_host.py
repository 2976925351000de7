"""Which kernel a predict request runs and with what grid, pinned on the host: the integers of the debug hook
alabi_debug_predict_plan (predict_plan.hip) against a Python restatement of the launchers' formulas as they stood before the plan
was moved out of gp_predict.hip / api.hip (written from that source: launch_predict_mean, want_winv, launch_predict_var,
alabi_gp_predict), anchored by rows derived by hand for 256 CUs.  No GPU needed.

Layout of the hook's 30 integers: [0, 6) mean (route 0 rowwise / 1 tile / 2 matrix cores, gridDim.x, parts, points per part, k-steps,
stride of the partial sums), [6] small-batch variance kernel, [7, 11) variance (route 1 product with L^-1 / 2 substitution /
3 first generation, TM, chunk in queries, first-generation grid), then (groups, nsplit, w2, parts, gx, grid_c) of the first chunk,
of the last chunk and of the first chunk when the cached L^-1 cannot be had, [29] L^-1 by recursive block inversion."""
import ctypes
import itertools
import os

import pytest

FLAGS = ["ALABI_PM_MFMA", "ALABI_PV_SMALL", "ALABI_PV_W", "ALABI_PV_W2", "ALABI_PV_LEGACY", "ALABI_WINV_DNC"]
CHUNK = "ALABI_PV_CHUNK_TILES"
SWITCHES = FLAGS + [CHUNK]
MS = [1, 16, 17, 64, 65, 128, 129, 300, 2047, 2048, 2085, 4096, 4097, 5000, 16384, 65536, 300000]
NS = [60, 192, 300, 2000, 2100, 5000]
DS = [1, 4, 10, 30, 31, 40]
CUS = [1, 64, 256, 304]
SINGLE = [{}] + [{k: v} for k in FLAGS for v in ("0", "1")] + [{CHUNK: "7"}, {CHUNK: "66"}]


# ---------------------------------------------------------------- the launchers' formulas, restated
def _first_is(env, name, ch):
    return env.get(name) is not None and env[name][:1] == ch


def _atoll(s):
    s = s.lstrip(" \t\n\v\f\r")
    sign, i = 1, 0
    if s[:1] in ("+", "-"):
        sign, i = (-1 if s[0] == "-" else 1), 1
    j = i
    while j < len(s) and s[j].isdigit():
        j += 1
    return sign * int(s[i:j]) if j > i else 0


def _nsplit(tiles, Npad, n_cu):
    if not tiles < 2 * n_cu:
        return 1
    return max(1, min(2 * n_cu // tiles, (Npad + 255) // 256, 8))


def _mean(M, Npad, d, n_cu, env):
    if M >= 2048 and d + 2 <= 32 and not _first_is(env, "ALABI_PM_MFMA", "0"):
        ks, wgs = (d + 2 + 3) // 4, (M + 255) // 256
        parts, pts = 1, Npad
        if wgs < 3 * n_cu:
            parts = (3 * n_cu + wgs - 1) // wgs
            tiles16 = Npad // 16
            parts = max(1, min(parts, tiles16 // 4))
            pts = (tiles16 + parts - 1) // parts * 16
            parts = (Npad + pts - 1) // pts
        return [2, wgs, parts, pts, ks, wgs * 256]
    if M <= 4096:
        return [0, M, 1, 0, 0, 0]
    tiles = (M + 63) // 64
    return [1, tiles, _nsplit(tiles, Npad, n_cu), 0, 0, tiles * 64]


def _chunk(mc, Npad, n_cu, use_w, TM, env):
    groups = (mc + 63) // 64
    if not use_w:
        return [groups, 1, 0, 1, 0, min((mc + TM - 1) // TM, n_cu)]
    w2 = groups >= 32 and not _first_is(env, "ALABI_PV_W2", "0")
    wgs = (groups + 1) // 2 if w2 else groups
    parts = max(1, min(n_cu // wgs, Npad // 64)) if wgs < n_cu else 1
    return [groups, _nsplit(groups, Npad, n_cu), int(w2), parts, min(wgs, n_cu), 0]


def _var(M, Npad, d, n_cu, env):
    small = M <= (128 if Npad <= 2048 else 64) and Npad >= 256 and d <= 32 and not _first_is(env, "ALABI_PV_SMALL", "0")
    if not (d <= 32 and not _first_is(env, "ALABI_PV_LEGACY", "1")):      # dim_bucket(d) <= 32 is d <= 32
        return [int(small), 3, 0, 0, min((M + 63) // 64, 512)] + [0] * 18
    TM = 16 if M <= 16 * n_cu else 64
    chunk_tiles = (2 << 30) // (Npad * 64 * 8)
    chunk_tiles = max(chunk_tiles // (2 * n_cu) * (2 * n_cu), 2 * n_cu)
    if env.get(CHUNK) is not None and _atoll(env[CHUNK]) > 0:
        chunk_tiles = _atoll(env[CHUNK])
    chunk = chunk_tiles * 64
    if chunk > M:
        chunk = (M + 63) // 64 * 64
    use_w = not _first_is(env, "ALABI_PV_W", "0")
    first, last = min(M, chunk), M - (M - 1) // chunk * chunk
    return ([int(small), 1 if use_w else 2, TM, chunk, 0] + _chunk(first, Npad, n_cu, use_w, TM, env) +
            _chunk(last, Npad, n_cu, use_w, TM, env) + _chunk(first, Npad, n_cu, False, TM, env))


def restated(M, N, d, n_cu, env):
    Npad = (N + 63) // 64 * 64
    return _mean(M, Npad, d, n_cu, env) + _var(M, Npad, d, n_cu, env) + [int(not _first_is(env, "ALABI_WINV_DNC", "0"))]


# ---------------------------------------------------------------- the hook
@pytest.fixture(scope="module")
def hook():
    from alabi_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fn = lib.alabi_debug_predict_plan
    fn.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    buf = (ctypes.c_longlong * 30)()

    def plan(M, N, d, n_cu):
        assert fn(M, N, d, n_cu, buf, 30) == 30
        return list(buf)
    return plan


@pytest.fixture
def setenv():
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}

    def use(env):
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
    yield use
    for k in SWITCHES:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


MEAN = ("route", "gx", "parts", "pts", "ks", "mu_stride")
VAR = ("small", "route", "TM", "chunk", "grid")
CH = ("groups", "nsplit", "w2", "parts", "gx", "grid_c")


def _named(r):
    out = {"mean_" + k: v for k, v in zip(MEAN, r[0:6])}
    out.update(zip(VAR, r[6:11]))
    out.update({"c0_" + k: v for k, v in zip(CH, r[11:17])})
    out.update({"nw_" + k: v for k, v in zip(CH, r[23:29])})
    return out


# (environment, M, N, d) -> named integers, derived by hand from the launchers for n_cu = 256
HAND = [
    ({}, 2048, 2048, 4, dict(mean_route=2, mean_gx=8, mean_parts=32, mean_pts=64, mean_ks=2)),     # ceil(768 / 8) = 96 -> 128 / 4 = 32 parts of 64
    ({}, 2048, 300, 4, dict(mean_route=2, mean_parts=5, mean_pts=64)),                             # Npad = 320: 20 tiles of 16 -> 5 parts
    ({}, 300000, 300, 4, dict(mean_route=2, mean_gx=1172, mean_parts=1, mean_pts=320)),            # 1172 workgroups >= 3 x 256
    ({"ALABI_PM_MFMA": "0"}, 5000, 300, 4, dict(mean_route=1, mean_gx=79, mean_parts=2, mean_mu_stride=79 * 64)),   # 512 / 79 = 6 -> 2 stages
    ({}, 100, 300, 4, dict(mean_route=0, mean_gx=100, mean_parts=1)),
    ({}, 300000, 2048, 4, dict(route=1, chunk=131072)),                                            # 2 GiB / (2048 x 512 B) = 2048 tiles
    ({CHUNK: "7"}, 300000, 2048, 4, dict(route=1, chunk=448)),
    ({}, 300, 300, 4, dict(small=0, route=1, c0_w2=0, c0_groups=5, c0_nsplit=2, c0_parts=5, c0_gx=5)),
    ({}, 2085, 300, 4, dict(small=0, route=1, c0_w2=1, c0_groups=33, c0_parts=5, c0_gx=17)),
    ({"ALABI_PV_W": "0"}, 300, 300, 4, dict(route=2, TM=16, c0_grid_c=19, c0_nsplit=1)),           # ceil(300 / 16) = 19 tiles < 256
    ({"ALABI_PV_W": "0"}, 5000, 300, 4, dict(route=2, TM=64, c0_grid_c=79)),
    ({}, 300, 300, 4, dict(nw_grid_c=19, nw_nsplit=1)),                                            # no room for L^-1: the substitution's grid
    ({"ALABI_PV_LEGACY": "1"}, 300, 300, 4, dict(route=3, grid=5)),
    ({}, 65536, 300, 40, dict(route=3, grid=512, small=0)),
    ({}, 100, 300, 4, dict(small=1)),
    ({}, 1, 300, 4, dict(small=1)),
    ({}, 100, 192, 4, dict(small=0)),                                                              # Npad = 192 < 256
    ({}, 128, 2048, 4, dict(small=1)),
    ({}, 129, 2048, 4, dict(small=0)),
    ({}, 64, 2100, 4, dict(small=1)),
    ({}, 65, 2100, 4, dict(small=0)),                                                              # Npad = 2112 > 2048: at most 64
    ({"ALABI_PV_SMALL": "0"}, 100, 300, 4, dict(small=0)),
]


@pytest.mark.parametrize("row", range(len(HAND)))
def test_hand_derived_rows(hook, setenv, row):
    env, M, N, d, want = HAND[row]
    setenv(env)
    got, re = _named(hook(M, N, d, 256)), _named(restated(M, N, d, 256, env))
    print(env, M, N, d, {k: got[k] for k in want})
    assert {k: got[k] for k in want} == want
    assert {k: re[k] for k in want} == want            # the restatement cannot drift together with the C++


@pytest.mark.parametrize("env", SINGLE, ids=lambda e: " ".join("%s=%s" % kv for kv in e.items()) or "unset")
def test_sweep_equals_the_restated_launchers(hook, setenv, env):
    setenv(env)
    for M, N, d, n_cu in itertools.product(MS, NS, DS, CUS):
        assert hook(M, N, d, n_cu) == restated(M, N, d, n_cu, env), (M, N, d, n_cu)


@pytest.mark.parametrize("name", SWITCHES)
def test_switch_reading(hook, setenv, name):
    """every value the tests and tools use, and junk: junk never changes a default the launchers kept"""
    points = list(itertools.product((1, 100, 300, 2085, 5000, 300000), (300, 2100), (4, 40), (256,)))
    setenv({})
    default = [hook(*p) for p in points]
    for value in ("0", "1", "7", "66", "", "x", "-3"):
        env = {name: value}
        setenv(env)
        got = [hook(*p) for p in points]
        assert got == [restated(*p, env) for p in points], value
        if value in ("", "x", "-3") or (name in FLAGS and value in ("7", "66")) or (name == CHUNK and value == "0"):
            assert got == default, value
