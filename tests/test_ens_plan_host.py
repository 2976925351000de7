"""How an ensemble handle is laid out and which way alabi_ens_run takes, pinned on the host: the integers of the debug hook
alabi_debug_ens_plan (ens_plan.hip) against a Python restatement of the rules as they stood, spread over the launch files, before
they were gathered there, anchored by rows derived by hand for 256 CUs.  No GPU needed.

The restatement was written from that source, function by function:
  _create       ens_create (api.hip): ALABI_ENS_THREADS, ALABI_ENS_CHUNK, ALABI_ENS_STREAM
  _ppt          ens_stream_ppt (ens_stream.hip) with the table ens_stream_max_db (ens_stream.hpp)
  _group        group_plan and group_lds (ens_group.hip): ALABI_ENS_GROUP_G16
  _mh_chunk     ens_mh_chunk, mh_lds_bytes (ens_mh.hip): ALABI_ENS_MH, ALABI_ENS_MH_CHUNK
  _hmc_chunk    ens_hmc_chunk, hmc_lds_bytes, hmc_threads (ens_hmc.hip): ALABI_ENS_HMC_CHUNK
  _np           the multi-proposal rule of launch_ens_half_args (ensemble.hip): ALABI_ENS_MULTI
  _route        alabi_ens_run (api.hip) with its `crowded` rule, ALABI_ENS_GROUP, ALABI_ENS_GRAPH, ALABI_ENS_GRAPH_STEPS, and the
                eligibility rules of ens_pair_ready (ens_pair.hip: ALABI_ENS_PAIR) and ens_place_ready (ens_place.hip: ALABI_ENS_PLACE)
and the two meanings of ALABI_ENS_SPIN_LIMIT (ens_stream_args: v polls; launch_ens_group: v - 1) and ALABI_ENS_SHARD_GRAPH (run_sharded).

Layout of the hook's 27 integers: [0, 3) creation plan (threads, chunk_cap, stream_grid), [3] point pairs per lane of the persistent
kernels, [4, 13) group blocking (ok, Q, G, NG, RT, tpm, ltw, KS, LDS bytes), [13] MH chunk, [14] HMC chunk, [15, 17) proposals per
workgroup of the two half-step launches of a step, [17, 23) route (path, chunk, pair, place, graph, graph steps), [23] the path when
the group kernel's buffers cannot be had, [24, 26) spin limit of ens_stream_kernel / ens_pair_kernel and of ens_group_kernel, [26] graph replay of the sharded run.

The sweep: W x E x d x N x n_cu x kernel family is 12 800 shapes.  Unset, all of them run with the stretch table and every 7th with
each other table / handle variant; under each single switch value every 37th shape runs with every variant.  7 and 37 share no
factor with the length of any axis (10, 4, 10, 4, 4, 2), so a thinned walk still visits every value of every axis and, as the
index runs mixed-radix through the product, every pair of neighbouring values many times.  Junk values run on a short list."""
import ctypes
import itertools
import os

import pytest

P = "ALABI_ENS_"
FLAGS = ["STREAM", "GROUP", "GROUP_G16", "GRAPH", "MH", "MULTI", "PAIR", "PLACE", "SHARD_GRAPH"]
NUMBERS = ["THREADS", "GRAPH_STEPS", "SPIN_LIMIT", "CHUNK", "MH_CHUNK", "HMC_CHUNK"]
SWITCHES = [P + n for n in FLAGS + NUMBERS]
WS = [1, 2, 3, 16, 17, 255, 256, 257, 2048, 8192]
ES = [1, 2, 8, 300]
DS = [1, 14, 15, 24, 25, 30, 31, 61, 62, 64]
NS = [60, 2000, 2100, 5000]
CUS = [1, 64, 256, 304]
SHAPES = list(itertools.product(WS, ES, DS, NS, CUS, (0, 1)))
VALUES = {"STREAM": "01", "GROUP": "01", "GROUP_G16": "01", "GRAPH": "01", "MH": "01", "MULTI": "0124", "PAIR": "01", "PLACE": "01",
          "SHARD_GRAPH": "01", "THREADS": ["64", "128", "256", "512", "1024", "100"], "GRAPH_STEPS": ["1", "2", "256", "1024", "5000"],
          "SPIN_LIMIT": ["1", "1000"], "CHUNK": ["1", "2", "16", "100", "2000"], "MH_CHUNK": ["1", "50", "100000"],
          "HMC_CHUNK": ["1", "50", "100000"]}
SINGLE = [{P + n: v} for n in FLAGS + NUMBERS for v in VALUES[n]]

# handle variants beyond the shape: what the move table and the setters leave on the handle
STRETCH = dict(ymap=0, threads=0, stream_ok=1, mh_ok=1, has_de=0, all_gauss=0, all_hmc=0, factors=0, n_moves=0, lmax=1, has_stream=1)
VARIANTS = {
    "stretch": {},
    "de": dict(has_de=1, n_moves=2),
    "gauss": dict(has_de=1, all_gauss=1, factors=1, n_moves=1),
    "gauss8": dict(has_de=1, all_gauss=1, factors=1, n_moves=8),              # 8 d^2 doubles: over the LDS bound from d = 48 on
    "gauss_t1024": dict(has_de=1, all_gauss=1, factors=1, n_moves=1, threads=1024),
    "gauss_mh_off": dict(has_de=1, all_gauss=1, factors=1, n_moves=1, mh_ok=0),
    "hmc": dict(all_hmc=1, factors=1, n_moves=1, lmax=10),
    "hmc8": dict(all_hmc=1, factors=1, n_moves=8, lmax=64),                  # over the LDS bound at d = 64
    "ymap": dict(ymap=1),
    "stream_off": dict(stream_ok=0),
    "null_stream": dict(has_stream=0),
}


# ---------------------------------------------------------------- the rules, restated
def _flag(env, name):
    v = env.get(P + name)
    return None if v is None else v[:1]


def _atoi(s):
    s = s.lstrip(" \t\n\v\f\r")
    sign, i = 1, 0
    if s[:1] in ("+", "-"):
        sign, i = (-1 if s[0] == "-" else 1), 1
    j = i
    while j < len(s) and s[j].isdigit():
        j += 1
    return sign * int(s[i:j]) if j > i else 0


def _num(env, name):
    v = env.get(P + name)
    return None if v is None else _atoi(v)


def _bucket(d):
    for b in (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64):
        if d <= b:
            return b
    return -1


def _create(W, E, Npad, n_cu, env):
    threads = 256 if Npad // 2 <= 1024 else 512
    v = _num(env, "THREADS")
    if v in (64, 128, 256, 512, 1024):
        threads = v
    cap = min(max((4 << 20) // (W * E), 16), 1024)
    v = _num(env, "CHUNK")
    if v is not None and 2 <= v < cap:
        cap = v
    grid = 0
    if E <= n_cu and _flag(env, "STREAM") != "0":
        grid = min(n_cu // E, (W + 1) // 2)
    return [threads, cap, grid]


def _max_db(T, ppt, generic):
    if T == 512:
        return {1: 12 if generic else 16, 2: 6 if generic else 10}.get(ppt, 0)
    if T == 256:
        return {1: 16, 2: 12 if generic else 16, 3: 8 if generic else 12, 4: 6 if generic else 10}.get(ppt, 0)
    return 0


def _ppt(h):
    T, half, db = h["threads"], h["Npad"] // 2, _bucket(h["d"])
    if h["d"] > 61 or db < 0 or h["ymap"] != 0:
        return 0
    ppt = (half + T - 1) // T
    return ppt if db <= _max_db(T, ppt, h["generic"]) else 0


def _group_lds_words(KS, QPAD, lds_tiles):
    S = 16 * lds_tiles
    return 256 + S * KS * 4 + S + QPAD * KS * 4 + 8 * QPAD + 4 * QPAD * 6 + 2


def _group(h, n_cu, env):
    d, none = h["d"], [0] * 9
    if d + 2 > 32 or h["ymap"] != 0 or h["W"] < 2 or h["E"] > n_cu:
        return none
    KS, n0, tiles = (d + 2 + 3) // 4, (h["W"] + 1) // 2, h["Npad"] // 16
    wide = KS > 4
    for attempt in (0, 1):
        if attempt == 0 and _flag(env, "GROUP_G16") == "1":
            continue
        G = 16 if (wide and attempt == 1) else 8
        RT = 5 if attempt == 0 else 0
        ng_max = n_cu // h["E"] // G
        if ng_max < 1:
            continue
        Q = 1
        while Q < 8 and (n0 + 16 * Q - 1) // (16 * Q) > ng_max:
            Q *= 2
        if (n0 + 16 * Q - 1) // (16 * Q) > ng_max or (wide and Q > 4) or (not wide and RT > 0 and Q > 2):
            continue
        QP = 16 * Q
        tpm = (tiles + G - 1) // G
        tpw = (tpm + 7) // 8
        ltw = tpw - RT if tpw > RT else 0
        lds = _group_lds_words(KS, QP, 8 * ltw) * 8
        if lds <= 160 * 1024 - 512:
            return [1, Q, G, (n0 + QP - 1) // QP, RT, tpm, ltw, KS, lds]
    return none


def _mh_chunk(h, n_cu, env):
    mh_lds = h["n_moves"] * h["d"] * h["d"] * 8
    if not h["all_gauss"] or not h["factors"] or h["threads"] > 512 or _bucket(h["d"]) < 0 or mh_lds > 128 * 1024:
        return 0
    if _flag(env, "MH") == "0":
        return 0
    rounds = (h["W"] * h["E"] + 2 * n_cu - 1) // (2 * n_cu)
    tiles = ((h["Npad"] >> 1) + h["threads"] - 1) // h["threads"]
    chunk = max(min(100000 // (3 * rounds * max(tiles, 1)), 16384), 64)
    v = _num(env, "MH_CHUNK")
    return v if v is not None and 1 <= v < chunk else chunk


def _hmc_chunk(h, n_cu, env):
    hmc_lds = (h["n_moves"] * h["d"] * (h["d"] | 1) + h["Npad"]) * 8
    if not h["all_hmc"] or not h["factors"] or _bucket(h["d"]) < 0 or hmc_lds > 128 * 1024:
        return 0
    T = min(h["threads"], 512)
    rounds = (h["W"] * h["E"] + 2 * n_cu - 1) // (2 * n_cu)
    tiles = ((h["Npad"] >> 1) + T - 1) // T
    chunk = max(min(100000 // (9 * rounds * max(tiles, 1) * h["lmax"]), 16384), 16)
    v = _num(env, "HMC_CHUNK")
    return v if v is not None and 1 <= v < chunk else chunk


def _np(h, total, n_cu, env):
    db, m, np_ = _bucket(h["d"]), _flag(env, "MULTI"), 1
    if h["threads"] <= 512 and db <= 24 and m != "0":
        if total > 3 * n_cu and db <= 16:
            np_ = 4
        elif total > n_cu:
            np_ = 2
        if m == "4" and db <= 16:
            np_ = 4
        if m == "2":
            np_ = 2
        if m == "1":
            np_ = 1
    return np_


def _route(h, n_cu, env, buffers=True):
    if h["all_hmc"]:
        chunk = _hmc_chunk(h, n_cu, env)
        return [5 if chunk > 0 else -1, chunk, 0, 0, 0, 0]
    if h["W"] < 2 and not h["all_gauss"]:
        return [-1, 0, 0, 0, 0, 0]
    if h["all_gauss"] and h["mh_ok"]:
        chunk = _mh_chunk(h, n_cu, env)
        if chunk > 0:
            return [4, chunk, 0, 0, 0, 0]
    g = _flag(env, "GROUP")
    can_stream = _ppt(h) > 0
    n0, grid = (h["W"] + 1) // 2, h["stream_grid"]
    crowded = can_stream and grid > 0 and (n0 + grid - 1) // grid >= 4
    use_group = bool(not h["has_de"] and h["stream_ok"] and h["has_stream"] and g != "0" and (g == "1" or not can_stream or crowded) and
                     h["has_hist"] and _group(h, n_cu, env)[0] and buffers)
    if not h["has_de"] and h["stream_ok"] and h["has_stream"] and (can_stream or use_group):
        if use_group:
            return [3, 0, 0, 0, 0, 0]
        pair = _flag(env, "PAIR") != "0" and h["d"] >= 1 and 2 * n0 * h["E"] <= n_cu
        place = _flag(env, "PLACE") != "0" and h["W"] == 2 * n0 and n0 % 8 == 0 and n0 <= 128
        return [1, 0, int(pair), int(place), 0, 0]
    gsteps = min(h["chunk_cap"], 256)
    v = _num(env, "GRAPH_STEPS")
    if v is not None and 0 < v <= h["chunk_cap"]:
        gsteps = v
    return [0, 0, 0, 0, int(bool(h["has_stream"]) and _flag(env, "GRAPH") != "0"), gsteps]


def _handle(shape, variant):
    W, E, d, N, _, generic = shape
    h = dict(STRETCH, W=W, E=E, d=d, Npad=(N + 63) // 64 * 64, generic=generic)
    h.update(VARIANTS[variant])
    return h


def restated(shape, variant, env):
    h, n_cu = _handle(shape, variant), shape[4]
    c = _create(h["W"], h["E"], h["Npad"], n_cu, env)
    if h["threads"] <= 0:
        h["threads"] = c[0]
    h["chunk_cap"], h["stream_grid"] = c[1], c[2]
    h["has_hist"] = int(c[2] > 0)
    h["stream_ok"] = int(h["stream_ok"] and h["has_hist"])
    n0 = (h["W"] + 1) // 2
    spin = _num(env, "SPIN_LIMIT")
    spin = spin if spin is not None and spin > 0 else 0
    return (c + [_ppt(h)] + _group(h, n_cu, env) + [_mh_chunk(h, n_cu, env), _hmc_chunk(h, n_cu, env),
            _np(h, n0 * h["E"], n_cu, env), _np(h, (h["W"] - n0) * h["E"], n_cu, env)] + _route(h, n_cu, env) +
            [_route(h, n_cu, env, buffers=False)[0], spin or 1 << 20, spin - 1 if spin else 1 << 20, int(_flag(env, "SHARD_GRAPH") == "1")])


# ---------------------------------------------------------------- the hook
FIELDS = ("W", "E", "d", "Npad", "generic", "ymap", "threads", "chunk_cap", "stream_grid", "has_hist", "stream_ok", "mh_ok", "has_de",
          "all_gauss", "all_hmc", "factors", "n_moves", "lmax", "mh_lds", "hmc_lds", "has_stream")


@pytest.fixture(scope="module")
def hook():
    from alabi_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fn = lib.alabi_debug_ens_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    buf = (ctypes.c_longlong * 27)()
    arr = (ctypes.c_int * len(FIELDS))()

    def plan(shape, variant):
        h = _handle(shape, variant)
        h.update(chunk_cap=0, stream_grid=0, has_hist=0, mh_lds=h["n_moves"] * h["d"] * h["d"] * 8,
                 hmc_lds=(h["n_moves"] * h["d"] * (h["d"] | 1) + h["Npad"]) * 8)
        arr[:] = [h[k] for k in FIELDS]
        assert fn(arr, len(FIELDS), shape[4], buf, 27) == 27
        return list(buf)
    plan.raw = fn
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


NAMES = ("threads", "chunk_cap", "stream_grid", "ppt", "g_ok", "Q", "G", "NG", "RT", "tpm", "ltw", "KS", "lds", "mh_chunk", "hmc_chunk",
         "np0", "np1", "path", "chunk", "pair", "place", "graph", "gsteps", "path_nobuf", "spin", "spin_group", "shard_graph")


def _named(r):
    return dict(zip(NAMES, r))


HEAD = (256, 1, 10, 2000, 256, 0)        # the headline shape: W = 256, one ensemble, d = 10, N = 2000, 256 CUs, squared exponential


def _with(**kw):
    s = dict(zip(("W", "E", "d", "N", "n_cu", "generic"), HEAD))
    s.update(kw)
    return tuple(s[k] for k in ("W", "E", "d", "N", "n_cu", "generic"))


# (environment, shape, variant) -> named integers, derived by hand from the parent's rules for 256 CUs
HAND = [
    # Npad = 2048: 256 lanes x 4 pairs, bucket 10 <= 10 fits; grid min(256, 128); ceil(128 / 128) = 1 < 4: not crowded; 2 x 128 = 256 <= 256 CUs
    ({}, HEAD, "stretch", dict(threads=256, chunk_cap=1024, stream_grid=128, ppt=4, path=1, pair=1, place=1, np0=1)),
    ({}, _with(n_cu=255), "stretch", dict(path=1, pair=0, stream_grid=128)),                        # 256 workgroups > 255 CUs
    ({P + "PAIR": "0"}, HEAD, "stretch", dict(path=1, pair=0, place=1)),
    ({P + "PLACE": "0"}, HEAD, "stretch", dict(path=1, pair=1, place=0)),
    ({}, _with(W=254), "stretch", dict(path=1, pair=1, place=0)),                                   # n0 = 127: no whole classes
    # W = 2048: grid 256, ceil(1024 / 256) = 4: crowded.  KS = 3, 32 groups of 8 at most: Q = 2 (32 tiles of 32), 128 point tiles / 8 = 16
    # per member, 2 per wave < 5 in registers; LDS 256 + 384 + 256 + 768 + 2 words
    ({}, _with(W=2048), "stretch", dict(path=3, ppt=4, g_ok=1, Q=2, G=8, NG=32, RT=5, tpm=16, ltw=0, KS=3, lds=13328, path_nobuf=1, np0=4)),
    ({P + "GROUP": "0"}, _with(W=2048), "stretch", dict(path=1, pair=0)),
    ({}, _with(W=1536), "stretch", dict(path=1, stream_grid=256)),                                  # ceil(768 / 256) = 3: not crowded
    # N = 5000: Npad = 5056, 512 lanes x 5 pairs has no row: the group kernel.  316 tiles / 8 = 40 per member, 5 per wave, all in registers
    ({}, _with(N=5000), "stretch", dict(threads=512, ppt=0, path=3, Q=1, G=8, NG=8, RT=5, tpm=40, ltw=0, KS=3, lds=7696, path_nobuf=0)),
    ({P + "GROUP": "1"}, HEAD, "stretch", dict(path=3, Q=1, NG=8, tpm=16)),                         # preferred where feasible
    # d = 16: KS = 5, wide rows.  G8 with register tiles first; ALABI_ENS_GROUP_G16=1 skips it: 16 members, none in registers
    ({P + "GROUP": "1"}, _with(d=16), "stretch", dict(path=3, G=8, RT=5, KS=5)),
    ({P + "GROUP": "1", P + "GROUP_G16": "1"}, _with(d=16), "stretch", dict(path=3, G=16, RT=0, KS=5, tpm=8, ltw=1)),
    ({}, _with(d=31), "stretch", dict(ppt=0, g_ok=0, path=0, graph=1, gsteps=256, np0=1)),           # d + 2 = 33 > 32: no group; bucket 32 > 24
    ({}, HEAD, "ymap", dict(ppt=0, g_ok=0, path=0, graph=1)),
    ({}, HEAD, "de", dict(path=0, graph=1, gsteps=256, np0=1, np1=1)),                               # 128 proposals <= 256 CUs
    ({P + "GRAPH": "0"}, HEAD, "de", dict(path=0, graph=0)),
    ({P + "GRAPH_STEPS": "2"}, HEAD, "de", dict(path=0, graph=1, gsteps=2)),
    ({P + "GRAPH_STEPS": "1025"}, HEAD, "de", dict(gsteps=256)),                                     # beyond chunk_cap = 1024
    ({}, HEAD, "null_stream", dict(path=0, graph=0)),
    ({}, HEAD, "stream_off", dict(path=0, graph=1)),
    ({}, _with(W=1024), "de", dict(np0=2, np1=2)),                                                   # 512 proposals > 256 CUs
    ({}, _with(W=2048), "de", dict(np0=4)),                                                          # 1024 > 768, bucket 10 <= 16
    ({P + "MULTI": "0"}, _with(W=2048), "de", dict(np0=1)),
    # all-Gaussian: one round of 256 workgroups over 512 slots, 4 tiles of 256 pairs: 100000 / 12
    ({}, HEAD, "gauss", dict(path=4, chunk=8333, mh_chunk=8333)),
    ({}, HEAD, "gauss_t1024", dict(path=0, mh_chunk=0, graph=1)),                                    # ens_mh_kernel has no 1024-lane form
    ({}, HEAD, "gauss_mh_off", dict(path=0)),
    ({P + "MH": "0"}, HEAD, "gauss", dict(path=0, mh_chunk=0)),
    ({P + "MH_CHUNK": "50"}, HEAD, "gauss", dict(path=4, chunk=50)),
    ({}, _with(d=48), "gauss8", dict(path=0, mh_chunk=0)),                                           # 8 x 48 x 48 x 8 = 147456 > 131072 bytes
    ({}, _with(W=1), "gauss", dict(path=4)),
    ({}, _with(W=1), "stretch", dict(path=-1)),
    # HMC: 100000 / (9 x 1 round x 4 tiles x 10 leapfrog steps)
    ({}, HEAD, "hmc", dict(path=5, chunk=277, hmc_chunk=277)),
    ({}, _with(d=64), "hmc8", dict(path=-1, hmc_chunk=0)),                                           # (8 x 64 x 65 + 2048) x 8 bytes > 128 KB
    ({P + "HMC_CHUNK": "7"}, HEAD, "hmc", dict(path=5, chunk=7)),
    ({P + "STREAM": "0"}, HEAD, "stretch", dict(stream_grid=0, path=0)),
    ({P + "THREADS": "512"}, HEAD, "stretch", dict(threads=512, ppt=2, path=1)),                     # bucket 10 <= 10 at 512 x 2
    ({P + "CHUNK": "16"}, HEAD, "stretch", dict(chunk_cap=16)),
    ({}, _with(E=300), "stretch", dict(stream_grid=0, path=0)),                                      # more ensembles than CUs
    ({P + "SPIN_LIMIT": "1"}, HEAD, "stretch", dict(spin=1, spin_group=0)),                          # group kernel: the first miss
    ({}, HEAD, "stretch", dict(spin=1 << 20, spin_group=1 << 20)),
    ({P + "SHARD_GRAPH": "1"}, HEAD, "stretch", dict(shard_graph=1)),
]


@pytest.mark.parametrize("row", range(len(HAND)))
def test_hand_derived_rows(hook, setenv, row):
    env, shape, variant, want = HAND[row]
    setenv(env)
    got, re = _named(hook(shape, variant)), _named(restated(shape, variant, env))
    print(env, shape, variant, {k: got[k] for k in want})
    assert {k: got[k] for k in want} == want
    assert {k: re[k] for k in want} == want            # the restatement cannot drift together with the C++


def test_sweep_unset(hook, setenv):
    setenv({})
    for i, shape in enumerate(SHAPES):
        for variant in (VARIANTS if i % 7 == 0 else ("stretch",)):
            assert hook(shape, variant) == restated(shape, variant, {}), (shape, variant)


@pytest.mark.parametrize("env", SINGLE, ids=lambda e: " ".join("%s=%s" % kv for kv in e.items()))
def test_sweep_under_one_switch(hook, setenv, env):
    setenv(env)
    for shape in SHAPES[::37]:
        for variant in VARIANTS:
            assert hook(shape, variant) == restated(shape, variant, env), (shape, variant)


@pytest.mark.parametrize("name", FLAGS + NUMBERS)
def test_switch_reading(hook, setenv, name):
    """junk never changes what an unset switch gives; a flag looks at its first character only"""
    points = [(s, v) for s in (HEAD, _with(W=2048), _with(N=5000), _with(d=16), _with(W=17, E=8, n_cu=64, generic=1)) for v in VARIANTS]
    setenv({})
    default = [hook(*p) for p in points]
    for value in ("", "x", "-3", "99999999", "0x", "1x"):
        env = {P + name: value}
        setenv(env)
        got = [hook(*p) for p in points]
        assert got == [restated(*p, env) for p in points], value
        if value in ("", "x", "-3") or (name in FLAGS and value == "99999999"):
            assert got == default, value


def test_short_and_null_buffers(hook, setenv):
    setenv({})
    arr = (ctypes.c_int * 4)(256, 1, 10, 2048)
    two = (ctypes.c_longlong * 2)(-1, -1)
    assert hook.raw(arr, 4, 256, two, 1) == 27 and two[1] == -1 and two[0] == 256
    assert hook.raw(arr, 4, 256, None, 0) == 27
    assert hook.raw(None, 0, 256, two, 2) == 0 and two[1] == -1            # no shape: nothing to plan
