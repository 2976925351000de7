"""What the plan says is what runs: one small handle per route of alabi_ens_run (N = 64, d = 2, 16 walkers, 4 steps; d = 16 for
the group kernel's wide rows).  After the run the integers of alabi_debug_ens_plan (ens_plan.hip) for the handle's shape, under the
same environment, equal what the launchers recorded on the handle: alabi_ens_last_path, alabi_ens_stream_variant,
alabi_ens_place_stats[0], alabi_ens_group_plan, alabi_ens_mh_plan[1] and alabi_ens_hmc_plan[1].  The route each case is meant to
reach is asserted as well, so the two cannot agree on a wrong one.  tests/test_ens_plan_host.py pins the plan's integers."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu

N, W, STEPS = 64, 16, 4
P = "ALABI_ENS_"
HOOK = ("threads", "chunk_cap", "stream_grid", "ppt", "g_ok", "Q", "G", "NG", "RT", "tpm", "ltw", "KS", "lds", "mh_chunk", "hmc_chunk",
        "np0", "np1", "path", "chunk", "pair", "place", "graph", "gsteps", "path_nobuf", "spin", "spin_group", "shard_graph")

# name -> (d, environment, moves, handle flags of the shape beyond the stretch table, what the case is meant to reach)
ROUTES = {
    "half": (2, {"STREAM": "0", "GRAPH": "0"}, None, {}, dict(path=0, graph=0)),
    "half_graph": (2, {"STREAM": "0", "GRAPH_STEPS": "2"}, None, {}, dict(path=0, graph=1, gsteps=2)),
    "stream": (2, {"PAIR": "0"}, None, {}, dict(path=1, pair=0)),
    "pair": (2, {"PLACE": "0"}, None, {}, dict(path=1, pair=1, place=0)),
    "pair_place": (2, {}, None, {}, dict(path=1, pair=1, place=1)),
    "group": (2, {"GROUP": "1"}, None, {}, dict(path=3, G=8, RT=5, KS=1)),
    "group_wide_g8": (16, {"GROUP": "1"}, None, {}, dict(path=3, G=8, RT=5, KS=5)),
    "group_wide_g16": (16, {"GROUP": "1", "GROUP_G16": "1"}, None, {}, dict(path=3, G=16, RT=0, KS=5)),
    "mh": (2, {}, "gauss", dict(has_de=1, all_gauss=1, factors=1, n_moves=1), dict(path=4)),
    "hmc": (2, {}, "hmc", dict(all_hmc=1, factors=1, n_moves=1, lmax=3), dict(path=5)),
}
FIELDS = ("W", "E", "d", "Npad", "generic", "ymap", "threads", "chunk_cap", "stream_grid", "has_hist", "stream_ok", "mh_ok", "has_de",
          "all_gauss", "all_hmc", "factors", "n_moves", "lmax", "mh_lds", "hmc_lds", "has_stream")


@pytest.fixture(scope="module")
def gps():
    import torch
    from alabi_amd import HipGP
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    out = {}
    for d in (2, 16):
        X, y, h = make_problem(N, d, 30 + d, log_wn=-9.0, ell2=2.0 * d)
        g = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"]); g.compute(X)
        out[d] = (g, y)
    return out


def _hook(d, flags):
    from alabi_amd import _lib
    lib = _lib.lib()
    n_cu = C.c_int(0)
    _lib.check(lib.alabi_device_info(C.byref(n_cu), None, None), "alabi_device_info")
    Npad = (N + 63) // 64 * 64
    h = dict(W=W, E=1, d=d, Npad=Npad, generic=0, ymap=0, threads=0, chunk_cap=0, stream_grid=0, has_hist=0, stream_ok=1, mh_ok=1,
             has_de=0, all_gauss=0, all_hmc=0, factors=0, n_moves=0, lmax=1, has_stream=1)
    h.update(flags)
    h.update(mh_lds=h["n_moves"] * d * d * 8, hmc_lds=(h["n_moves"] * d * (d | 1) + Npad) * 8)
    fn = lib.alabi_debug_ens_plan
    fn.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int]
    fn.restype = C.c_int
    out = (C.c_longlong * len(HOOK))()
    assert fn((C.c_int * len(FIELDS))(*[h[k] for k in FIELDS]), len(FIELDS), n_cu.value, out, len(HOOK)) == len(HOOK)
    return dict(zip(HOOK, (int(v) for v in out)))


def _ints(s, call, n, ctype=C.c_int):
    from alabi_amd import _lib
    out = (ctype * n)()
    args = (s._ens, out, 0) if call == "alabi_ens_place_stats" else (s._ens, out)
    _lib.check(getattr(_lib.lib(), call)(*args), call)
    return [int(v) for v in out]


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_plan_is_what_runs(gps, monkeypatch, route):
    from alabi_amd import EnsembleSampler, _lib
    from alabi_amd.moves import GaussianMove, HMCMove
    d, env, moves, flags, meant = ROUTES[route]
    for k in ("STREAM", "GROUP", "GROUP_G16", "GRAPH", "GRAPH_STEPS", "MH", "MULTI", "PAIR", "PLACE", "THREADS", "CHUNK", "MH_CHUNK",
              "HMC_CHUNK", "SPIN_LIMIT"):
        monkeypatch.delenv(P + k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(P + k, v)                      # the same environment at creation, at the run and at the hook
    g, y = gps[d]
    mv = {None: None, "gauss": GaussianMove(0.05), "hmc": HMCMove(0.05 * np.eye(d), step_size=0.1, n_leapfrog=3)}[moves]
    s = EnsembleSampler(W, d, g, y, np.array([[-3.0, 3.0]] * d), seed=5, moves=mv, live_dangerously=True)
    # (16 walkers in 16 dimensions: the centred start has rank 15, which the route does not care about)
    s.run_mcmc(np.random.RandomState(3).uniform(-2, 2, (W, d)), STEPS, skip_initial_state_check=True)
    assert getattr(s, "stream_fallbacks", 0) == 0
    plan = _hook(d, flags)
    path = _ints(s, "alabi_ens_last_path", 1)[0]
    print(route, {k: plan[k] for k in ("path", "pair", "place", "graph", "gsteps", "chunk", "Q", "G", "NG", "RT", "tpm", "ltw", "KS", "lds")}, path)
    assert {k: plan[k] for k in meant} == meant
    assert path == plan["path"]
    assert _ints(s, "alabi_ens_stream_variant", 1)[0] == plan["pair"]          # both 0 off path 1
    if plan["path"] == 1 and plan["pair"]:
        assert _ints(s, "alabi_ens_place_stats", 3, C.c_longlong)[0] == plan["place"]
    if plan["path"] == 3:
        assert _ints(s, "alabi_ens_group_plan", 8) == [plan[k] for k in ("Q", "G", "NG", "RT", "tpm", "ltw", "KS", "lds")]
    if plan["path"] == 4:
        assert plan["chunk"] == plan["mh_chunk"] > 0 and _ints(s, "alabi_ens_mh_plan", 4)[1] == plan["mh_chunk"]
    if plan["path"] == 5:
        assert plan["chunk"] == plan["hmc_chunk"] > 0 and _ints(s, "alabi_ens_hmc_plan", 4)[1] == plan["hmc_chunk"]
    assert s.get_chain().shape == (STEPS, W, d) and np.all(np.isfinite(s.get_log_prob()))
