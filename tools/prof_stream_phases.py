"""Phase breakdown of the persistent ensemble kernel, real-time stamps of the hand-off wave of one workgroup (needs a build
with -DALABI_STREAM_PROF: see tools/README.md)."""
import ctypes, sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from alabi_amd import EnsembleSampler, HipGP, _lib
from alabi_amd.workloads import make_config
cfg = make_config("C3", N=int(os.environ.get("PROF_N", "2000")))
h = cfg["hyper"]
gp = HipGP(cfg["d"], h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"]); gp.compute(cfg["X"])
s = EnsembleSampler(cfg["W"], cfg["d"], gp, cfg["y"], cfg["bounds"], seed=1)
s.run_mcmc(cfg["p0"], 1024); torch.cuda.synchronize()
t0 = time.perf_counter(); s.run_mcmc(None, 1024); torch.cuda.synchronize(); dt = time.perf_counter() - t0
out = (ctypes.c_longlong * 16)()
L = _lib.lib()
L.alabi_debug_stream_prof.argtypes = [ctypes.POINTER(ctypes.c_longlong)]
print("rc", L.alabi_debug_stream_prof(out), "path", s.last_path, "wall us/half-step", 1e6 * dt / 2048)
v = list(out)[:6]
n = max(v[4], 1)
# stamps are wall_clock64() (the constant 100 MHz counter): the shader clock under-counts when two waves share a SIMD, and the
# hand-off wave does
names = ["poll wait (hand-off wave)", "rows detected -> barrier A", "barrier A -> barrier B (compute waves)", "barrier B -> row store issued"]
tot = sum(v[:4])
tick_ns = 1e9 * dt / max(v[5], 1)                    # calibrated against the call's wall time (nominal 10 ns)
for nm, x in zip(names, v[:4]):
    print(f"{nm:40s} {x / n:9.2f} ticks/item {x / n * tick_ns:9.1f} ns  {100.0 * x / tot:5.1f}%")
print("items", n, "ticks total", v[5], "ticks/item", v[5] / n, "=> tick ns", tick_ns)
