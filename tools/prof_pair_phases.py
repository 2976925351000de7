"""Phase breakdown of the pair variant of the persistent ensemble kernel (ens_pair_kernel): real-time stamps of the hand-off waves of
both workgroups of one pair, the verdict poll of the speculative items, the publish -> detect times of the proposal array and
of the verdict, and the items whose inputs the fetch-ahead of the previous item had complete, so that the input poll was skipped
(needs a build with -DALABI_PAIR_PROF: see tools/README.md).  "detected" is the stamp behind the input poll: for an item whose
inputs were fetched ahead it is the top of the item, not the arrival of the words.
Every build: the looks of the verdict poll and of the input poll (alabi_ens_pair_stats3), for all pairs.  PROF_CONFIG selects
C1, C2 or C3 (default), PROF_N the size of the training set."""
import ctypes, sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from alabi_amd import EnsembleSampler, HipGP, _lib
from alabi_amd.workloads import make_config
name = os.environ.get("PROF_CONFIG", "C3")
cfg = make_config(name, N=int(os.environ["PROF_N"]) if "PROF_N" in os.environ else None)
h = cfg["hyper"]
gp = HipGP(cfg["d"], h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"]); gp.compute(cfg["X"])
s = EnsembleSampler(cfg["W"], cfg["d"], gp, cfg["y"], cfg["bounds"], seed=1)
s.run_mcmc(cfg["p0"], 1024); torch.cuda.synchronize()
looks = (ctypes.c_longlong * 20)()
_lib.check(_lib.lib().alabi_ens_pair_stats3(s._ens, looks, 1), "alabi_ens_pair_stats3")     # counting on, from the next run
t0 = time.perf_counter(); s.run_mcmc(None, 1024); torch.cuda.synchronize(); dt = time.perf_counter() - t0
L = _lib.lib()
_lib.check(L.alabi_ens_pair_stats3(s._ens, looks, 0), "alabi_ens_pair_stats3")
print(name, "path", s.last_path, "variant", s.last_stream_variant, "wall us/half-step (counting on)", 1e6 * dt / 2048)
for role, base in (("R (assumes rejected)", 0), ("A (assumes accepted)", 10)):
    for poll, q in (("verdict poll, class-1 items", looks[base:base + 5]), ("input poll, items not fetched complete", looks[base + 5:base + 10])):
        n = max(q[0], 1)
        print(f"  {role:22s} {poll:40s} polls {q[0]:8d}  looks {q[1]:8d} ({q[1] / n:5.2f} per poll)  decided at look 1: {q[2]:8d} "
              f"({100.0 * q[2] / n:5.1f}%)  look 2: {q[3]:8d} ({100.0 * q[3] / n:5.1f}%)  look >= 3: {q[4]:8d} ({100.0 * q[4] / n:5.1f}%)")
if not hasattr(L, "alabi_debug_pair_prof"):
    sys.exit(0)                                      # not a -DALABI_PAIR_PROF build: no stamps
out = (ctypes.c_longlong * 26)()
L.alabi_debug_pair_prof.argtypes = [ctypes.POINTER(ctypes.c_longlong)]
print("rc", L.alabi_debug_pair_prof(out), "path", s.last_path, "variant", s.last_stream_variant, "wall us/half-step", 1e6 * dt / 2048)
v = list(out)
names = ["input poll wait (hand-off wave)", "rows detected -> barrier A", "barrier A -> barrier B (verdict poll included)",
         "barrier B -> row store issued"]
for role, base in (("R (assumes rejected)", 0), ("A (assumes accepted)", 8)):
    r = v[base:base + 8]
    n = max(r[4], 1)
    tick_ns = 1e9 * dt / max(r[5], 1)                # calibrated against the call's wall time (nominal 10 ns)
    tot = sum(r[:4])
    print(role)
    for nm, x in zip(names, r[:4]):
        print(f"  {nm:46s} {x / n:9.2f} ticks/item {x / n * tick_ns:9.1f} ns  {100.0 * x / max(tot, 1):5.1f}%")
    print(f"  verdict poll, per class-1 item {r[6] / max(r[7], 1) * tick_ns:9.1f} ns  ({r[7]} of {r[4]} items)")
    q = v[16 + (4 if base else 0):][:4]
    print(f"  prop publish -> detected by this reader    {q[0] / max(q[1], 1) * tick_ns:9.1f} ns  (n = {q[1]})")
    print(f"  row store -> verdict detected by this reader {q[2] / max(q[3], 1) * tick_ns:9.1f} ns  (n = {q[3]})")
    print(f"  inputs complete at first look (fetched ahead)  {v[24 + (1 if base else 0)]} of {r[4]} items")
    print("  items", r[4], "ticks total", r[5], "=> tick ns", tick_ns)
