"""diagnostics.summary on a device chain: the default run_emcee chain (5e4 steps x 256 walkers x 10 parameters, 1 GB) and its
post-burn-in views, the time split into the sort / rank part (torch.sort, run lengths, ndtri) and alabi_chain_split_stats, next to
get_autocorr_time(tol=0)'s integrated_time on the same chain in the same process.  Host clock around work that ends in a device
synchronise; every shape is warmed once, then timed `--reps` times (all repetitions are printed: the spread is the noise).
python tools/prof_diagnostics.py [--steps 50000 --walkers 256 --dim 10 --reps 3 --out profiles/diagnostics.txt]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from alabi_amd import diagnostics
from alabi_amd.mcmc_utils import integrated_time

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50000); ap.add_argument("--walkers", type=int, default=256)
ap.add_argument("--dim", type=int, default=10); ap.add_argument("--reps", type=int, default=3); ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize()
    return r, time.perf_counter() - t0


torch.zeros(1, device="cuda"); torch.cuda.synchronize()
say("python tools/prof_diagnostics.py " + " ".join(sys.argv[1:]))
say(f"device: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); torch {torch.__version__}; "
    "times: host clock around a device synchronise, one process, every shape warmed once")
# per walker a 64-tap moving average with weights 0.9^j (an AR(1) with phi = 0.9 up to 0.9^64 = 1e-3), made on the device from a seed
g = torch.Generator(device="cuda"); g.manual_seed(1)
x = torch.randn((a.steps, a.walkers, a.dim), dtype=torch.float64, device="cuda", generator=g)
w =0.9 ** torch.arange(64, dtype=torch.float64, device="cuda")
y = torch.zeros_like(x)
for j in range(64):
    y[j:] += w[j] * x[:a.steps - j]
x = y; del y
say(f"chain [{a.steps}, {a.walkers}, {a.dim}] fp64, {x.numel() * 8 / 1e6:.0f} MB, moving average of 64 taps of 0.9^j (tau ~ 19)")
for name, view in (("whole chain", x), ("discard 5000", x[5000:]), ("discard 5000, thin 10", x[5000 + 9::10])):
    if view.shape[0] < 4:
        continue
    diagnostics.summary(view)                             # warm-up of every shape
    for rep in range(a.reps):
        s, total = timed(lambda: diagnostics.summary(view))
        tm = {}
        _, split_total = timed(lambda: diagnostics.summary(view, timings=tm))
        say(f"{name:24s} [{view.shape[0]} steps, step stride {view.stride(0)}] rep {rep}: summary {total * 1e3:8.1f} ms | with the split's "
            f"synchronises {split_total * 1e3:8.1f} ms = sort/rank {tm.get('sort_rank', 0) * 1e3:8.1f} + alabi_chain_split_stats "
            f"{tm.get('split_stats', 0) * 1e3:8.1f} + host (Geyer, copies) {(split_total - sum(tm.values())) * 1e3:7.1f}")
    say(f"{name:24s} rhat max {np.nanmax(s['rhat']):.4f}  ess_bulk min {np.nanmin(s['ess_bulk']):.0f}  ess_tail min {np.nanmin(s['ess_tail']):.0f}  "
        f"ess_mean min {np.nanmin(s['ess_mean']):.0f} of {2 * (view.shape[0] // 2) * a.walkers} draws")
integrated_time(x, tol=0)
for rep in range(a.reps):
    tau, t = timed(lambda: integrated_time(x, tol=0))
    say(f"integrated_time(tol=0) on the whole chain (what get_autocorr_time runs) rep {rep}: {t * 1e3:8.1f} ms, tau max {np.max(tau):.2f}")
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
