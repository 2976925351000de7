"""Time per full step of the HMC move at C3 (N = 2000, d = 10, 256 walkers) and at 1024 walkers, chain stored, by device events:

  (g)  GaussianMove on ens_mh_kernel (path 4): one VALUE evaluation per step -- the yardstick of the same visit,
  (h1) (h4) (h8)  HMCMove with n_leapfrog = 1, 4, 8 on ens_hmc_kernel (path 5): n_leapfrog value-and-gradient evaluations per step,
  and the same four at 1024 walkers.

The variants are timed in alternation, --runs rounds of --steps steps each after a warm-up of every variant, so that what else
the device is doing falls on all of them alike; the median, the minimum and the maximum of the rounds are printed as one JSON
line.  Derived: the time per value-and-gradient evaluation is the slope (h8 - h1) / 7 -- what one more leapfrog step costs, free of
the per-step overhead (draws, accept test, chain store) --, the time per value evaluation is (g), which includes that overhead and
so flatters the ratio a little; both are printed with their ratio.

    python tools/prof_hmc_move.py > profiles/moves_step_hmc.txt

--adapt adds the warm-up: (a1) (a4) (a8) are the same moves on ens_hmc_adapt_kernel (alabi_ens_hmc_adapt, dual averaging running
from a fresh state every round, chain stored), timed in the same alternation, so "adapt_over_hmc" compares the two kernels within
one visit; and EnsembleSampler.tune_hmc(nwarmup=500) is run once from the Laplace covariance at the MAP (what
SurrogateModel.laplace_approximation calls map_cov_scaled) and once from identity cov, n_leapfrog = 4, with its wall time, the
step size and the terminal acceptance statistic it lands on.

    python tools/prof_hmc_move.py --adapt > profiles/moves_step_hmc_adapt.txt
"""
import argparse
import ctypes as C
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--steps", type=int, default=1024)
ap.add_argument("--tag", default="")
ap.add_argument("--adapt", action="store_true", help="also time ens_hmc_adapt_kernel and a tune_hmc(nwarmup=500)")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from alabi_amd import EnsembleSampler, HipGP, _lib  # noqa: E402
from alabi_amd.moves import GaussianMove, HMCMove  # noqa: E402
from alabi_amd.workloads import make_config  # noqa: E402

assert torch.cuda.is_available(), "this measurement needs the GPU"
cfg = make_config("C3")
h = cfg["hyper"]
d = cfg["d"]
gp = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"])
gp.compute(cfg["X"])
width = cfg["bounds"][:, 1] - cfg["bounds"][:, 0]
cov = (0.05 * width) ** 2                                   # the proposal scale of tools/prof_gauss_move.py, here the mass matrix


def make(W, p0, moves):
    s = EnsembleSampler(W, d, gp, cfg["y"], cfg["bounds"], seed=5, moves=moves)
    s.run_mcmc(p0, 200, store=False)                       # warm-up: code objects
    torch.cuda.synchronize()
    return s


def timed(s):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    s.run_mcmc(None, args.steps, store=True)
    b.record()
    torch.cuda.synchronize()
    acc = float(s.acceptance_fraction.mean())
    s.reset()
    return a.elapsed_time(b) * 1e3 / args.steps, acc


def timed_adapt(s):
    """--steps warm-up steps on ens_hmc_adapt_kernel from a fresh dual-averaging state, chain stored."""
    from alabi_amd import hmc_adapt as ha
    state = torch.as_tensor(ha.initial_state(s.total_walkers, s.moves[0][0].resolved_step_size(d)), device="cuda")
    chain = torch.empty((args.steps, s.total_walkers, d), dtype=torch.float64, device="cuda")
    stat = torch.zeros(s.total_walkers, dtype=torch.float64, device="cuda")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    s._hmc_adapt(args.steps, state, ha.DA_DEFAULTS, chain=chain, accept_stat=stat)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / args.steps, float(stat.mean()) / args.steps


p0 = cfg["p0"]
rs = np.random.RandomState(9)
p1024 = cfg["bounds"][:, 0] + width * rs.uniform(0.3, 0.7, (1024, d))
variants = {}
for tag, W, start in (("", cfg["W"], p0), ("_1024", 1024, p1024)):
    variants["g" + tag] = make(W, start, GaussianMove(cov))
    for L in (1, 4, 8):
        variants[f"h{L}{tag}"] = make(W, start, HMCMove(cov, n_leapfrog=L))
        if args.adapt:
            variants[f"a{L}{tag}"] = make(W, start, HMCMove(cov, n_leapfrog=L))
us = {k: [] for k in variants}
accs, paths = {}, {}
for r in range(args.runs):
    for k, s in variants.items():
        if k.startswith("a"):
            t, accs[k] = timed_adapt(s)                     # (acceptance: the mean acceptance statistic of the round)
            paths[k] = "hmc-adapt"
        else:
            t, accs[k] = timed(s)
            paths[k] = s.last_path
        us[k].append(t)
assert all(paths[k] == {"g": "metropolis", "h": "hmc", "a": "hmc-adapt"}[k[0]] for k in paths), paths
plan = (C.c_int * 4)()
_lib.lib().alabi_ens_hmc_plan(variants["h8"]._ens, plan)
out = {"tag": args.tag, "config": "C3", "N": int(cfg["X"].shape[0]), "d": d, "W": int(cfg["W"]), "steps": args.steps, "runs": args.runs,
       "step_size": float(d) ** -0.25, "unit": "us per full step, device events, chain stored",
       "hmc_plan_h8": dict(zip(("threads", "chunk", "lds_bytes", "tiled"), map(int, plan)))}
med = {}
for k, v in us.items():
    med[k] = float(np.median(v))
    out[k] = {"median": med[k], "min": float(np.min(v)), "max": float(np.max(v)), "runs": [round(x, 3) for x in v], "path": paths[k],
              "acceptance": accs[k]}
for tag in ("", "_1024"):
    grad = (med["h8" + tag] - med["h1" + tag]) / 7.0
    out["derived" + tag] = {"us_per_value_and_gradient_evaluation": grad, "us_per_value_evaluation": med["g" + tag],
                            "ratio": grad / med["g" + tag], "us_per_step_overhead_h1": med["h1" + tag] - grad}
if args.adapt:
    out["adapt_over_hmc"] = {f"L{L}{tag}": med[f"a{L}{tag}"] / med[f"h{L}{tag}"] for tag in ("", "_1024") for L in (1, 4, 8)}
    out["hmc_run_to_run_spread"] = {k: (float(np.max(v)) - float(np.min(v))) / med[k] for k, v in us.items() if k[0] in "ha"}
    # tune_hmc(nwarmup=500) at C3 from the Laplace covariance at the MAP and from identity cov
    from alabi_amd.laplace import laplace_covariance  # noqa: E402
    base = variants["h4"]
    res = base.maximize(torch.as_tensor(p0[:16], device="cuda"))
    best = int(torch.argmax(res.log_prob))
    H = base.log_prob_hessian(res.x[best:best + 1])[0].cpu().numpy()
    lap = laplace_covariance(H)
    out["tune_hmc"] = {}
    for name, c in (("map_cov", lap), ("identity", 1.0)):
        if c is None:
            out["tune_hmc"][name] = "the Hessian at the best maximum is not negative definite"
            continue
        for nwarm in (100, 500):                           # the first on a sampler of its own: code objects, allocator
            s = EnsembleSampler(cfg["W"], d, gp, cfg["y"], cfg["bounds"], seed=5, moves=HMCMove(c, n_leapfrog=4))
            s.tune_hmc(p0, nwarmup=nwarm)
            torch.cuda.synchronize()
            if nwarm == 100:
                s._release()
        tun = s.hmc_tuning
        s.run_mcmc(None, 500, store=False)
        out["tune_hmc"][name] = {"nwarmup": 500, "n_leapfrog": 4, "wall_seconds": tun["seconds"], "step_size": tun["step_size"],
                                 "step_sizes_at_window_ends": tun["step_sizes"], "mean_accept_stat_terminal": tun["mean_accept_stat"],
                                 "acceptance_fraction_next_500": float(s.acceptance_fraction.mean()),
                                 "adapted_variances": [float(v) for v in tun["cov"]]}
        s._release()
print(json.dumps(out))
for s in variants.values():                                # not at interpreter shutdown, when the library may be gone
    s._release()
