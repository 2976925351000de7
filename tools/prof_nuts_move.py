"""Time per transition of the NUTS move at C3 (N = 2000, d = 10, 256 walkers) and at 1024 walkers, chain stored, by device events,
beside the HMC move of the same visit:

  (h1) (h8)  HMCMove with n_leapfrog = 1 and 8 on ens_hmc_kernel (path 5): the yardstick -- the time per value-and-gradient
             evaluation is the slope (h8 - h1) / 7, what one more leapfrog step costs, measured afresh in this run,
  (n)        NUTSMove(max_depth = --depth) with the same cov and step size on ens_nuts_kernel (path 6): us per transition, leaves per
             transition (alabi_ens_nuts_stats of the timed round), us per leaf, mean depth, divergences, mean acceptance statistic,
  and the same three at 1024 walkers.

The variants are timed in alternation, --runs rounds of --steps steps each after a warm-up of every variant, so that what else
the device is doing falls on all of them alike; the median, the minimum and the maximum of the rounds are printed as one JSON
line.  Derived: us per leaf over us per value-and-gradient evaluation -- what the tree logic, the second half kick, the fourth
barrier and the load imbalance between walkers (a launch ends with its deepest trees) add to an evaluation.

    python tools/prof_nuts_move.py > profiles/moves_step_nuts.txt

--adapt measures the warm-up instead (256 walkers):
  (s) (a)    --steps sampling transitions on ens_nuts_kernel and as many warm-up transitions on ens_nuts_adapt_kernel
             (alabi_ens_nuts_adapt) in alternation, from the same walkers, at the same draw counter and with the state frozen at the
             same step size (gamma = inf, mu = ln e): the same trees (leaf for leaf where exp(ln e) = e), so the difference is what
             ADAPT costs; leaves per transition are printed for both,
  (t)        EnsembleSampler.tune_nuts(500) end to end from NUTSMove(cov): seconds, the step size and the terminal mean acceptance
             statistic it lands on, with and without the step-size search, beside tune_hmc(500) of HMCMove(cov, n_leapfrog=4).

    python tools/prof_nuts_move.py --adapt > profiles/moves_step_nuts_adapt.txt
"""
import argparse
import ctypes as C
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--steps", type=int, default=512)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--tag", default="")
ap.add_argument("--adapt", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from alabi_amd import EnsembleSampler, HipGP, _lib  # noqa: E402
from alabi_amd.moves import HMCMove, NUTSMove  # noqa: E402
from alabi_amd.workloads import make_config  # noqa: E402

assert torch.cuda.is_available(), "this measurement needs the GPU"
cfg = make_config("C3")
h = cfg["hyper"]
d = cfg["d"]
gp = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"])
gp.compute(cfg["X"])
width = cfg["bounds"][:, 1] - cfg["bounds"][:, 0]
cov = (0.05 * width) ** 2                                   # the mass matrix of tools/prof_hmc_move.py


def make(W, p0, moves):
    s = EnsembleSampler(W, d, gp, cfg["y"], cfg["bounds"], seed=5, moves=moves)
    s.run_mcmc(p0, 100, store=False)                       # warm-up: code objects
    torch.cuda.synchronize()
    return s


def timed(s):
    nuts = s.nuts_stats is not None
    if nuts:
        s.nuts_counts(reset=True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    s.run_mcmc(None, args.steps, store=True)
    b.record()
    torch.cuda.synchronize()
    acc = float(s.acceptance_fraction.mean())
    extra = None
    if nuts:
        counts, a_sum = s.nuts_counts(reset=True)
        n = args.steps * s.total_walkers
        extra = {"leaves_per_transition": float(counts[:, 0].sum()) / n, "mean_depth": float(counts[:, 1].sum()) / n,
                 "divergences": int(counts[:, 2].sum()), "mean_accept_stat": float(a_sum.sum()) / max(int(counts[:, 0].sum()), 1),
                 "most_leaves_of_a_walker_over_mean": float(counts[:, 0].max()) / max(float(counts[:, 0].mean()), 1.0)}
    s.reset()
    return a.elapsed_time(b) * 1e3 / args.steps, acc, extra


def adapt_report():
    W, p0 = int(cfg["W"]), cfg["p0"]
    eps = float(d) ** -0.25
    s = make(W, p0, NUTSMove(cov, max_depth=args.depth))
    par = _lib.host_doubles((0.8, float("inf"), 10.0, 0.75))
    state = torch.zeros((W, 5), dtype=torch.float64, device="cuda")
    state[:, 2] = state[:, 4] = float(np.log(eps))
    counts = torch.zeros((W, 3), dtype=torch.int64, device="cuda")
    leaf_sum, stat = torch.zeros(W, dtype=torch.float64, device="cuda"), torch.zeros(W, dtype=torch.float64, device="cuda")
    chain = torch.empty((args.steps, W, d), dtype=torch.float64, device="cuda")
    us, leaves = {"sample": [], "adapt": []}, {"sample": [], "adapt": []}
    for r in range(args.runs + 1):                             # round 0 warms the adapt kernel's code object up
        c0, l0, step0 = s._coords.clone(), s._logp.clone(), s._rng_step
        t, _, extra = timed(s)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        counts.zero_(); state[:, 0] = 0.0
        torch.cuda.synchronize()
        a.record()
        _lib.check(_lib.lib().alabi_ens_nuts_adapt(s._ens, _lib.ptr(c0), _lib.ptr(l0), step0, args.steps, 1, _lib.ptr(state), par, _lib.ptr(chain),
                                                   None, None, _lib.ptr(counts), _lib.ptr(leaf_sum), _lib.ptr(stat), _lib.current_stream()),
                   "alabi_ens_nuts_adapt")
        b.record()
        torch.cuda.synchronize()
        same = bool(torch.equal(c0, s._coords))                # exp(ln e) may be an ulp off e: then the trees differ in detail only
        if r:
            us["sample"].append(t); us["adapt"].append(a.elapsed_time(b) * 1e3 / args.steps)
            leaves["sample"].append(extra["leaves_per_transition"]); leaves["adapt"].append(float(counts[:, 0].sum()) / (args.steps * W))
    out = {"tag": args.tag, "config": "C3", "N": int(cfg["X"].shape[0]), "d": d, "W": W, "steps": args.steps, "runs": args.runs,
           "step_size": eps, "max_depth": args.depth, "unit": "us per transition, device events, chain stored; frozen state: the same trees"}
    for k in us:
        out[k] = {"median": float(np.median(us[k])), "min": float(np.min(us[k])), "max": float(np.max(us[k])),
                  "runs": [round(x, 3) for x in us[k]], "leaves_per_transition": float(np.median(leaves[k]))}
    out["adapt_over_sample"] = out["adapt"]["median"] / out["sample"]["median"]
    out["adapt_us_per_leaf_over_sample"] = (out["adapt"]["median"] / out["adapt"]["leaves_per_transition"]) / (
        out["sample"]["median"] / out["sample"]["leaves_per_transition"])
    out["same_walkers_after_the_last_round"] = same
    s._release()
    tune = {}
    for key, kw in (("search", {}), ("no_search", {"init_step_size": None})):
        best = None
        for rep in range(2):                                   # the second call has its code objects
            t = EnsembleSampler(W, d, gp, cfg["y"], cfg["bounds"], seed=5, moves=NUTSMove(cov, max_depth=args.depth))
            t.tune_nuts(p0, nwarmup=500, **kw)
            best = {k: v for k, v in t.nuts_tuning.items() if k in ("step_size", "step_sizes", "mean_accept_stat", "mean_depth", "divergences",
                                                                    "seconds", "window_ends")}
            best["search_iters_min_max"] = [[int(i.min()), int(i.max())] for i in t.nuts_tuning["search_iters"]]
            if rep:
                t.run_mcmc(None, 200)
                best["next_200_transitions"] = t.nuts_stats
            t._release()
        tune["tune_nuts_" + key] = best
    for rep in range(2):
        t = EnsembleSampler(W, d, gp, cfg["y"], cfg["bounds"], seed=5, moves=HMCMove(cov, n_leapfrog=4))
        t.tune_hmc(p0, nwarmup=500)
        tune["tune_hmc_4_leapfrog"] = {k: v for k, v in t.hmc_tuning.items() if k in ("step_size", "step_sizes", "mean_accept_stat", "seconds")}
        t._release()
    out["tune_500"] = tune
    print(json.dumps(out))


if args.adapt:
    adapt_report()
    sys.exit(0)

p0 = cfg["p0"]
rs = np.random.RandomState(9)
p1024 = cfg["bounds"][:, 0] + width * rs.uniform(0.3, 0.7, (1024, d))
variants = {}
for tag, W, start in (("", cfg["W"], p0), ("_1024", 1024, p1024)):
    for L in (1, 8):
        variants[f"h{L}{tag}"] = make(W, start, HMCMove(cov, n_leapfrog=L))
    variants["n" + tag] = make(W, start, NUTSMove(cov, max_depth=args.depth))
us = {k: [] for k in variants}
accs, paths, trees = {}, {}, {k: [] for k in variants if k[0] == "n"}
for r in range(args.runs):
    for k, s in variants.items():
        t, accs[k], extra = timed(s)
        paths[k] = s.last_path
        us[k].append(t)
        if extra is not None:
            trees[k].append(extra)
assert all(paths[k] == {"h": "hmc", "n": "nuts"}[k[0]] for k in paths), paths
plan = (C.c_int * 4)()
_lib.lib().alabi_ens_nuts_plan(variants["n"]._ens, plan)
out = {"tag": args.tag, "config": "C3", "N": int(cfg["X"].shape[0]), "d": d, "W": int(cfg["W"]), "steps": args.steps, "runs": args.runs,
       "step_size": float(d) ** -0.25, "max_depth": args.depth, "unit": "us per transition (full step), device events, chain stored",
       "nuts_plan": dict(zip(("threads", "chunk", "lds_bytes", "tiled"), map(int, plan)))}
med = {}
for k, v in us.items():
    med[k] = float(np.median(v))
    out[k] = {"median": med[k], "min": float(np.min(v)), "max": float(np.max(v)), "runs": [round(x, 3) for x in v], "path": paths[k],
              "acceptance": accs[k]}
    if k in trees:
        out[k]["trees"] = {key: float(np.median([t[key] for t in trees[k]])) for key in trees[k][0]}
for tag in ("", "_1024"):
    grad = (med["h8" + tag] - med["h1" + tag]) / 7.0
    leaves = out["n" + tag]["trees"]["leaves_per_transition"]
    per_leaf = med["n" + tag] / leaves
    out["derived" + tag] = {"us_per_transition": med["n" + tag], "leaves_per_transition": leaves, "us_per_leaf": per_leaf,
                            "us_per_value_and_gradient_evaluation_hmc": grad, "leaf_over_hmc_evaluation": per_leaf / grad,
                            "us_per_step_hmc8": med["h8" + tag]}
print(json.dumps(out))
for s in variants.values():                                # not at interpreter shutdown, when the library may be gone
    s._release()
