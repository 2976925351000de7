"""Time per full step of the Gaussian Metropolis move at C3 (N = 2000, d = 10, 256 walkers), chain stored, by device events:

  (a) GaussianMove on ens_mh_kernel (path 4: one workgroup per walker, all steps of a chunk in one launch),
  (b) the same set with one launch per half step (path 0, alabi_ens_set_stream(ens, 0)),
  (c) StretchMove on path 0,
  (d) the default persistent kernel,
  (a1024) as (a) with 1024 walkers.

The variants are timed in alternation, --runs rounds of --steps steps each after a warm-up of every variant, so that what else
the device is doing falls on all of them alike; the median, the minimum and the maximum of the rounds are printed as one JSON
line.  (a) and (b) must end with the same chain: the script compares them bit for bit before it reports a time.

    python tools/prof_gauss_move.py > profiles/moves_step_gauss.txt
"""
import argparse
import ctypes as C
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--steps", type=int, default=2048)
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from alabi_amd import EnsembleSampler, HipGP, _lib  # noqa: E402
from alabi_amd.moves import GaussianMove, StretchMove  # noqa: E402
from alabi_amd.workloads import make_config  # noqa: E402

assert torch.cuda.is_available(), "this measurement needs the GPU"
cfg = make_config("C3")
h = cfg["hyper"]
d = cfg["d"]
gp = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"])
gp.compute(cfg["X"])
width = cfg["bounds"][:, 1] - cfg["bounds"][:, 0]
cov = (0.05 * width) ** 2                                   # a diagonal proposal, 5 % of the box per coordinate


def make(W, p0, path0=False, **kw):
    s = EnsembleSampler(W, d, gp, cfg["y"], cfg["bounds"], seed=5, **kw)
    s._ensure_ens()
    if path0:
        _lib.check(_lib.lib().alabi_ens_set_stream(s._ens, 0), "alabi_ens_set_stream")
    s.run_mcmc(p0, 600, store=False)                       # warm-up: code objects, graph capture
    torch.cuda.synchronize()
    return s


def timed(s):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    s.run_mcmc(None, args.steps, store=True)
    b.record()
    torch.cuda.synchronize()
    chain = s.get_chain_device()[-args.steps:].clone()
    acc = float(s.acceptance_fraction.mean())
    s.reset()
    return a.elapsed_time(b) * 1e3 / args.steps, chain, acc


p0 = cfg["p0"]
rs = np.random.RandomState(9)
p1024 = cfg["bounds"][:, 0] + width * rs.uniform(0.3, 0.7, (1024, d))
variants = {
    "a_gauss_path4": make(cfg["W"], p0, moves=GaussianMove(cov)),
    "b_gauss_path0": make(cfg["W"], p0, path0=True, moves=GaussianMove(cov)),
    "c_stretch_path0": make(cfg["W"], p0, path0=True, moves=StretchMove()),
    "d_default_persistent": make(cfg["W"], p0),
    "a1024_gauss_path4": make(1024, p1024, moves=GaussianMove(cov)),
}
us = {k: [] for k in variants}
accs, paths = {}, {}
for r in range(args.runs):
    chains = {}
    for k, s in variants.items():
        t, chains[k], accs[k] = timed(s)
        us[k].append(t)
        paths[k] = s.last_path
    assert torch.equal(chains["a_gauss_path4"], chains["b_gauss_path0"]), "path 4 and path 0 differ"
assert paths["a_gauss_path4"] == "metropolis" and paths["b_gauss_path0"] == "launch-per-half-step", paths
plan = (C.c_int * 4)()
_lib.lib().alabi_ens_mh_plan(variants["a_gauss_path4"]._ens, plan)
out = {"tag": args.tag, "config": "C3", "N": int(cfg["X"].shape[0]), "d": d, "steps": args.steps, "runs": args.runs,
       "unit": "us per full step, device events, chain stored", "mh_plan": dict(zip(("threads", "chunk", "lds_bytes", "tiled"), map(int, plan)))}
for k, v in us.items():
    out[k] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "runs": [round(x, 3) for x in v],
              "path": paths[k], "acceptance": accs[k]}
print(json.dumps(out))
for s in variants.values():                                # not at interpreter shutdown, when the library may be gone
    s._release()
