"""Launch-per-half-step cost of the DE, snooker, walk and KDE moves against the stretch move at C3 (N = 2000, d = 10, W = 256).

A move set holding a DEMove or a SnookerMove runs alabi_ens_run with one launch per half step (the two- and three-partner
instantiations of ens_half_kernel); the stretch move is measured on the same path (ALABI_ENS_STREAM=0), so the sets differ in
the proposal's construction alone.  A set holding a WalkMove or a KDEMove runs the whole-half instantiation, a KDE set one
pre-pass launch in front of every half step as well ("de_with_idle_prepass": a KDE move of weight 0 beside DE, so the pre-pass
is launched and leaves at once).  Prints the median of --runs timed runs of --steps steps each, in us per half step, as one
JSON line.

    python tools/prof_moves.py                      # this checkout
    python tools/prof_moves.py --root ../parent     # another checkout (one without alabi_amd.moves measures the stretch run only)
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--steps", type=int, default=2048)
ap.add_argument("--tag", default="")
args = ap.parse_args()
os.environ["ALABI_ENS_STREAM"] = "0"                # read when the ensemble handle is created
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from alabi_amd import EnsembleSampler, HipGP  # noqa: E402
from alabi_amd.workloads import make_config  # noqa: E402

cfg = make_config("C3")
h = cfg["hyper"]
gp = HipGP(cfg["d"], h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"])
gp.compute(cfg["X"])


def measure(**kw):
    s = EnsembleSampler(cfg["W"], cfg["d"], gp, cfg["y"], cfg["bounds"], seed=5, **kw)
    s.run_mcmc(cfg["p0"], 600, store=False)         # warm-up: graph capture included
    torch.cuda.synchronize()
    us = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.run_mcmc(None, args.steps, store=True)
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) / (2 * args.steps) * 1e6)
        acc = float(s.acceptance_fraction.mean())
        s.reset()
    assert s.last_path == "launch-per-half-step", s.last_path
    return {"median_us_per_half_step": float(np.median(us)), "min": float(np.min(us)), "max": float(np.max(us)),
            "runs": [round(u, 4) for u in us], "acceptance": acc}


out = {"tag": args.tag, "root": os.path.abspath(args.root), "config": "C3", "steps": args.steps, "stretch": measure()}
try:
    from alabi_amd.moves import DEMove, StretchMove
except ImportError:
    out["de"] = None                                # a checkout without the moves
else:
    out["de"] = measure(moves=DEMove())
    out["de_stretch_mix"] = measure(moves=[(DEMove(), 0.5), (StretchMove(), 0.5)])
    try:
        from alabi_amd.moves import SnookerMove
    except ImportError:
        out["snooker"] = None                       # a checkout without the snooker move
    else:
        out["snooker"] = measure(moves=SnookerMove())
        out["de_snooker_mix"] = measure(moves=[(DEMove(), 0.8), (SnookerMove(), 0.2)])
    try:
        from alabi_amd.moves import KDEMove, WalkMove
    except ImportError:
        out["walk"] = None                          # a checkout without the walk and KDE moves
    else:
        out["walk"] = measure(moves=WalkMove())
        out["walk_s8"] = measure(moves=WalkMove(s=8))
        out["kde"] = measure(moves=KDEMove())
        out["de_kde_mix"] = measure(moves=[(DEMove(), 0.7), (KDEMove(), 0.3)])
        out["de_with_idle_prepass"] = measure(moves=[(DEMove(), 1.0), (KDEMove(), 0.0)])
print(json.dumps(out))
