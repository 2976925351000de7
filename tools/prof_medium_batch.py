"""Mean + variance for 17 ... 128 queries: groups of 16 through predict_var_small_kernel (ALABI_PV_SMALL=1, the default up to
128 queries, 64 beyond Npad = 2048) against the K* pre-pass + tile product (ALABI_PV_SMALL=0).  The cross-over itself is a constant
of predict_var_small (csrc/predict_plan.hip); moving it takes a rebuild.
PYTHONPATH=. python tools/prof_medium_batch.py [C3 C4 ...]"""
import os, sys, time
import numpy as np, torch
from alabi_amd import HipGP
from alabi_amd.workloads import make_config
for name in (sys.argv[1:] or ["C3", "C4"]):
    cfg = make_config(name); h = cfg["hyper"]
    gp = HipGP(cfg["d"], h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"]); gp.compute(cfg["X"])
    y = torch.as_tensor(cfg["y"], device="cuda")
    Xs = torch.as_tensor(np.random.RandomState(0).uniform(cfg["bounds"][:, 0], cfg["bounds"][:, 1], (128, cfg["d"])), device="cuda")
    for M in (17, 32, 64, 96, 128):
        row = []
        for small in ("0", "1"):
            os.environ["ALABI_PV_SMALL"] = small
            r = gp.predict_device(y, Xs[:M], return_var=True); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(30): r = gp.predict_device(y, Xs[:M], return_var=True)
            torch.cuda.synchronize(); row.append(((time.perf_counter() - t0) / 30 * 1e3, r[1].cpu().numpy()))
        print(f"{name} M={M}: tiles {row[0][0]:.3f} ms, groups of 16 {row[1][0]:.3f} ms, max |dvar|/amp {np.max(np.abs(row[0][1]-row[1][1]))/np.exp(h['log_amp']):.1e}", flush=True)
