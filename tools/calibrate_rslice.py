"""Calibration of the default number of slice updates per walk of sample="rslice" (alabi_amd.nested.SLICES_MULT), on the CPU:
the 24-D separable Gaussian of tests/rslice_numpy.py, nlive = 200, dlogz = 0.1, slices = m (3 + d) for m = 1..4, 8 seeds.
The rule (NOTES.md "Nested sampling"): the smallest m with |mean(log Z - truth)| <= 2 rms(logzerr) / sqrt(8).

    python tools/calibrate_rslice.py run SEED      # one JSON line per m for that seed (the seeds are independent processes)
    python tools/calibrate_rslice.py table FILE... # the decision table from the collected lines
"""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

D, NLIVE, DLOGZ = 24, 200, 0.1


def run(seed):
    from alabi_amd import nested as ns
    from rslice_numpy import SliceCubeBackend, separable_gaussian
    logl, lo, hi, truth = separable_gaussian(D)
    for m in (1, 2, 3, 4):
        be = SliceCubeBackend(logl, lo, hi, seed=1000 + seed)
        s = ns.NestedSampler(be, NLIVE, sample="rslice", slices=m * (3 + D), seed=seed)
        t0 = time.perf_counter()
        r = s.run_nested(dlogz=DLOGZ)
        print(json.dumps(dict(seed=seed, m=m, logz=float(r.logz[-1]), truth=truth, logzerr=float(r.logzerr[-1]),
                              niter=int(r.niter), ncall=int(r.ncall), n_stuck=int(r.n_stuck), scale=s.scale,
                              wall_s=time.perf_counter() - t0)), flush=True)


def table(files):
    rows = [json.loads(line) for f in files for line in open(f) if line.startswith("{")]
    for m in (1, 2, 3, 4):
        rr = [r for r in rows if r["m"] == m]
        if not rr:
            continue
        err = np.array([r["logz"] - r["truth"] for r in rr])
        rms = math.sqrt(np.mean([r["logzerr"] ** 2 for r in rr]))
        bound = 2 * rms / math.sqrt(len(rr))
        print(f"m={m} seeds={len(rr)} mean_err={err.mean():+.3f} bound={bound:.3f} rms_logzerr={rms:.3f} "
              f"evals_per_dead={np.mean([r['ncall'] / r['niter'] for r in rr]):.0f} "
              f"stuck={sum(r['n_stuck'] for r in rr)} scale={np.mean([r['scale'] for r in rr]):.2f} "
              f"{'PASS' if abs(err.mean()) <= bound else 'fail'}  errs={np.round(err, 2).tolist()}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]))
    else:
        table(sys.argv[2:])
