"""Times SurrogateModel.find_map(method="bfgs-gpu") against the Nelder-Mead default, and laplace_approximation, at the C3 size
(N_train = 2000, d = 10), both in the same visit on the same model; writes profiles/map_find.txt.

    python tools/prof_map.py [--ntrain 2000] [--ndim 10] [--restarts 15] [--repeat 3]

The model has the bench's flagship shape: a Gaussian-like log-likelihood on [-3, 3]^d, 2000 uniform training points, a
squared-exponential surrogate whose hyper-parameters are fitted once by maximum likelihood (init_gp, one restart) before anything is
timed, so that the two methods see one fixed surrogate.
Each method is timed ``repeat`` times after one untimed call; the median is reported with the spread.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ntrain", type=int, default=2000)
    ap.add_argument("--ndim", type=int, default=10)
    ap.add_argument("--restarts", type=int, default=15)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_find.txt"))
    a = ap.parse_args()
    import torch
    from alabi_amd import SurrogateModel
    d = a.ndim
    centre = np.linspace(-0.8, 0.8, d)
    scale = np.linspace(0.6, 1.4, d)

    def lnlike(theta):
        r = (np.asarray(theta, dtype=np.float64).reshape(-1) - centre) / scale
        return float(-0.5 * r @ r)

    sm = SurrogateModel(lnlike_fn=lnlike, bounds=[(-3.0, 3.0)] * d, savedir=tempfile.mkdtemp(), verbose=False, random_state=0)
    sm.init_samples(ntrain=a.ntrain, ntest=20, sampler="uniform")
    sm.init_gp(kernel="ExpSquaredKernel", fit_amp=True, fit_mean=True, white_noise=-9, hyperopt_method="ml", gp_nopt=1)

    def timed(fn):
        fn()
        out = []
        for _ in range(a.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return out

    t_nm = timed(lambda: sm.find_map(nRestarts=a.restarts))
    nm = dict(lnprob=float(sm.map_lnprob), theta=sm.map_theta.tolist())
    t_gpu = timed(lambda: sm.find_map(method="bfgs-gpu", nRestarts=a.restarts))
    gpu = dict(lnprob=float(sm.map_lnprob), status=int(sm.map_status), evaluations=int(sm.map_evaluations), theta=sm.map_theta.tolist())
    t_lap = timed(lambda: sm.laplace_approximation(nRestarts=64))
    # the launch alone: the starts on the device already
    s = sm._map_sampler
    starts = torch.as_tensor(np.random.RandomState(0).uniform(-2.9, 2.9, (64, d)) * sm._map_plan.t_mult + sm._map_plan.t_add, device="cuda")
    s.maximize(starts)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record(); res = s.maximize(starts); ev1.record(); torch.cuda.synchronize()
    launch_ms = ev0.elapsed_time(ev1)
    ev0.record(); s.log_prob_hessian(res.x[:1]); ev1.record(); torch.cuda.synchronize()
    hess_ms = ev0.elapsed_time(ev1)
    rec = dict(device=torch.cuda.get_device_name(0), ntrain=a.ntrain, ndim=d, restarts=a.restarts, repeat=a.repeat,
               find_map_nelder_mead_s=dict(median=float(np.median(t_nm)), all=t_nm), find_map_bfgs_gpu_s=dict(median=float(np.median(t_gpu)), all=t_gpu),
               laplace_approximation_s=dict(median=float(np.median(t_lap)), all=t_lap),
               maximize_64_starts_launch_ms=launch_ms, maximize_64_starts_evaluations=int(res.evaluations.sum().item()),
               maximize_64_starts_status=sorted(set(res.status.cpu().tolist())), log_prob_hessian_1_point_ms=hess_ms,
               nelder_mead=nm, bfgs_gpu=gpu, laplace_logz=sm.laplace_logz, map_on_bound=sm.map_on_bound.tolist(),
               speedup=float(np.median(t_nm) / np.median(t_gpu)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("find_map at N_train = %d, d = %d, %d restarts, same visit, same model (tools/prof_map.py)\n" % (a.ntrain, d, a.restarts))
        f.write("  Nelder-Mead (default)      %.4f s  (median of %d: %s)\n" % (np.median(t_nm), a.repeat, ["%.4f" % t for t in t_nm]))
        f.write("  method=\"bfgs-gpu\"          %.4f s  (median of %d: %s)\n" % (np.median(t_gpu), a.repeat, ["%.4f" % t for t in t_gpu]))
        f.write("  laplace_approximation(64)  %.4f s  (median of %d: %s)\n" % (np.median(t_lap), a.repeat, ["%.4f" % t for t in t_lap]))
        f.write("  maximize, 64 starts, launch alone (HIP events): %.3f ms, %d evaluations; log_prob_hessian at one point: %.3f ms\n" % (
            launch_ms, rec["maximize_64_starts_evaluations"], hess_ms))
        f.write("  map_lnprob: Nelder-Mead %.12g, bfgs-gpu %.12g (status %d, %d evaluations)\n" % (nm["lnprob"], gpu["lnprob"], gpu["status"],
                                                                                                 gpu["evaluations"]))
        f.write(json.dumps(rec) + "\n")
    print(open(a.out).read())


if __name__ == "__main__":
    main()
