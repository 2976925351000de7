"""The convergence loop of the reference's KL-vs-iteration tutorial on one benchmark, without plotting: init_samples / init_gp,
then batches of active_train each followed by run_dynesty on the surrogate, one run_dynesty on the true likelihood, and the
KDE KL divergence (alabi_amd.metrics.kl_divergence_kde) between each surrogate posterior and the true one.

    python tools/demo_kl_vs_iteration.py                       # gaussian_2d, 5 batches of 10 iterations
    python tools/demo_kl_vs_iteration.py eggbox 8 20           # benchmark, batches, iterations per batch
"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from alabi_amd import SurrogateModel, benchmarks, metrics
    name = sys.argv[1] if len(sys.argv) > 1 else "gaussian_2d"
    nbatch = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    per = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    bench = getattr(benchmarks, name)
    t_all = time.perf_counter()
    with tempfile.TemporaryDirectory() as savedir:
        sm = SurrogateModel(lnlike_fn=bench["fn"], bounds=bench["bounds"], savedir=savedir, verbose=False, random_state=0,
                            cache=False)
        sm.init_samples(ntrain=5)
        sm.init_gp(kernel="ExpSquaredKernel", fit_amp=True, fit_mean=True, white_noise=-12, hyperopt_method="ml")
        t0 = time.perf_counter()
        sm.run_dynesty(like_fn="true", mode="static", sampler_kwargs={"seed": 1}, min_ess=5000)
        true = sm.dynesty_samples
        print(f"true run_dynesty: {true.shape[0]} samples in {time.perf_counter() - t0:.2f} s", flush=True)
        for b in range(1, nbatch + 1):
            t0 = time.perf_counter()
            sm.active_train(niter=per, algorithm="bape", gp_opt_freq=10)
            t_train = time.perf_counter() - t0
            t0 = time.perf_counter()
            sm.run_dynesty(mode="static", sampler_kwargs={"seed": 1 + b}, min_ess=5000)
            t_ns = time.perf_counter() - t0
            t0 = time.perf_counter()
            kl = metrics.kl_divergence_kde(sm.dynesty_samples, true)
            t_kl = time.perf_counter() - t0
            print(f"batch {b}: ntrain {len(sm._theta):4d}  KL {kl:.5f}  (active_train {t_train:.2f} s, run_dynesty {t_ns:.3f} s, "
                  f"kl_divergence_kde {t_kl * 1e3:.1f} ms)", flush=True)
    print(f"total wall {time.perf_counter() - t_all:.2f} s")


if __name__ == "__main__":
    main()
