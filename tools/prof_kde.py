"""DeviceKDE measurements (DESIGN.md "Gaussian KDE"): logpdf and kl_divergence_kde at the shapes of the convergence loop
against scipy.stats.gaussian_kde.  Per (N, d, M): the wall time of DeviceKDE.logpdf on device tensors, the kernel time between
HIP events around it, kernel evaluations per second, the same logpdf through scipy (timed on a subset of the points and
scaled linearly when N M d is large), and kl_divergence_kde with both sample sets of size N and n_eval = M (wall; scipy's
estimate = two KDE pdf evaluations at M points).

    python tools/prof_kde.py                 # all four shapes, one JSON line each
    python tools/prof_kde.py 100000 2 1000   # one shape
"""
import json
import os
import sys
import time

import numpy as np
import torch
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(100000, 2, 1000), (200000, 10, 1000), (20000, 10, 20000), (1000000, 20, 1000)]
FP64_VALU_PEAK = 39.3e12         # fp64 vector lane-instructions / s (78.6 TFLOP/s counted as FMA = 2 flops)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def measure(N, d, M, reps=20):
    from alabi_amd import DeviceKDE, metrics
    rng = np.random.default_rng(N + d + M)
    X = rng.normal(size=(d, N))
    Q = rng.normal(size=(d, M)) * 1.2
    Xd, Qd = torch.as_tensor(X, device="cuda"), torch.as_tensor(Q, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kde = DeviceKDE(Xd)
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0
    for _ in range(3):
        kde.logpdf(Qd)
    torch.cuda.synchronize()
    walls, kern = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        kde.logpdf(Qd)
        e1.record()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        kern.append(e0.elapsed_time(e1) * 1e-3)
    t_wall, t_kern = float(np.median(walls)), float(np.median(kern))
    # scipy: the whole call when cheap, else a subset of the points scaled to M
    ref = stats.gaussian_kde(X)
    m_sub = M if N * M * d <= 2e9 else max(8, int(2e9 / (N * d)))
    t0 = time.perf_counter()
    ref_log = ref.logpdf(Q[:, :m_sub])
    t_scipy = (time.perf_counter() - t0) * M / m_sub
    err = float(np.max(np.abs(kde.logpdf(Q[:, :m_sub]) - ref_log)))
    # kl_divergence_kde: two sample sets of N, M evaluation points
    Y = rng.normal(size=(N, d)) * 1.1 + 0.1
    np.random.seed(0)
    metrics.kl_divergence_kde(X.T, Y, n_eval=M)                       # warm-up
    kls = []
    for _ in range(3):
        np.random.seed(0)
        t0 = time.perf_counter()
        metrics.kl_divergence_kde(X.T, Y, n_eval=M)
        kls.append(time.perf_counter() - t0)
    parts, pts = kde.plan(M)
    evals = float(N) * M
    emit(N=N, d=d, M=M, parts=parts, pts=pts, build_s=t_build, logpdf_wall_s=t_wall, logpdf_kernel_s=t_kern,
         evals_per_s=evals / t_kern, scipy_logpdf_s=t_scipy, scipy_points_timed=m_sub, speedup_wall=t_scipy / t_wall,
         max_abs_err_vs_scipy=err, kl_kde_wall_s=float(np.median(kls)), kl_kde_scipy_est_s=2 * t_scipy,
         valu_frac_at_12_per_eval=evals / t_kern * 12 / FP64_VALU_PEAK)


def main():
    torch.cuda.set_device(0)
    if len(sys.argv) == 4:
        measure(*(int(a) for a in sys.argv[1:]))
        return
    for shape in SHAPES:
        measure(*shape)


if __name__ == "__main__":
    main()
