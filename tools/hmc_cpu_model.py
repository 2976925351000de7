"""CPU model of what the HMC move buys: integrated autocorrelation time of the stretch move against HMC on an analytic Gaussian
target, in plain NumPy (no GPU, no library; NOT a GPU timing).

Target: a d-dimensional Gaussian with standard deviations log-spaced from 0.1 to 1 (d = 32 by default), 64 walkers started from
exact draws.  Moves: the stretch move (a = 2, emcee's red-blue halves), and the rule of alabi_amd.moves.HMCMove with identity mass
(eps = 0.10, 16 leapfrog steps), with the diagonal covariance as ``cov`` (eps = 0.71, 4 leapfrog steps) and MALA with it (eps =
0.71, 1 step), and the rule of alabi_amd.moves.NUTSMove (tests/nuts_numpy.py: multinomial NUTS) with the diagonal covariance (eps =
0.71, max_depth 8), whose evaluations per step are the leaves it made per transition.  tau: the mean over coordinates of oracle.autocorr_oracle.integrated_time of the chain [steps, walkers, d].
Cost per independent sample in kernel sums: max(tau, 1) x (evaluations per step) x --grad-cost for a value-and-gradient evaluation
(4.1 value evaluations, measured on the device at C3: profiles/moves_step_hmc.txt), x 1 for a value evaluation.

    python tools/hmc_cpu_model.py [--d 32] [--seed 1]

--nuts-warmup runs only the NumPy statement of the NUTS warm-up (tests/nuts_adapt_numpy.py: step-size search, dual averaging on the
tree's mean acceptance statistic, windowed mass matrix) on the same target from identity mass, --warmup transitions of --walkers
walkers (16 by default in this leg), beside tests/hmc_adapt_numpy.py's warm-up of an HMC move with 4 leapfrog steps: the step sizes
and terminal acceptance statistics the two land on, and the recovered variances.

    python tools/hmc_cpu_model.py --nuts-warmup [--d 8] [--seed 1] [--warmup 300]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))   # the NumPy statement of NUTS
from oracle.autocorr_oracle import integrated_time  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--d", type=int, default=32)
ap.add_argument("--walkers", type=int, default=64)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--stretch-steps", type=int, default=40000)
ap.add_argument("--hmc-steps", type=int, default=4000)
ap.add_argument("--nuts-steps", type=int, default=1000)
ap.add_argument("--grad-cost", type=float, default=4.1)
ap.add_argument("--nuts-warmup", action="store_true")
ap.add_argument("--warmup", type=int, default=300)
args = ap.parse_args()
if args.nuts_warmup and "--walkers" not in sys.argv:
    args.walkers = 16
d, W = args.d, args.walkers
sd = np.logspace(-1.0, 0.0, d)
lnp = lambda x: -0.5 * np.sum((x / sd) ** 2, axis=-1)  # noqa: E731
grad = lambda x: -x / sd ** 2  # noqa: E731


def stretch(x, nsteps, rs, a=2.0):
    lp = lnp(x)
    chain = np.empty((nsteps, W, d)); nacc = 0
    half = W // 2
    for t in range(nsteps):
        for S, Cm in ((slice(0, half), slice(half, W)), (slice(half, W), slice(0, half))):
            s, c = x[S], x[Cm]
            z = ((a - 1.0) * rs.rand(len(s)) + 1.0) ** 2 / a
            q = c[rs.randint(len(c), size=len(s))]
            q = q - (q - s) * z[:, None]
            lq = lnp(q)
            acc = (d - 1) * np.log(z) + lq - lp[S] > np.log(rs.rand(len(s)))
            x[S] = np.where(acc[:, None], q, s); lp[S] = np.where(acc, lq, lp[S]); nacc += acc.sum()
        chain[t] = x
    return chain, nacc / (nsteps * W)


def hmc(x, nsteps, rs, c, eps, L):
    """alabi_amd.moves.HMCMove's rule with the diagonal scale factor c (C = diag(c))."""
    lp, g = lnp(x), grad(x)
    chain = np.empty((nsteps, W, d)); nacc = 0
    for t in range(nsteps):
        z0 = rs.randn(W, d)
        z = z0 + 0.5 * eps * c * g
        q = x.copy()
        for l in range(L):
            q = q + eps * c * z
            gq = grad(q)
            z = z + (0.5 * eps if l == L - 1 else eps) * c * gq
        lq = lnp(q)
        acc = lq - 0.5 * np.sum(z * z, axis=1) - lp + 0.5 * np.sum(z0 * z0, axis=1) > np.log(rs.rand(W))
        x = np.where(acc[:, None], q, x); lp = np.where(acc, lq, lp); g = np.where(acc[:, None], gq, g); nacc += acc.sum()
        chain[t] = x
    return chain, nacc / (nsteps * W)


def nuts(x, nsteps, rs, c, eps, max_depth):
    """alabi_amd.moves.NUTSMove's rule (tests/nuts_numpy.py) with the diagonal scale factor c; the box is far away."""
    import hmc_numpy as hm
    import nuts_numpy as nn
    tgt = hm.GaussianTarget(np.zeros(d), np.diag(sd ** 2), np.stack([-1e6 * np.ones(d), 1e6 * np.ones(d)], axis=1))
    lp, g, _ = tgt.value_grad(x)
    chain = np.empty((nsteps, W, d)); leaves = taken = 0
    for t in range(nsteps):
        x, lp, g, trace, _ = nn.nuts_step_arrays(tgt, x, lp, g, np.diag(c), eps, rs.randn(W, d), rs.randint(0, 1 << 30, size=W),
                                                 rs.rand(W, (1 << max_depth) - 1), rs.rand(W, max_depth), max_depth)
        leaves += trace[:, 1].sum(); taken += trace[:, 3].sum()
        chain[t] = x
    return chain, taken / (nsteps * W), leaves / (nsteps * W)


def nuts_warmup_leg():
    import hmc_adapt_numpy as han
    import hmc_numpy as hm
    import nuts_adapt_numpy as nan_
    tgt = hm.GaussianTarget(np.zeros(d), np.diag(sd ** 2), np.stack([np.full(d, -10.0), np.full(d, 10.0)], axis=1))
    p0 = np.random.RandomState(args.seed).randn(W, d) * sd
    eps0 = hm.default_step_size(d)
    res = {"target": f"{d}-D Gaussian, standard deviations log-spaced 0.1 ... 1, identity mass at the start", "walkers": W, "seed": args.seed,
           "nwarmup": args.warmup, "note": "CPU model in NumPy, not a GPU number"}
    for key, search in (("nuts_search", True), ("nuts_no_search", False)):
        w = nan_.warmup(tgt, p0, args.warmup, args.seed, (1.0, eps0, 8, None, 1.0), metric="diag", search=search)
        ratio = w.cov / sd ** 2
        res[key] = {"step_size": w.step_size, "step_sizes": w.step_sizes, "mean_accept_stat": w.mean_accept_stat, "mean_depth": w.mean_depth,
                    "divergences": w.divergences, "variance_ratio_min_max": [float(ratio.min()), float(ratio.max())],
                    "search_iters_min_max": [[int(i.min()), int(i.max())] for i in w.search_iters]}
    h = han.warmup(tgt, p0, args.warmup, args.seed, (1.0, eps0, 4, None, 1.0), metric="diag")
    ratio = h.cov / sd ** 2
    res["hmc_4_leapfrog"] = {"step_size": h.step_size, "step_sizes": h.step_sizes, "mean_accept_stat": h.mean_accept_stat,
                             "variance_ratio_min_max": [float(ratio.min()), float(ratio.max())]}
    print(json.dumps(res, indent=1))


if args.nuts_warmup:
    nuts_warmup_leg()
    sys.exit(0)

out = {"target": f"{d}-D Gaussian, standard deviations log-spaced 0.1 ... 1", "walkers": W, "seed": args.seed,
       "stretch_steps": args.stretch_steps, "hmc_steps": args.hmc_steps, "note": "CPU model in NumPy, not a GPU number"}
start = lambda rs: rs.randn(W, d) * sd  # noqa: E731
rs = np.random.RandomState(args.seed)
ch, acc = stretch(start(rs), args.stretch_steps, rs)
out["stretch"] = {"tau": float(np.mean(integrated_time(ch))), "acceptance": float(acc), "evaluations_per_step": 1, "cost_factor": 1}
for name, c, eps, L in (("hmc_identity_mass_eps0.10_L16", np.ones(d), 0.10, 16), ("hmc_diag_cov_eps0.71_L4", sd, 0.71, 4),
                        ("mala_diag_cov_eps0.71_L1", sd, 0.71, 1)):
    rs = np.random.RandomState(args.seed + 1)
    ch, acc = hmc(start(rs), args.hmc_steps, rs, c, eps, L)
    out[name] = {"tau": float(np.mean(integrated_time(ch))), "acceptance": float(acc), "evaluations_per_step": L, "cost_factor": args.grad_cost}
rs = np.random.RandomState(args.seed + 2)
ch, acc, leaves = nuts(start(rs), args.nuts_steps, rs, sd, 0.71, 8)
out["nuts_diag_cov_eps0.71_depth8"] = {"tau": float(np.mean(integrated_time(ch))), "moved_fraction": float(acc), "nuts_steps": args.nuts_steps,
                                       "evaluations_per_step": float(leaves), "cost_factor": args.grad_cost,
                                       "note": "NOT a GPU number: leaves per transition and tau from the NumPy model"}
for k, v in out.items():
    if isinstance(v, dict) and "tau" in v:
        v["gradient_evaluations_per_independent_sample"] = max(v["tau"], 1.0) * v["evaluations_per_step"] if k != "stretch" else None
        v["kernel_sums_per_independent_sample"] = max(v["tau"], 1.0) * v["evaluations_per_step"] * v["cost_factor"]
for k, v in out.items():
    if isinstance(v, dict) and "tau" in v:
        v["fewer_kernel_sums_than_stretch"] = out["stretch"]["kernel_sums_per_independent_sample"] / v["kernel_sums_per_independent_sample"]
print(json.dumps(out, indent=1))
