"""Nested sampling measurements (DESIGN.md "Nested sampling"): ns_walk_kernel per step at N=2000, d=10 for K = 64 / 256 / 1024
walks against the ensemble's per-step time, and run_dynesty end to end at the tutorial's settings and at C3 size, with a
reference-shaped CPU leg (one oracle predict per likelihood call, as dynesty calls the reference's surrogate).

    python tools/prof_nested.py            # everything, one JSON line per measurement
    python tools/prof_nested.py walk       # only the walk kernel (the part to run under rocprofv3 --kernel-trace --stats)
    python tools/prof_nested.py slice      # ns_slice_kernel beside ns_walk_kernel (alternating, same process) at d = 10 and 24,
                                           # and run_dynesty at C3 size with sample="rwalk" / "rslice"
    python tools/prof_nested.py --normal   # Gaussian priors: the walk and the slice kernel at N = 2000, d = 10, K = 64 / 256 with the
                                           # uniform map and with a normal prior on every coordinate, three rounds each (the
                                           # uniform rows also run on a tree without the feature, for a before / after), and the
                                           # tutorial-sized run_dynesty with prior_transform_normal fused / as a host callable
    python tools/prof_nested.py --unif     # uniform draws in bounding ellipsoids (run_pymultinest's move): HIP-event time of one draw +
                                           # select launch pair at M = 256 / 1024 / 4096 candidates for N = 2000, d = 10 and N = 200,
                                           # d = 2; wall time, ncall, evals_launched and evaluations per dead point of the tutorial
                                           # setting and of C3 size with sample="unif" beside sample="rwalk" on the same build.
                                           # Writes profiles/nested_unif.txt as well.
    python tools/prof_nested.py --mlf      # the MLFriends region (run_ultranest's move): HIP-event time of ns_mlf_radius_kernel (30
                                           # rounds) and of one ns_mlf_draw_kernel + select pair beside the ns_unif_draw_kernel +
                                           # select pair, in turn on the same build, at (N, d) = (2000, 10) and (200, 2) with 400
                                           # live points; run_ultranest beside run_pymultinest end to end on the 2-D Rosenbrock
                                           # surrogate.  Writes profiles/nested_mlfriends.txt as well.
"""
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from conftest import make_problem  # noqa: E402


_SINK = None


def emit(**kw):
    print(json.dumps(kw), flush=True)
    if _SINK is not None:
        _SINK.write(json.dumps(kw) + "\n")
        _SINK.flush()


def walk_kernel():
    from alabi_amd import EnsembleSampler, HipGP
    from alabi_amd.nested import GPUWalkBackend
    N, d, walks = 2000, 10, 25
    X, y, h = make_problem(N, d, 0)
    g = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"])
    g.compute(X)
    box = np.array([[-3.0, 3.0]] * d)
    be = GPUWalkBackend(g, y, box, seed=1, to_theta=lambda u: u)
    u, l = be.prior(0, 4096)
    lstar = float(np.quantile(l, 0.5))
    keep = np.flatnonzero(l > lstar)
    chol = np.linalg.cholesky(np.cov(u.T))
    flop_eval = N * (2 * d + 33)          # per GP mean: d fma + ~33 fp64 ops of exp / sign per training point (se_pair_terms)
    for K in (64, 256, 1024):
        idx = keep[np.arange(K) % len(keep)]
        u0 = torch.as_tensor(u[idx], device="cuda")
        l0 = torch.as_tensor(l[idx], device="cuda")
        ch = torch.as_tensor(chol, device="cuda")
        uo, lo = torch.empty_like(u0), torch.empty_like(l0)
        nacc = torch.zeros(2 * K, dtype=torch.int32, device="cuda")
        from alabi_amd import _lib
        lib, ns, st = _lib.lib(), be._ensure(), _lib.current_stream()

        def once(call):
            _lib.check(lib.alabi_ns_walk(ns, call, 0, _lib.ptr(u0), _lib.ptr(l0), K, lstar, _lib.ptr(ch), 0.5, walks,
                                         _lib.ptr(uo), _lib.ptr(lo), _lib.ptr(nacc), st), "alabi_ns_walk")
        for i in range(3):
            once(i)
        torch.cuda.synchronize()
        reps = 20
        t0 = time.perf_counter()
        for i in range(reps):
            once(100 + i)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        evals = float(nacc[K:].sum().item())
        emit(what="ns_walk", N=N, d=d, K=K, walks=walks, path=be.last_path(), us_per_launch=dt * 1e6,
             us_per_step=dt * 1e6 / walks, walk_steps_per_s=K * walks / dt, evals_last_launch=evals,
             gflops_wall=evals * flop_eval / dt / 1e9)
    # the ensemble at the same GP: time per step and per proposal
    W, steps = 256, 400
    s = EnsembleSampler(W, d, g, y, box, seed=3)
    p0 = np.random.RandomState(0).uniform(-1, 1, (W, d))
    s.run_mcmc(p0, 50)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.run_mcmc(s.get_last_sample().coords, steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    emit(what="ensemble_reference_point", N=N, d=d, W=W, us_per_step=dt / steps * 1e6, us_per_half_step=dt / steps / 2 * 1e6,
         proposals_per_s=W * steps / dt)
    be.close()


def slice_kernel(N, d, rounds=3, reps=10):
    """ns_slice_kernel and ns_walk_kernel in turn, `rounds` times each per K: the spread of the walk figure over the rounds is the
    margin for comparing the slice kernel's time per evaluation of its longest walk (the dependent chain) with the walk's per step."""
    from alabi_amd import HipGP, _lib
    from alabi_amd.nested import GPUWalkBackend, default_slices
    walks, slices = 25, default_slices(d)
    X, y, h = make_problem(N, d, 0)
    g = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"])
    g.compute(X)
    box = np.array([[-3.0, 3.0]] * d)
    be = GPUWalkBackend(g, y, box, seed=1, to_theta=lambda u: u)
    u, l = be.prior(0, 4096)
    lstar = float(np.quantile(l, 0.5))
    keep = np.flatnonzero(l > lstar)
    chol = np.linalg.cholesky(np.cov(u.T))
    lib, ns, st = _lib.lib(), be._ensure(), _lib.current_stream()
    for K in (64, 256, 1024):
        idx = keep[np.arange(K) % len(keep)]
        u0 = torch.as_tensor(u[idx], device="cuda")
        l0 = torch.as_tensor(l[idx], device="cuda")
        ch = torch.as_tensor(chol, device="cuda")
        uo, lo = torch.empty_like(u0), torch.empty_like(l0)
        cnt = torch.zeros(4 * K, dtype=torch.int32, device="cuda")

        def walk(call):
            _lib.check(lib.alabi_ns_walk(ns, call, 0, _lib.ptr(u0), _lib.ptr(l0), K, lstar, _lib.ptr(ch), 0.5, walks,
                                         _lib.ptr(uo), _lib.ptr(lo), _lib.ptr(cnt), st), "alabi_ns_walk")

        def slc(call, scale=1.0):
            _lib.check(lib.alabi_ns_slice(ns, call, 0, _lib.ptr(u0), _lib.ptr(l0), K, lstar, _lib.ptr(ch), scale, slices,
                                          _lib.ptr(uo), _lib.ptr(lo), _lib.ptr(cnt), st), "alabi_ns_slice")
        for fn in (walk, slc):                       # warm-up
            fn(1)
            fn(2)
        torch.cuda.synchronize()
        for rnd in range(rounds):
            for name, fn in (("walk", walk), ("slice", slc)):
                evals, longest, dt = 0, 0, 0.0
                for i in range(reps):                # the same calls in every round: the same work, so the rounds compare
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(100 + i)
                    torch.cuda.synchronize()
                    dt += time.perf_counter() - t0
                    c = cnt.cpu().numpy()
                    ev = c[K:2 * K] if name == "walk" else c[:K]
                    evals += int(ev.sum())
                    longest += int(ev.max()) if name == "slice" else walks
                us = dt / reps * 1e6
                emit(what="ns_" + name, N=N, d=d, K=K, round=rnd, path=be.last_path(), us_per_launch=us,
                     steps_or_slices=walks if name == "walk" else slices, evals_per_launch=evals / reps,
                     longest_chain=longest / reps, us_per_link_of_longest_chain=us * reps / longest,
                     mean_over_max_evals=(evals / K) / longest if name == "slice" else None,
                     evals_per_s=evals / dt)
        if K == 64:
            # the same launch at other scales: short axes give many stepping-out links per slice, long ones many shrink draws, so
            # the launch time over (slices, links of the longest walk) separates the cost of setting up a slice from that of a link
            for scale in (0.1, 0.3, 3.0):
                slc(1, scale)
                torch.cuda.synchronize()
                dt, rows = 0.0, []
                for i in range(reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    slc(100 + i, scale)
                    torch.cuda.synchronize()
                    dt += time.perf_counter() - t0
                    rows.append(cnt.cpu().numpy().reshape(4, K).copy())
                c = np.mean(rows, axis=0)
                emit(what="ns_slice_scale_sweep", N=N, d=d, K=K, scale=scale, slices=slices, us_per_launch=dt / reps * 1e6,
                     longest_chain=float(np.mean([r[0].max() for r in rows])), evals_per_walk=float(c[0].mean()),
                     expansions_per_walk=float(c[1].mean()), contractions_per_walk=float(c[2].mean()), capped=float(c[3].sum()))
    be.close()


def normal_prior(N=2000, d=10, rounds=3, reps=10):
    """Per walk step and per link of the longest slice chain, uniform map against a normal prior on all d coordinates, in turn in
    one process; the spread of a row over its rounds is the margin for comparing two rows (or two trees)."""
    import inspect

    from alabi_amd import HipGP, _lib
    from alabi_amd.nested import GPUWalkBackend, default_slices
    walks, slices = 25, default_slices(d)
    X, y, h = make_problem(N, d, 0)
    g = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"])
    g.compute(X)
    box = np.array([[-3.0, 3.0]] * d)
    priors = {"uniform": {}}
    if "normal_prior" in inspect.signature(GPUWalkBackend.__init__).parameters:
        priors["normal"] = {"normal_prior": (np.zeros(d), np.ones(d))}
    lib, st = _lib.lib(), _lib.current_stream()
    for K in (64, 256):
        legs = []
        for prior, kw in priors.items():
            be = GPUWalkBackend(g, y, box, seed=1, to_theta=lambda u: u, **kw)
            u, l = be.prior(0, 4096)
            lstar = float(np.quantile(l, 0.5))
            keep = np.flatnonzero(l > lstar)
            idx = keep[np.arange(K) % len(keep)]
            legs.append(dict(prior=prior, be=be, ns=be._ensure(), lstar=lstar, u0=torch.as_tensor(u[idx], device="cuda"),
                             l0=torch.as_tensor(l[idx], device="cuda"),
                             ch=torch.as_tensor(np.linalg.cholesky(np.cov(u.T)), device="cuda")))
        uo, lo = torch.empty_like(legs[0]["u0"]), torch.empty_like(legs[0]["l0"])
        cnt = torch.zeros(4 * K, dtype=torch.int32, device="cuda")

        def launch(leg, move, call):
            fn, n, name = (lib.alabi_ns_walk, walks, "alabi_ns_walk") if move == "walk" else (lib.alabi_ns_slice, slices, "alabi_ns_slice")
            _lib.check(fn(leg["ns"], call, 0, _lib.ptr(leg["u0"]), _lib.ptr(leg["l0"]), K, leg["lstar"], _lib.ptr(leg["ch"]),
                          0.5 if move == "walk" else 1.0, n, _lib.ptr(uo), _lib.ptr(lo), _lib.ptr(cnt), st), name)
        for leg in legs:
            for move in ("walk", "slice"):
                launch(leg, move, 1)
                launch(leg, move, 2)
        torch.cuda.synchronize()
        for rnd in range(rounds):
            for move in ("walk", "slice"):
                for leg in legs:
                    evals, longest, dt = 0, 0, 0.0
                    for i in range(reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        launch(leg, move, 100 + i)
                        torch.cuda.synchronize()
                        dt += time.perf_counter() - t0
                        c = cnt.cpu().numpy()
                        ev = c[K:2 * K] if move == "walk" else c[:K]
                        evals += int(ev.sum())
                        longest += int(ev.max()) if move == "slice" else walks
                    emit(what="ns_" + move, prior=leg["prior"], N=N, d=d, K=K, round=rnd, path=leg["be"].last_path(),
                         us_per_launch=dt / reps * 1e6, us_per_link_of_longest_chain=dt * 1e6 / longest,
                         evals_per_launch=evals / reps)
        for leg in legs:
            leg["be"].close()


def normal_prior_end_to_end(nlive=100, runs=3):
    """The tutorial-sized run (2-D, dynamic) under a normal prior on theta_2: prior_transform_normal (fused where the tree has it)
    against the same transform written by hand, which is a host callable."""
    import tempfile
    from functools import partial

    from scipy.stats import norm

    from alabi_amd import SurrogateModel
    from alabi_amd import utility as ut
    bounds = [(-4.0, 4.0)] * 2
    sm = SurrogateModel(lnlike_fn=_gauss(2, 0), bounds=bounds, savedir=tempfile.mkdtemp(), verbose=False, random_state=0, cache=False)
    sm.init_samples(ntrain=200)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1)

    def by_hand(u):
        return np.array([-4.0 + 8.0 * u[0], norm.ppf(u[1], 0.0, 1.0)])
    transforms = {"by_hand": by_hand}
    if hasattr(ut, "prior_transform_normal"):
        transforms["prior_transform_normal"] = partial(ut.prior_transform_normal, bounds=bounds, data=[(None, None), (0.0, 1.0)])
    for name, pt in transforms.items():
        for run in range(runs + 1):                               # run 0: warm-up
            t0 = time.perf_counter()
            sm.run_dynesty(prior_transform=pt, mode="dynamic", sampler_kwargs={"nlive": nlive, "seed": 1 + run}, min_ess=0)
            wall = time.perf_counter() - t0
            r = sm.dynesty_results
            if run:
                emit(what="run_dynesty", config="tutorial_normal_prior", transform=name, path=sm.dynesty_path, nlive=nlive, run=run,
                     wall_s=wall, niter=int(r.niter), ncall=int(r.ncall), logz=float(r.logz[-1]), logzerr=float(r.logzerr[-1]))


def end_to_end_moves(d=10, ntrain=2000, nlive=500):
    import tempfile

    from alabi_amd import SurrogateModel
    sm = SurrogateModel(lnlike_fn=_gauss(d, 0), bounds=[(-2.0, 2.0)] * d, savedir=tempfile.mkdtemp(), verbose=False,
                        random_state=0, cache=False)
    sm.init_samples(ntrain=ntrain)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1)
    sm.run_dynesty(mode="static", sampler_kwargs={"nlive": 100, "seed": 1}, run_kwargs={"maxiter": 500}, min_ess=0)   # warm-up
    for sample in ("rwalk", "rslice", "rwalk", "rslice"):
        t0 = time.perf_counter()
        sm.run_dynesty(mode="static", sampler_kwargs={"nlive": nlive, "seed": 2, "sample": sample}, min_ess=0)
        wall = time.perf_counter() - t0
        r = sm.dynesty_results
        emit(what="run_dynesty", config="C3", sample=sample, d=d, N=ntrain, nlive=nlive, wall_s=wall, niter=int(r.niter),
             ncall=int(r.ncall), evals_per_dead_point=r.ncall / r.niter, evals_per_s=r.ncall / wall, logz=float(r.logz[-1]),
             logzerr=float(r.logzerr[-1]), status=r.status, n_stuck=int(r.n_stuck), scale=float(sm.dynesty_sampler.scale))


def unif_kernels(N, d, rounds=3, reps=10):
    """One ns_unif_draw_kernel + ns_unif_select_kernel pair by HIP events, `rounds` times per M; the ellipsoids are the sampler's own
    bounds around the prior draws above the median logL, need = M / 4."""
    from alabi_amd import HipGP, _lib
    from alabi_amd.nested import GPUWalkBackend, bounding_ellipsoids
    X, y, h = make_problem(N, d, 0)
    g = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"])
    g.compute(X)
    box = np.array([[-3.0, 3.0]] * d)
    be = GPUWalkBackend(g, y, box, seed=1, to_theta=lambda u: u)
    u, l = be.prior(0, 4096)
    lstar = float(np.quantile(l, 0.5))
    ells = bounding_ellipsoids(u[l > lstar], "multi")
    lib, ns, st = _lib.lib(), be._ensure(), _lib.current_stream()
    tab = [torch.as_tensor(a, device="cuda") for a in (ells.centres, ells.axes, ells.inv_axes, ells.cum)]
    for M in (256, 1024, 4096):
        need = M // 4
        cu = torch.empty((M, d), dtype=torch.float64, device="cuda")
        cl = torch.empty(M, dtype=torch.float64, device="cuda")
        cs = torch.empty(M, dtype=torch.int32, device="cuda")
        uo = torch.empty((need, d), dtype=torch.float64, device="cuda")
        lo = torch.empty(need, dtype=torch.float64, device="cuda")
        counts = torch.zeros(5, dtype=torch.int32, device="cuda")

        def pair(call):
            _lib.check(lib.alabi_ns_unif_draw(ns, call, 0, M, 1, len(ells), *[_lib.ptr(t) for t in tab], _lib.ptr(cu), _lib.ptr(cl),
                                              _lib.ptr(cs), st), "alabi_ns_unif_draw")
            _lib.check(lib.alabi_ns_unif_select(ns, M, _lib.ptr(cu), _lib.ptr(cl), _lib.ptr(cs), lstar, need, _lib.ptr(uo),
                                                _lib.ptr(lo), _lib.ptr(counts), st), "alabi_ns_unif_select")
        pair(1)
        pair(2)
        torch.cuda.synchronize()
        for rnd in range(rounds):
            ms, ev = 0.0, 0
            for i in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                pair(100 + i)
                b.record()
                torch.cuda.synchronize()
                ms += a.elapsed_time(b)
                ev += int((cs == 2).sum().item())
            c = counts.cpu().numpy()
            emit(what="ns_unif_draw+select", N=N, d=d, M=M, need=need, ellipsoids=len(ells), round=rnd, path=be.last_path(),
                 us_per_pair=ms / reps * 1e3, evals_per_launch=ev / reps, us_per_evaluated_candidate=ms * 1e3 / max(ev, 1),
                 last_counts=[int(v) for v in c])
    be.close()


def unif_end_to_end(name, d, ntrain, nlive, bounds, runs=2):
    """run_pymultinest (sample="unif") beside run_dynesty static with sample="rwalk", same model, same build, alternating."""
    import tempfile

    from alabi_amd import SurrogateModel
    sm = SurrogateModel(lnlike_fn=_gauss(d, 0), bounds=[bounds] * d, savedir=tempfile.mkdtemp(), verbose=False,
                        random_state=0, cache=False)
    sm.init_samples(ntrain=ntrain)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1)
    for run in range(runs + 1):                                   # run 0: warm-up
        t0 = time.perf_counter()
        sm.run_pymultinest(sampler_kwargs={"n_live_points": nlive, "seed": 1 + run}, min_ess=0)
        wall = time.perf_counter() - t0
        r, s = sm.pymultinest_results, sm.pymultinest_sampler
        if run:
            emit(what="run_pymultinest", config=name, sample="unif", d=d, N=ntrain, nlive=nlive, run=run, wall_s=wall,
                 niter=int(r.niter), ncall=int(r.ncall), evals_launched=int(s.backend.evals_launched),
                 evals_per_dead_point=r.ncall / r.niter, launched_per_dead_point=s.backend.evals_launched / r.niter,
                 max_ellipsoids=int(max(s.n_ellipsoids)), logz=float(r.logz[-1]), logzerr=float(r.logzerr[-1]), status=r.status)
        t0 = time.perf_counter()
        sm.run_dynesty(mode="static", sampler_kwargs={"nlive": nlive, "seed": 1 + run, "sample": "rwalk"}, min_ess=0)
        wall = time.perf_counter() - t0
        r = sm.dynesty_results
        if run:
            emit(what="run_dynesty", config=name, sample="rwalk", d=d, N=ntrain, nlive=nlive, run=run, wall_s=wall,
                 niter=int(r.niter), ncall=int(r.ncall), evals_per_dead_point=r.ncall / r.niter, logz=float(r.logz[-1]),
                 logzerr=float(r.logzerr[-1]), status=r.status)


def mlf_kernels(N, d, nlive=400, B=30, rounds=3, reps=10):
    """ns_mlf_radius_kernel, and the draw + select pair with and without the neighbour test, by HIP events, in turn.  Live points:
    `nlive` of the prior draws above the median logL; r^2 the bootstrapped radius of those points, as the sampler would use."""
    from alabi_amd import HipGP, _lib
    from alabi_amd.nested import GPUWalkBackend, bounding_ellipsoids, mlfriends_metric
    X, y, h = make_problem(N, d, 0)
    g = HipGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"])
    g.compute(X)
    box = np.array([[-3.0, 3.0]] * d)
    be = GPUWalkBackend(g, y, box, seed=1, to_theta=lambda u: u)
    u, l = be.prior(0, 4096)
    lstar = float(np.quantile(l, 0.5))
    live = u[l > lstar][:nlive]
    ells = bounding_ellipsoids(live, "multi")
    _, minv, w = mlfriends_metric(live, ells)
    lib, ns, st = _lib.lib(), be._ensure(), _lib.current_stream()
    tab = [torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in (ells.centres, ells.axes, ells.inv_axes, ells.cum, w, minv)]
    r2d = torch.empty(B, dtype=torch.float64, device="cuda")

    def radius(call):
        _lib.check(lib.alabi_ns_mlf_radius(ns, call, len(w), _lib.ptr(tab[4]), B, _lib.ptr(r2d), st), "alabi_ns_mlf_radius")
    radius(1)
    radius(2)
    torch.cuda.synchronize()
    r2 = float(r2d.max().item())
    for rnd in range(rounds):
        ms = 0.0
        for i in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            radius(100 + i)
            b.record()
            torch.cuda.synchronize()
            ms += a.elapsed_time(b)
        emit(what="ns_mlf_radius", N=N, d=d, nlive=len(w), B=B, round=rnd, us_per_launch=ms / reps * 1e3, r2=r2)
    for M in (256, 1024, 4096):
        need = M // 4
        cu = torch.empty((M, d), dtype=torch.float64, device="cuda")
        cl = torch.empty(M, dtype=torch.float64, device="cuda")
        cs = torch.empty(M, dtype=torch.int32, device="cuda")
        uo = torch.empty((need, d), dtype=torch.float64, device="cuda")
        lo = torch.empty(need, dtype=torch.float64, device="cuda")
        counts = torch.zeros(5, dtype=torch.int32, device="cuda")

        def select():
            _lib.check(lib.alabi_ns_unif_select(ns, M, _lib.ptr(cu), _lib.ptr(cl), _lib.ptr(cs), lstar, need, _lib.ptr(uo),
                                                _lib.ptr(lo), _lib.ptr(counts), st), "alabi_ns_unif_select")

        def unif_pair(call):
            _lib.check(lib.alabi_ns_unif_draw(ns, call, 0, M, 1, len(ells), *[_lib.ptr(t) for t in tab[:4]], _lib.ptr(cu), _lib.ptr(cl),
                                              _lib.ptr(cs), st), "alabi_ns_unif_draw")
            select()

        def mlf_pair(call):
            _lib.check(lib.alabi_ns_mlf_draw(ns, call, 0, M, 1, len(ells), *[_lib.ptr(t) for t in tab[:4]], len(w), _lib.ptr(tab[4]),
                                             _lib.ptr(tab[5]), r2, _lib.ptr(cu), _lib.ptr(cl), _lib.ptr(cs), st), "alabi_ns_mlf_draw")
            select()
        for fn in (unif_pair, mlf_pair):
            fn(1)
            fn(2)
        torch.cuda.synchronize()
        for rnd in range(rounds):
            for name, fn in (("ns_unif_draw+select", unif_pair), ("ns_mlf_draw+select", mlf_pair)):
                ms, ev = 0.0, 0
                for i in range(reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn(100 + i)
                    b.record()
                    torch.cuda.synchronize()
                    ms += a.elapsed_time(b)
                    ev += int((cs == 2).sum().item())
                emit(what=name, N=N, d=d, M=M, need=need, nlive=len(w), ellipsoids=len(ells), round=rnd, path=be.last_path(),
                     us_per_pair=ms / reps * 1e3, evals_per_launch=ev / reps, last_counts=[int(v) for v in counts.cpu().numpy()])
    be.close()


def _rosenbrock(theta):
    t = np.atleast_2d(theta)
    out = -((1.0 - t[:, 0]) ** 2 + 100.0 * (t[:, 1] - t[:, 0] ** 2) ** 2) / 100.0
    return out if np.ndim(theta) == 2 else float(out[0])


def mlf_end_to_end(ntrain=200, nlive=400, runs=3):
    """run_ultranest (static, sample="mlfriends") beside run_pymultinest (sample="unif") on the surrogate of the 2-D Rosenbrock
    likelihood on [-5, 5]^2, same model, same build, alternating, both stopped at dlogz = log1p(0.01)."""
    import tempfile

    from alabi_amd import SurrogateModel
    sm = SurrogateModel(lnlike_fn=_rosenbrock, bounds=[(-5.0, 5.0)] * 2, savedir=tempfile.mkdtemp(), verbose=False, random_state=0,
                        cache=False)
    sm.init_samples(ntrain=ntrain)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1)
    for run in range(runs + 1):                                   # run 0: warm-up
        t0 = time.perf_counter()
        sm.run_ultranest(sampler_kwargs={"seed": 1 + run}, run_kwargs={"min_num_live_points": nlive, "max_num_improvement_loops": 0},
                         min_ess=0)
        wall = time.perf_counter() - t0
        r, s = sm.ultranest_results, sm.ultranest_sampler
        if run:
            emit(what="run_ultranest", config="rosenbrock", sample="mlfriends", N=ntrain, nlive=nlive, run=run, wall_s=wall,
                 niter=int(r.niter), ncall=int(r.ncall), evals_launched=int(s.backend.evals_launched),
                 evals_per_dead_point=r.ncall / r.niter, launched_per_dead_point=s.backend.evals_launched / r.niter,
                 iterations=len(s.radius2), max_ellipsoids=int(max(s.n_ellipsoids)), logz=float(r.logz[-1]),
                 logzerr=float(r.logzerr[-1]), status=r.status)
        t0 = time.perf_counter()
        sm.run_pymultinest(sampler_kwargs={"n_live_points": nlive, "seed": 1 + run, "evidence_tolerance": math.log1p(0.01)}, min_ess=0)
        wall = time.perf_counter() - t0
        r, s = sm.pymultinest_results, sm.pymultinest_sampler
        if run:
            emit(what="run_pymultinest", config="rosenbrock", sample="unif", N=ntrain, nlive=nlive, run=run, wall_s=wall,
                 niter=int(r.niter), ncall=int(r.ncall), evals_launched=int(s.backend.evals_launched),
                 evals_per_dead_point=r.ncall / r.niter, launched_per_dead_point=s.backend.evals_launched / r.niter,
                 iterations=len(s.n_ellipsoids), max_ellipsoids=int(max(s.n_ellipsoids)), logz=float(r.logz[-1]),
                 logzerr=float(r.logzerr[-1]), status=r.status)


def _gauss(d, seed):
    rng = np.random.RandomState(seed)
    A = rng.randn(d, d)
    prec = A @ A.T / d + 0.5 * np.eye(d)

    def like(theta):
        t = np.atleast_2d(theta)
        out = -0.5 * np.einsum("ni,ij,nj->n", t, prec, t)
        return out if np.ndim(theta) == 2 else float(out[0])
    return like


def end_to_end(name, d, ntrain, nlive, mode, bounds):
    import tempfile

    from alabi_amd import SurrogateModel
    from oracle.gp_oracle import OracleGP
    sm = SurrogateModel(lnlike_fn=_gauss(d, 0), bounds=[bounds] * d, savedir=tempfile.mkdtemp(), verbose=False,
                        random_state=0, cache=False)
    sm.init_samples(ntrain=ntrain)
    sm.init_gp(hyperopt_method="ml", gp_nopt=1)
    sm.run_dynesty(mode=mode, sampler_kwargs={"nlive": nlive, "seed": 1}, min_ess=0)     # warm-up (library load, first calls)
    t0 = time.perf_counter()
    sm.run_dynesty(mode=mode, sampler_kwargs={"nlive": nlive, "seed": 2}, min_ess=0)
    wall = time.perf_counter() - t0
    r = sm.dynesty_results
    emit(what="run_dynesty", config=name, d=d, N=ntrain, nlive=nlive, mode=mode, wall_s=wall, niter=int(r.niter),
         nsamples=int(len(r.logl)), ncall=int(r.ncall), evals_per_s=r.ncall / wall, iters_per_s=r.niter / wall,
         logz=float(r.logz[-1]), logzerr=float(r.logzerr[-1]), status=r.status, n_stuck=int(r.n_stuck))
    # reference-shaped CPU leg: dynesty hands the reference's surrogate_log_likelihood ONE point per call
    hp = sm.gp.get_parameter_vector(include_frozen=True)
    o = OracleGP(d, hp[0], hp[1], hp[2], hp[3:]).compute(sm._theta)
    pts = np.random.RandomState(1).uniform(bounds[0], bounds[1], (400, d))
    t0 = time.perf_counter()
    for p in pts:
        o.predict(sm._y, p.reshape(1, -1))
    per = (time.perf_counter() - t0) / len(pts)
    emit(what="cpu_reference_shaped", config=name, N=ntrain, d=d, s_per_eval=per, evals_per_s=1.0 / per,
         est_wall_s_for_same_ncall=per * r.ncall)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    torch.cuda.set_device(0)
    if what in ("--unif", "unif"):
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        _SINK = open(os.path.join(ROOT, "profiles", "nested_unif.txt"), "w")
        _SINK.write("# python tools/prof_nested.py --unif : one JSON line per measurement (times: HIP events for the launch pairs, "
                    "wall clock for the runs)\n")
        unif_kernels(2000, 10)
        unif_kernels(200, 2)
        unif_end_to_end("tutorial", 2, 200, 100, (-4.0, 4.0))
        unif_end_to_end("C3", 10, 2000, 500, (-2.0, 2.0))
        _SINK.close()
    if what in ("--mlf", "mlf"):
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        _SINK = open(os.path.join(ROOT, "profiles", "nested_mlfriends.txt"), "w")
        _SINK.write("# python tools/prof_nested.py --mlf : one JSON line per measurement (times: HIP events for the launches, wall "
                    "clock for the runs)\n")
        mlf_kernels(2000, 10)
        mlf_kernels(200, 2)
        mlf_end_to_end()
        _SINK.close()
    if what in ("--normal", "normal"):
        normal_prior()
        normal_prior_end_to_end()
    if what in ("all", "walk"):
        walk_kernel()
    if what == "slice":
        slice_kernel(2000, 10)
        slice_kernel(2000, 24)
        end_to_end_moves()
    if what in ("all", "e2e"):
        end_to_end("tutorial", 2, 200, 100, "dynamic", (-4.0, 4.0))
        end_to_end("C3", 10, 2000, 500, "static", (-2.0, 2.0))
