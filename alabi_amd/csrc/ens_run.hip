// Running a chain on an ensemble handle: alabi_ens_run dispatches on the route of ens_plan.hip to one function per way of
// running (HMC and NUTS chunks, MH chunks, persistent kernel, one launch per half step with graph replay); alabi_ens_draw and
// alabi_ens_half_step* drive single half steps, alabi_ens_restore / alabi_ens_last_state hand back what a persistent call kept.
#include <cmath>
#include <cstring>

#include "gp_device.hpp"

using namespace alabi;

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

namespace alabi {
HalfArgs base_args(alabi_ens* e, double* coords, double* logp) {
    HalfArgs h{};
    alabi_gp* gp = e->gp;
    h.coords = coords; h.logp = logp; h.consts = e->consts;
    h.Xt = gp->Xt; h.alpha = gp->alpha; h.Npad = gp->Npad;
    h.Xc = gp->Xc; h.ens_h = gp->ens_h; h.centre = gp->xa_centre;
    // the affine map of the log-probability folds into the amplitude and the mean: c (amp s + m) + e = (c amp) s + (c m + e)
    h.amp = e->lp_scale * std::exp(gp->log_amp); h.mean = std::fma(e->lp_scale, gp->mean, e->lp_shift); h.kf = gp->kf;
    h.W = e->W; h.d = e->d; h.n0 = (e->W + 1) / 2;
    h.thin_by = 1; h.run_state = e->run_state;
    h.has_prior = e->has_prior; h.prior_const = e->prior_const; h.ymap = e->ymap;
    return h;
}

int alabi_ens_half_step_hist(alabi_ens* e, const double* coords, const double* logp, int t, int split, int part_begin, int part_end,
                             const double* shist, double* out, const EnsSwitches& sw, hipStream_t s) {
    if (!e || t < 0 || t >= e->drawn_n || e->E != 1 || !shist || !out || e->has_de) return ALABI_BAD_ARGUMENT;
    int st = ens_sync_consts(e, s);
    if (st != ALABI_OK) return st;
    HalfArgs h = base_args(e, const_cast<double*>(coords), const_cast<double*>(logp));
    h.rec = offset_draws(e->draws, (size_t)t * e->W);
    h.local_t = t; h.split = split; h.part_begin = part_begin;
    h.shist = shist; h.sout = out;
    return launch_ens_half_args(e, h, part_end - part_begin, sw, s);
}
}  // namespace alabi

namespace {

// The arguments of alabi_ens_run, as every way of running takes them
struct RunCall {
    double *coords, *logp;
    long long step0, nsteps;
    int thin_by;
    double a;
    double *chain, *chain_logp;
    long long* n_accept;
    hipStream_t s;
};

int set_run_state(alabi_ens* e, long long step0, long long done, hipStream_t s) {
    long long host[2] = {step0, done};
    ALABI_HIP_CHECK(hipMemcpyAsync(e->run_state, host, sizeof(host), hipMemcpyHostToDevice, s));
    ALABI_HIP_CHECK(hipStreamSynchronize(s));  // `host` is a stack buffer
    return ALABI_OK;
}

// enqueue `n` steps that consume the chunk buffers (draw + 2n half steps + advance)
int enqueue_chunk(alabi_ens* e, HalfArgs h, int n, double a, const EnsSwitches& sw, hipStream_t s) {
    int st;
    if ((st = launch_ens_draw(e, n, a, s)) != ALABI_OK) return st;
    const int n0 = h.n0, n1 = e->W - n0;
    const size_t WT = (size_t)e->W * e->E;
    for (int t = 0; t < n; ++t) {
        h.rec = offset_draws(e->draws, (size_t)t * WT);
        set_move_args(e, h, (size_t)t);
        h.local_t = t; h.part_begin = 0;
        h.split = 0;
        if (e->has_kde && (st = launch_ens_kde_prepass(e, h, s)) != ALABI_OK) return st;
        if ((st = launch_ens_half_args(e, h, n0, sw, s)) != ALABI_OK) return st;
        h.split = 1;
        if (e->has_kde && n1 > 0 && (st = launch_ens_kde_prepass(e, h, s)) != ALABI_OK) return st;
        if ((st = launch_ens_half_args(e, h, n1, sw, s)) != ALABI_OK) return st;
    }
    return launch_ens_advance(e, n, s);
}

// (coords, logp, n_accept) <- what ens_call_prologue_kernel saved at the start of the last persistent call
int ens_restore(alabi_ens* e, double* coords, double* logp, long long* n_accept, hipStream_t s) {
    if (!e->save || !e->save_valid) return ALABI_NOT_COMPUTED;
    const size_t WT = (size_t)e->W * e->E;
    const double* sv = e->save;
    ALABI_HIP_CHECK(hipMemcpyAsync(coords, sv, WT * e->d * sizeof(double), hipMemcpyDeviceToDevice, s));
    ALABI_HIP_CHECK(hipMemcpyAsync(logp, sv + WT * e->d, WT * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (n_accept && e->save_accept)
        ALABI_HIP_CHECK(hipMemcpyAsync(n_accept, sv + WT * (e->d + 1), WT * sizeof(long long), hipMemcpyDeviceToDevice, s));
    return ALABI_OK;
}

// ---- path 5.  An all-HMC set: every step of a chunk in one launch of ens_hmc_kernel.
int run_hmc_chunks(alabi_ens* e, const RunCall& c, int chunk) {
    int st;
    for (long long done = 0; done < c.nsteps; done += chunk) {
        const int K = (int)(c.nsteps - done < chunk ? c.nsteps - done : chunk);
        if ((st = launch_ens_hmc(e, c.coords, c.logp, c.step0, done, K, c.thin_by, c.chain, c.chain_logp, c.n_accept, 0, 0.0, nullptr, nullptr, c.s)) != ALABI_OK) return st;
    }
    e->hmc_plan[1] = chunk;
    return ALABI_OK;
}

// ---- path 6.  An all-NUTS set: every transition of a chunk in one launch of ens_nuts_kernel.
int run_nuts_chunks(alabi_ens* e, const RunCall& c, int chunk) {
    int st;
    for (long long done = 0; done < c.nsteps; done += chunk) {
        const int K = (int)(c.nsteps - done < chunk ? c.nsteps - done : chunk);
        if ((st = launch_ens_nuts(e, c.coords, c.logp, c.step0, done, K, c.thin_by, c.chain, c.chain_logp, c.n_accept, nullptr, c.s)) != ALABI_OK) return st;
    }
    e->nuts_plan[1] = chunk;
    return ALABI_OK;
}

// ---- path 4.  An all-Gaussian set: W independent chains, one workgroup per walker, every step of a chunk in one launch
// (ens_mh_kernel).  The step counters travel by value; nothing is read back.
int run_mh_chunks(alabi_ens* e, const RunCall& c, int chunk) {
    int st;
    for (long long done = 0; done < c.nsteps; done += chunk) {
        const int K = (int)(c.nsteps - done < chunk ? c.nsteps - done : chunk);
        if ((st = launch_ens_mh(e, c.coords, c.logp, c.step0, done, K, c.thin_by, c.chain, c.chain_logp, c.n_accept, c.s)) != ALABI_OK) return st;
    }
    e->mh_plan[1] = chunk;
    return ALABI_OK;
}

// ---- paths 1 and 3: the persistent kernels

// Clean-row accounting of a persistent call.  The history (and the pair kernel's prop) is trusted to hold the sentinel only in the
// rows this handle's last use of it left so: a stream call that ended without a time-out.  The counts are taken at the start of
// the call and zeroed on the handle, so a call that fails on the way leaves everything dirty; rows 1..need are polled by this call.
struct CleanRows {
    int hist, prop;     // clean rows the call found
    bool pair;
    CleanRows(alabi_ens* e, bool use_pair) : hist(e->hist_clean), prop(use_pair ? e->prop_clean : 0), pair(use_pair) {
        e->hist_clean = 0;
        if (use_pair) e->prop_clean = 0;
    }
    // rows the call's first chunk refills in front of its persistent kernel (0: none)
    int hist_fill(long long done, int need) const { return (done == 0 && hist < need) ? need : 0; }
    int prop_fill(long long done, int need) const { return (done == 0 && prop < need) ? need : 0; }
    // after the read-back: the epilogues put the sentinel back unless the call timed out (flag) or ran on the group kernel
    void settle(alabi_ens* e, bool use_group, int flag, int need) const {
        e->hist_clean = (!use_group && !flag) ? (hist > need ? hist : need) : 0;
        if (pair) e->prop_clean = !flag ? (prop > need ? prop : need) : 0;
    }
};

// Draw-ahead protocol of ens_stream_kernel / ens_pair_kernel.  The draws depend on nothing but the step counter.  In a call of
// several chunks those of the next chunk are made on the side stream while this chunk's persistent kernel runs (it occupies half
// of the CUs), into the buffer set the previous chunk has released; behind the call's last persistent kernel the same is done for
// the first chunk of the NEXT call, which by then finds them in draws2 if it continues where this one ends (step, a, move table).
// Two events order the streams: ev_free (main -> side: the buffer is no longer read), ev_drawn (side -> main: the draws are there).
// Pair kernel with placement: every chunk's records go through ens_place_kernel right behind their draws, on the stream that drew them.
struct DrawAhead {
    alabi_ens* e;
    const RunCall& c;
    bool two_sets;      // the second buffer set, the side stream and the events exist
    bool place;
    bool issued = false;   // the current chunk's records were drawn on the side stream during the previous chunk

    // start of the call: do the records drawn behind the last call fit this one (hit)?  If not, the first chunk's are drawn here.
    int begin(int need) {
        const bool hit = two_sets && e->ahead_valid && e->ahead_step == c.step0 && e->ahead_a == c.a && e->ahead_moves_gen == e->moves_gen &&
                         need <= e->ahead_n;
        // hit or not, the main stream goes on behind the pending launch of the side stream: draws2 is never written from two streams
        if (e->ahead_pending) ALABI_HIP_CHECK(hipStreamWaitEvent(c.s, e->ev_drawn, 0));
        e->ahead_pending = false; e->ahead_valid = false;
        e->draw_set = hit ? 1 : 0;
        e->boundary_stats[hit ? 0 : 1]++;
        int st;
        if (!hit && (st = launch_ens_draw_at(e, e->draws, need, c.a, false, c.step0, c.s)) != ALABI_OK) return st;
        if (place && !(hit && e->ahead_placed) && (st = launch_ens_place(e, hit ? e->draws2 : e->draws, need, true, c.s)) != ALABI_OK) return st;
        return ALABI_OK;
    }
    DrawBuffers& current() const { return e->draw_set ? e->draws2 : e->draws; }
    // in front of a chunk's persistent kernel: its records are in current() -- drawn ahead, by begin(), or here
    int records(long long done, int K, bool last) {
        int st;
        if (issued) ALABI_HIP_CHECK(hipStreamWaitEvent(c.s, e->ev_drawn, 0));
        else if (done > 0) {
            if ((st = launch_ens_draw_at(e, current(), K, c.a, false, c.step0 + done, c.s)) != ALABI_OK) return st;
            if (place && (st = launch_ens_place(e, current(), K, true, c.s)) != ALABI_OK) return st;
        }
        issued = false;
        // everything that read the other buffer set is behind this point.  The draws for the next call go into draws2
        // whichever set this chunk reads, and start behind its persistent kernel, not beside it
        if (two_sets && !last) ALABI_HIP_CHECK(hipEventRecord(e->ev_free, c.s));
        return ALABI_OK;
    }
    // behind the launch of a chunk's persistent kernel: the next chunk's draws, or (last) those of the next call's first chunk
    int ahead(long long done, int K, bool last) {
        if (!two_sets) return ALABI_OK;
        int st;
        if (last) ALABI_HIP_CHECK(hipEventRecord(e->ev_free, c.s));
        const long long rem2 = c.nsteps - done - K;
        const int K2 = last ? e->chunk_cap : (int)(rem2 < e->chunk_cap ? rem2 : e->chunk_cap);
        ALABI_HIP_CHECK(hipStreamWaitEvent(e->side_stream, e->ev_free, 0));
        DrawBuffers& into = (last || e->draw_set == 0) ? e->draws2 : e->draws;
        if ((st = launch_ens_draw_at(e, into, K2, c.a, false, c.step0 + done + K, e->side_stream)) != ALABI_OK) return st;
        if (place && (st = launch_ens_place(e, into, K2, !last, e->side_stream)) != ALABI_OK) return st;
        ALABI_HIP_CHECK(hipEventRecord(e->ev_drawn, e->side_stream));
        if (last) {
            e->ahead_pending = true; e->ahead_valid = true;
            e->ahead_step = c.step0 + c.nsteps; e->ahead_a = c.a; e->ahead_moves_gen = e->moves_gen; e->ahead_n = K2;
            e->ahead_placed = place;
        } else {
            issued = true;
        }
        return ALABI_OK;
    }
    void next_chunk() { if (two_sets) e->draw_set ^= 1; }
};

// Persistent dataflow path: training set pinned in registers (Npad <= 2048: 256 compute lanes x up to 4 point pairs), one
// workgroup per list position -- or ens_group_kernel (use_group).  It synchronises at the end to read the time-out flag and
// returns ALABI_TIMEOUT when it is set.
// ens_stream_kernel's chunks take the step counters by value and their epilogue leaves run_state as the other paths
// would (no upload, no host synchronisation in front of the first launch).
int run_persistent(alabi_ens* e, const RunCall& c, bool use_group, bool allow_pair, const EnsRoute& route, const EnsSwitches& sw) {
    hipStream_t s = c.s;
    int st;
    const int need = (int)(c.nsteps < e->chunk_cap ? c.nsteps : e->chunk_cap);   // rows 1..need are polled by this call
    // Two workgroups per list position (ens_pair_kernel) where 2 ceil(W/2) E of them fit one per CU.  That leaves no spare CU, so
    // a time-out of the pair variant is retried by alabi_ens_run on ens_stream_kernel, from the walkers saved here, before it is reported.
    const bool use_pair = !use_group && allow_pair && ens_pair_ready(e, route.pair);
    e->last_variant = use_pair ? 1 : 0;
    const CleanRows clean(e, use_pair);
    if (use_group && (st = set_run_state(e, c.step0, 0, s)) != ALABI_OK) return st;
    // A time-out's second run is on ens_stream_kernel and reads the records as they were drawn.
    DrawAhead draws{e, c, !use_group && ens_draw_ahead_ready(e), use_pair && ens_place_ready(e, route.place)};
    if (!use_group && (st = draws.begin(need)) != ALABI_OK) return st;
    // one launch: the walkers saved (a time-out is repeated from there), the flag cleared, row 0 of the history
    if ((st = launch_ens_call_prologue(e, c.coords, c.logp, c.n_accept, !use_group, s)) != ALABI_OK) return st;
    for (long long done = 0; done < c.nsteps;) {
        const long long remaining = c.nsteps - done;
        const int K = (int)(remaining < e->chunk_cap ? remaining : e->chunk_cap);
        if (use_group) {
            if ((st = launch_ens_draw(e, K, c.a, s)) != ALABI_OK) return st;
            if ((st = launch_ens_group(e, c.coords, c.logp, K, c.thin_by, c.chain, c.chain_logp, c.n_accept, sw, s)) != ALABI_OK) return st;
            if ((st = launch_ens_advance(e, K, s)) != ALABI_OK) return st;
        } else {
            const bool last = remaining == K;
            if ((st = draws.records(done, K, last)) != ALABI_OK) return st;
            const DrawBuffers& cur = draws.current();
            if ((st = use_pair ? launch_ens_pair_kernel(e, cur, K, clean.hist_fill(done, need), clean.prop_fill(done, need), draws.place, sw, s)
                               : launch_ens_stream_kernel(e, cur, K, clean.hist_fill(done, need), sw, s)) != ALABI_OK)
                return st;
            if ((st = draws.ahead(done, K, last)) != ALABI_OK) return st;
            if ((st = launch_ens_stream_epilogue(e, c.coords, c.logp, K, c.thin_by, c.chain, c.chain_logp, c.n_accept, c.step0 + done + K, done,
                                                 use_pair, last, s)) != ALABI_OK)
                return st;
            draws.next_chunk();
        }
        done += K;
    }
    // one read-back: the flag and, on ens_stream_kernel / ens_pair_kernel, the walkers the last epilogue left beside it
    const size_t WTs = (size_t)e->W * e->E;
    const size_t back = use_group ? sizeof(unsigned long long) : (1 + WTs * (e->d + 1)) * sizeof(unsigned long long);
    ALABI_HIP_CHECK(hipMemcpyAsync(e->state_host, e->state_dev, back, hipMemcpyDeviceToHost, s));
    ALABI_HIP_CHECK(hipStreamSynchronize(s));
    const int flag = *reinterpret_cast<const int*>(e->state_host);
    clean.settle(e, use_group, flag, need);
    e->last_state_ok = !use_group && !flag;
    if (flag) e->ahead_valid = false;             // (the launch stays pending: the next call waits for it before it draws)
    return flag ? ALABI_TIMEOUT : ALABI_OK;
}

// ---- path 0: one launch per half step; a call of at least two chunks of graph_steps replays a captured chunk.
// The graph key does not hold ALABI_ENS_MULTI: a cached graph keeps the proposals per workgroup it was captured with.
int run_half_steps(alabi_ens* e, const RunCall& c, const EnsRoute& route, const EnsSwitches& sw) {
    hipStream_t s = c.s;
    int st;
    if ((st = set_run_state(e, c.step0, 0, s)) != ALABI_OK) return st;
    HalfArgs h = base_args(e, c.coords, c.logp);
    h.chain = c.chain; h.chain_logp = c.chain_logp; h.n_accept = c.n_accept; h.thin_by = c.thin_by;
    const int gsteps = route.graph_steps;
    long long remaining = c.nsteps;
    if (route.graph && remaining >= 2LL * gsteps) {
        alabi_ens::GraphKey key{c.coords, c.logp, c.chain, c.chain_logp, c.n_accept, c.thin_by, gsteps, c.a, e->gp->gen};
        const bool same = e->graph_exec && memcmp(&key, &e->graph_key, sizeof(key)) == 0;
        if (!same) {
            if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }
            hipGraph_t graph = nullptr;
            ALABI_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            st = enqueue_chunk(e, h, gsteps, c.a, sw, s);
            hipError_t ce = hipStreamEndCapture(s, &graph);
            if (st != ALABI_OK) { if (graph) (void)hipGraphDestroy(graph); return st; }
            if (ce != hipSuccess) return hip_fail(ce, "hipStreamEndCapture", __FILE__, __LINE__);
            hipError_t ie = hipGraphInstantiate(&e->graph_exec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (ie != hipSuccess) { e->graph_exec = nullptr; return hip_fail(ie, "hipGraphInstantiate", __FILE__, __LINE__); }
            e->graph_key = key;
            e->graph_steps = gsteps;
        }
        while (remaining >= gsteps) {
            ALABI_HIP_CHECK(hipGraphLaunch(e->graph_exec, s));
            remaining -= gsteps;
        }
    }
    while (remaining > 0) {
        const int n = (int)(remaining < e->chunk_cap ? remaining : e->chunk_cap);
        if ((st = enqueue_chunk(e, h, n, c.a, sw, s)) != ALABI_OK) return st;
        remaining -= n;
    }
    return ALABI_OK;
}

}  // namespace

extern "C" {

int alabi_ens_restore(alabi_ens* e, double* coords, double* logp, long long* n_accept, void* stream) {
    if (!e || !coords || !logp) return ALABI_BAD_ARGUMENT;
    return ens_restore(e, coords, logp, n_accept, as_stream(stream));
}

int alabi_ens_last_state(alabi_ens* e, double* coords_out, double* logp_out) {
    if (!e || !coords_out || !logp_out) return ALABI_BAD_ARGUMENT;
    if (!e->last_state_ok || !e->state_host) return ALABI_NOT_COMPUTED;
    const size_t WT = (size_t)e->W * e->E;
    memcpy(coords_out, e->state_host + 1, WT * e->d * sizeof(double));
    memcpy(logp_out, e->state_host + 1 + WT * e->d, WT * sizeof(double));
    return ALABI_OK;
}

int alabi_ens_run(alabi_ens* e, double* coords, double* logp, long long step0, long long nsteps, int thin_by,
                  double a, double* chain, double* chain_logp, long long* n_accept, void* stream) {
    if (!e || !coords || !logp || nsteps < 0 || thin_by < 1 || !(a > 1.0)) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    if (nsteps == 0) return ALABI_OK;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = ens_sync_consts(e, s)) != ALABI_OK) return st;
    const RunCall c{coords, logp, step0, nsteps, thin_by, a, chain, chain_logp, n_accept, s};
    const EnsSwitches sw = ens_switches();
    const EnsShape sh = ens_shape(e, s != nullptr);
    EnsRoute route = ens_route(sh, e->n_cu, sw);
    // the plan wants the group kernel; whether its hand-off buffers can be had is the launcher's to say
    if (route.path == 3 && !ens_group_buffers(e, sw, s)) route = ens_route(sh, e->n_cu, sw, false);
    if (route.path < 0) return ALABI_BAD_ARGUMENT;
    e->last_path = route.path;
    e->last_state_ok = false;
    switch (route.path) {
        case 6: return run_nuts_chunks(e, c, route.chunk);
        case 5: return run_hmc_chunks(e, c, route.chunk);
        case 4: return run_mh_chunks(e, c, route.chunk);
        case 3: return run_persistent(e, c, true, false, route, sw);
        case 1:
            st = run_persistent(e, c, false, true, route, sw);
            if (st != ALABI_TIMEOUT || e->last_variant != 1) return st;
            // a time-out of the pair kernel: restore the walkers, turn the pair variant off for this handle and run the call again on
            // ens_stream_kernel (the history is marked dirty, the flag is cleared at the start of the run); a second time-out is reported
            if ((st = ens_restore(e, coords, logp, n_accept, s)) != ALABI_OK) return st;
            e->pair_state = -1;
            return run_persistent(e, c, false, false, route, sw);
        default: return run_half_steps(e, c, route, sw);
    }
}

int alabi_ens_hmc_adapt(alabi_ens* e, double* coords, double* logp, long long step0, long long nsteps, int thin_by, double* da_state,
                        const double* da_par, double* chain, double* chain_logp, long long* n_accept, double* accept_stat, void* stream) {
    if (!e || !coords || !logp || !da_state || !da_par || nsteps < 0 || thin_by < 1) return ALABI_BAD_ARGUMENT;
    const double delta = da_par[0], gamma = da_par[1], t0 = da_par[2], kappa = da_par[3];
    if (!(delta > 0.0 && delta < 1.0) || !(gamma > 0.0) || !(t0 >= 0.0) || !std::isfinite(t0) || !(kappa > 0.5 && kappa <= 1.0))
        return ALABI_BAD_ARGUMENT;                                    // (gamma = +inf is allowed: ln e stays at mu)
    if (!e->all_hmc || e->moves.n != 1) return ALABI_BAD_ARGUMENT;    // one step size is adapted: exactly one kind-6 move
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    const int chunk = ens_hmc_chunk(ens_shape(e, s != nullptr), e->n_cu, ens_switches());
    if (chunk <= 0) return ALABI_BAD_ARGUMENT;                        // the factor and the weights exceed the LDS, or no dimension bucket
    if (nsteps == 0) return ALABI_OK;
    int st;
    if ((st = ens_sync_consts(e, s)) != ALABI_OK) return st;
    for (long long done = 0; done < nsteps; done += chunk) {
        const int K = (int)(nsteps - done < chunk ? nsteps - done : chunk);
        if ((st = launch_ens_hmc_adapt(e, coords, logp, step0, done, K, thin_by, chain, chain_logp, n_accept, da_state, da_par, accept_stat, s)) != ALABI_OK)
            return st;
    }
    e->hmc_plan[1] = chunk;
    return ALABI_OK;
}

int alabi_ens_nuts_adapt(alabi_ens* e, double* coords, double* logp, long long step0, long long nsteps, int thin_by, double* da_state,
                         const double* da_par, double* chain, double* chain_logp, long long* n_accept, long long* counts, double* accept_sum,
                         double* accept_stat, void* stream) {
    if (!e || !coords || !logp || !da_state || !da_par || nsteps < 0 || thin_by < 1) return ALABI_BAD_ARGUMENT;
    const double delta = da_par[0], gamma = da_par[1], t0 = da_par[2], kappa = da_par[3];
    if (!(delta > 0.0 && delta < 1.0) || !(gamma > 0.0) || !(t0 >= 0.0) || !std::isfinite(t0) || !(kappa > 0.5 && kappa <= 1.0))
        return ALABI_BAD_ARGUMENT;                                    // (gamma = +inf is allowed: ln e stays at mu)
    if (!e->all_nuts || e->moves.n != 1) return ALABI_BAD_ARGUMENT;   // one step size is adapted: exactly one kind-7 move
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    const int chunk = ens_nuts_chunk(ens_shape(e, s != nullptr), e->n_cu, ens_switches());
    if (chunk <= 0) return ALABI_BAD_ARGUMENT;                        // factor, weights and checkpoints exceed the LDS, or no dimension bucket
    if (nsteps == 0) return ALABI_OK;
    int st;
    if ((st = ens_sync_consts(e, s)) != ALABI_OK) return st;
    for (long long done = 0; done < nsteps; done += chunk) {
        const int K = (int)(nsteps - done < chunk ? nsteps - done : chunk);
        if ((st = launch_ens_nuts_adapt(e, coords, logp, step0, done, K, thin_by, chain, chain_logp, n_accept, da_state, da_par, counts,
                                        accept_sum, accept_stat, s)) != ALABI_OK)
            return st;
    }
    e->nuts_plan[1] = chunk;
    return ALABI_OK;
}

int alabi_ens_find_step_size(alabi_ens* e, const double* coords, const double* logp, long long step, int k_move, double* ln_e, int* iters,
                             void* stream) {
    if (!e || !coords || !logp || !ln_e) return ALABI_BAD_ARGUMENT;
    if (!(e->all_hmc || e->all_nuts) || k_move < 0 || k_move >= e->moves.n) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = ens_sync_consts(e, s)) != ALABI_OK) return st;
    return launch_ens_step_search(e, coords, logp, step, k_move, ln_e, iters, s);
}

int alabi_ens_draw(alabi_ens* e, long long step0, int nsteps, double a, void* stream) {
    if (!e || nsteps <= 0 || nsteps > e->chunk_cap || !(a > 1.0)) return ALABI_BAD_ARGUMENT;
    if (e->W < 2 && !e->all_gauss && !e->all_nuts) return ALABI_BAD_ARGUMENT;   // a red-blue record names a walker of the other half
    if (e->all_hmc || e->all_nuts) return ALABI_BAD_ARGUMENT;         // an HMC or NUTS step has no record: its draws are made where it runs
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = set_run_state(e, step0, 0, s)) != ALABI_OK) return st;
    e->drawn_n = nsteps;
    return launch_ens_draw(e, nsteps, a, s);
}

int alabi_ens_half_step(alabi_ens* e, double* coords, double* logp, int t, int split, int part_begin, int part_end,
                        long long* n_accept, void* stream) {
    if (!e || !coords || !logp || t < 0 || t >= e->drawn_n || (split != 0 && split != 1) || e->E != 1)
        return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    int st = ens_sync_consts(e, as_stream(stream));
    if (st != ALABI_OK) return st;
    HalfArgs h = base_args(e, coords, logp);
    const int nS = split == 0 ? h.n0 : e->W - h.n0;
    if (part_begin < 0 || part_end > nS || part_begin > part_end) return ALABI_BAD_ARGUMENT;
    h.rec = offset_draws(e->draws, (size_t)t * e->W);
    set_move_args(e, h, (size_t)t);
    h.local_t = t; h.split = split; h.part_begin = part_begin; h.n_accept = n_accept;
    if (e->has_kde && part_end > part_begin && (st = launch_ens_kde_prepass(e, h, as_stream(stream))) != ALABI_OK) return st;
    return launch_ens_half_args(e, h, part_end - part_begin, ens_switches(), as_stream(stream));
}

}  // extern "C"
