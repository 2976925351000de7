// Persistent ensemble kernel ("stream" kernel) for gfx950: ens_stream_kernel, the version history's prologue and epilogue
// kernels and the launches (the fit rule: ens_stream_ppt in ens_plan.hip).  The draws, the records and the launch-per-half-step kernels are in ensemble.hip, the
// pair variant of this kernel in ens_pair.hip, what the two share in ens_stream.hpp.
#include <cstdlib>
#include "ens_stream.hpp"

namespace alabi {

// ---------------------------------------------------------------------------------------------------
// Persistent dataflow variant ("stream" kernel).  One workgroup per list position b (and ensemble) lives for
// K whole steps.  Its share of the training set (2 points x (D + 1) doubles per lane) is loaded ONCE and stays
// in VGPRs, so a proposal costs the distance/exp/reduction only.  There is no barrier between half steps: the
// state of every walker after every step is a row of the version history `hist[v][walker] = (coords, logp)`
// (v = number of steps that walker has completed; immutable once written), and a proposal waits only for the
// two rows it reads -- its own walker at version t and its partner at version t (+1 if the partner belongs to
// the half already updated in this step).  Hand-off follows cdna_hip_programming.md Guideline 16 form R2 (the
// data is the flag): rows of versions 1..K start as a sentinel NaN; every word is written by ONE aligned 8-byte
// write-through store (sc1 = relaxed agent-scope atomic store) and the consumer's lanes poll their own words
// with sc1 loads (L1 bypassed) until none is the sentinel -- no release fence, no drain, no separate flag word.
// Correctness never depends on placement or timing; every spin is bounded
// (a timeout sets *err and every workgroup leaves, the host then falls back to the launch-per-half-step path).
// All workgroups must be co-resident: the host launches at most one per CU.
#ifdef ALABI_STREAM_PROF
__device__ long long g_stream_prof[16];
#endif

// blockDim.x = TMAX = 64 + compute threads (a multiple of 64) + 64.  Three roles, ONE LOOP EACH over the workgroup's proposals;
// the loops meet only at the two barriers of a proposal (A: the proposal is in LDS, B: the wave partials are in LDS), so no role
// carries another role's registers or steps through another role's exec-mask ladders (round 5: the single loop body spilled 12
// SGPRs into VGPR lanes and read several of them back between barrier B and the row store).
//   wave 0          the ONLY wave on the hand-off chain: polls the two rows, forms the proposal, publishes it in LDS,
//                   and after the reduction does the accept test and the one row store.  It computes no kernel values
//                   and issues no other memory operation: gfx950 returns a wave's vector memory operations in issue
//                   order (one vmcnt), so any ordinary load or store would put its latency in front of the next poll.
//                   It takes the abort decision from its own register.  Its loop has no divergent branch and no exit from
//                   inside: either makes the compiler thread the whole loop nest through flag registers and exec-mask
//                   ladders, which then stand on the chain of every half step (tests/test_stream_chain_isa.py counts them).
//   waves 1..nwc    the training-set share of each lane lives in VGPRs for the whole launch; between the two barriers
//                   of a proposal they evaluate the kernel sum and leave one partial per wave in LDS.  The in-bounds flag
//                   sits in the word behind the proposal (qs_s[par][D]): one batch of LDS reads brings both, issued whole
//                   before the flag is tested.
//   last wave       fetches the packed proposal records (one 32-byte load) three proposals ahead into an LDS ring.
// Waves other than wave 0 look at the abort word after barrier B, where they delay nobody.  Every role steps through the
// proposals with the same StreamItems::next, so all waves execute the same number of barriers, early exit included.
// The chain, the thinning and the acceptance counters are NOT written here: every version of every walker is a row of
// `hist` (coords, logp, accepted), and ens_hist_epilogue_kernel copies it out after the launch at HBM speed.
template <int D, int PPT, int TMAX, bool GENERIC>
__global__ void __launch_bounds__(TMAX)
ens_stream_kernel(StreamArgs p) {
    __shared__ __attribute__((aligned(16))) double scratch[2][16];   // wave partials, by proposal parity
    __shared__ unsigned long long rec_s[4][4];                       // proposal-record ring (last wave -> wave 0)
    __shared__ __attribute__((aligned(16))) double qs_s[2][ALABI_MAX_DIM];   // scaled proposal [0, D) and its in-bounds flag [D], by proposal parity
    __shared__ double consts_s[6][ALABI_MAX_DIM];                    // 1/length scale, lower, upper bound, prior mean, prior 1/std, centre
    __shared__ int abort_s;                                          // a bounded spin ran out: written by wave 0 before barrier A
    static_assert(D < ALABI_MAX_DIM && TMAX >= 192 && TMAX % 64 == 0, "ens_stream_kernel: shape");
    constexpr int TC = TMAX - 128, nwc = TC >> 6;                    // the host launches exactly TMAX threads
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);         // wave-uniform: the role branches are scalar
    const bool comm = wv == 0, service = wv == nwc + 1, compute = !comm && !service;
    const int b = blockIdx.x, e = blockIdx.y, E = gridDim.y;
    const int WT = p.W * E, row = p.d + 2;
#ifdef ALABI_STREAM_PROF
    long long prof[5] = {0, 0, 0, 0, 0};
    const long long prof_begin = wall_clock64();
#endif
    f64x2 xa[PPT][D], aa[PPT];
    stream_setup<D, PPT, TC, GENERIC>(p, compute, xa, aa, consts_s, scratch, abort_s);

    // This workgroup's proposals: list positions b, b+G, b+2G, ... of every half step, in (step, split, position)
    // order.  Every dependency points to an EARLIER half step, so the globally oldest unfinished proposal can always
    // run: no deadlock as long as all G x E workgroups are resident.
    const StreamItems items{p, (int)gridDim.x, b};
    // Proposal records depend on nothing: the last wave fetches them three proposals ahead (lane l < 4 loads word l).
    unsigned long long pend = 0;
    int pt = 0, psplit = 0, pbb = b, pslot = 0;
    if (service) {                                    // prologue: items 0 and 1 into the ring, item 2 in flight
        for (int i = 0; i < 2; ++i) {
            const unsigned long long v = stream_record_load(p, E, e, lane, pt, psplit, pbb);
            if (lane < 4) rec_s[pslot & 3][lane] = v;
            items.next(pt, psplit, pbb); ++pslot;
        }
        pend = stream_record_load(p, E, e, lane, pt, psplit, pbb);
    }
    __syncthreads();
    int t = 0, split = 0, bb = b, item = 0;           // b < G <= n0: the first item is valid

    if (comm) {
        // ---- hand-off wave: poll -> proposal -> LDS -> A -> (prior term, reject row, next decode) -> B -> partials -> accept -> store
        // The chain from the arrival of the polled words to barrier A is straight-line code over all 64 lanes: lanes beyond
        // the row poll its last word again (every address is one of the row's own), so no load, test or LDS write needs
        // an exec mask; what those lanes compute is masked out of the in-bounds vote and never read.  While the compute waves
        // work the wave forms everything the accept test does not produce -- the address of the new row, the row as it is
        // written if the proposal is rejected, the accept operands, the next proposal's addresses -- so that behind barrier B
        // only the sum of the partials and the accept test remain.
        const int n0_lane = lane < p.d ? lane : p.d, n1_lane = lane < p.d ? lane : p.d - 1;
        int n_w = 0; double n_zz = 0.0;
        const unsigned long long *n_hw = p.hist, *n_hc = p.hist;
        auto decode_next = [&](int it, int tt, int sp) {
            const unsigned long long* rs = rec_s[it & 3];
            const unsigned long long ids = rs[0];
            n_w = (int)(unsigned)(ids & 0xffffffffull);
            const int cw = (int)(unsigned)(ids >> 32);
            n_zz = __longlong_as_double((long long)rs[1]);
            // own row at version t, partner row at version t (+1 when the partner's half went first)
            n_hw = p.hist + ((size_t)tt * WT + n_w) * row + n0_lane;
            n_hc = p.hist + ((size_t)(tt + sp) * WT + cw) * row + n1_lane;
        };
        const double il_r = consts_s[0][lane], lo_r = consts_s[1][lane], hi_r = consts_s[2][lane], c_r = consts_s[5][lane];
        const bool needc = lane < p.d;
        const unsigned long long coord_lanes = (1ull << p.d) - 1;
        decode_next(0, 0, 0);
        while (t < p.K) {
            const int par = item & 1;
#ifdef ALABI_STREAM_PROF
            const long long c0 = wall_clock64();
#endif
            // The data IS the flag (Guideline 16 form R2): every word of a row is one aligned 8-byte sc1 store
            // over a sentinel NaN that no coordinate or log-probability can equal; lane k polls its own words.
            unsigned long long ws, wc;
            const bool pending = stream_poll(p, [&] {
                ws = ld_sc1(n_hw);
                wc = ld_sc1(n_hc);
                return __builtin_amdgcn_ballot_w64(ws == ALABI_HIST_EMPTY || wc == ALABI_HIST_EMPTY) != 0;
            });
            // Bounded spin ran out: every workgroup leaves, the host falls back.  The cold block rejoins the fast path instead of
            // leaving the loops from inside (exits from a loop nest cost flag registers and ladders on the fast path too): a NaN
            // stretch factor puts the proposal out of bounds, so the compute waves skip it; this is the last proposal, its
            // row is not stored, and the other waves see abort_s behind barrier B.
            if (__builtin_expect(pending, 0)) {
                n_zz = __builtin_nan("");
                abort_s = 1;                          // (every lane writes the same: no divergent branch in this loop)
                __hip_atomic_store(p.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#ifdef ALABI_STREAM_PROF
            const long long c1 = wall_clock64();
#endif
            // lane k < d: coordinate k, lane d: logp
            const double sv = __longlong_as_double((long long)ws), cv = __longlong_as_double((long long)wc);
            const double qv = cv - (cv - sv) * n_zz;
            // one compare mask per bound, tested against the lanes that hold a coordinate
            const bool all_in = (__builtin_amdgcn_ballot_w64(qv > lo_r) & __builtin_amdgcn_ballot_w64(qv < hi_r) & coord_lanes)
                                == coord_lanes;
            double qs = qv * il_r;
            if (!GENERIC) qs -= c_r;
            // The in-bounds flag travels in the word behind the proposal, as the high half of 1.0 or 0.0: a second write, which
            // the LDS performs after the first (lane D wrote 0.0 there), so no select of the flag stands in front of the first.
            // The words behind the flag are never read.
            qs_s[par][lane] = needc ? qs : 0.0;
            reinterpret_cast<int*>(&qs_s[par][D])[1] = all_in ? 0x3ff00000 : 0;
            __syncthreads();                          // barrier A: the proposal is in LDS
            __builtin_amdgcn_sched_barrier(0);        // nothing of the idle window's work in front of it
#ifdef ALABI_STREAM_PROF
            const long long c2 = wall_clock64();
#endif
            // idle until barrier B: everything of the store that does not need the partials, then the next proposal
            int t2 = t, s2 = split, b2 = bb;
            items.next(t2, s2, b2);
            if (pending) t2 = p.K;
            double prior_q = 0.0;                     // normal-prior term of this proposal (0.0 adds exactly nothing)
            if (p.has_prior) {                        // normal_prior_sum with a select for its branch
                const double u = (qv - consts_s[3][lane]) * consts_s[4][lane];
                prior_q = lane_bcast(wave_sum_dpp(needc ? -0.5 * u * u : 0.0), 63) + p.prior_const;
            }
            // this lane's word of the new row; the lanes behind the row write its last word, the acceptance flag, again
            size_t out_word = ((size_t)(t + 1) * WT + n_w) * row + (lane <= p.d ? lane : p.d + 1);
            double lnfac = __longlong_as_double((long long)rec_s[item & 3][2]);
            double lnu = __longlong_as_double((long long)rec_s[item & 3][3]);
            double lp_old = lane_bcast(sv, p.d);      // lane d loaded logp
            // the new row of the walker, lanes k < d coordinates, lane d logp, lane d+1 the acceptance flag: as it is written
            // if the proposal is rejected, and if it is accepted (lane d of that one takes lp_new behind barrier B)
            unsigned long long w_rej = needc ? ws : lane == p.d ? (unsigned long long)__double_as_longlong(lp_old) : 0ull;
            // (an out-of-bounds proposal is rejected whatever the test behind barrier B says: lp_new = -inf fails it)
            unsigned long long w_acc = !all_in ? w_rej : needc ? (unsigned long long)__double_as_longlong(qv) : 1ull;
            const bool takes_lp = all_in && lane == p.d;
            int part = par * (int)sizeof(scratch[0]);
            if (t2 < p.K) decode_next(item + 1, t2, s2);
            // pin the above in front of the barrier: none of it may sink behind it, into the store's exec mask or the next poll
            // (values, not pointers: a pointer that passed through here would lose its address space)
            asm volatile("" : "+v"(out_word), "+v"(w_rej), "+v"(w_acc), "+v"(lp_old), "+v"(lnfac), "+v"(lnu), "+v"(prior_q), "+v"(part));
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();                          // barrier B: the wave partials are in LDS
#ifdef ALABI_STREAM_PROF
            const long long c3 = wall_clock64();
#endif
            const double* partials = reinterpret_cast<const double*>(reinterpret_cast<const char*>(&scratch[0][0]) + part);
            const double lp_new = fma(p.amp, wave_partials_tree<nwc>(partials), p.mean) + prior_q;
            const bool acc = lnfac + lp_new - lp_old > lnu;
            if (takes_lp) w_acc = (unsigned long long)__double_as_longlong(lp_new);
            if (!pending) st_sc1(p.hist + out_word, acc ? w_acc : w_rej);
            t = t2; split = s2; bb = b2; ++item;
#ifdef ALABI_STREAM_PROF
            { const long long c4 = wall_clock64();
              prof[0] += c1 - c0; prof[1] += c2 - c1; prof[2] += c3 - c2; prof[3] += c4 - c3; prof[4] += 1; }
#endif
        }
#ifdef ALABI_STREAM_PROF
        if (tid == 0 && blockIdx.x == 3 && blockIdx.y == 0) {
            for (int i = 0; i < 5; ++i) g_stream_prof[i] = prof[i];
            g_stream_prof[5] = wall_clock64() - prof_begin;
        }
#endif
    } else if (compute) {
        stream_compute_loop<D, PPT, GENERIC>(p, items, xa, aa, qs_s, scratch, abort_s, lane, wv);
    } else {
        // ---- record wave: under the compute waves' kernel sum, ring slot item+2, issue the load of item+3
        while (t < p.K) {
            items.next(t, split, bb);
            __syncthreads();                          // barrier A
            if (lane < 4) rec_s[pslot & 3][lane] = pend;
            items.next(pt, psplit, pbb); ++pslot;
            pend = stream_record_load(p, E, e, lane, pt, psplit, pbb);
            __syncthreads();                          // barrier B
            if (abort_s) return;
        }
    }
}

#ifdef ALABI_STREAM_PROF
extern "C" int alabi_debug_stream_prof(long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stream_prof), sizeof(long long) * 16);
}
#endif

// hist[0] <- (coords, logp); and back: (coords, logp) <- hist[K]
__global__ void __launch_bounds__(256)
ens_hist_fill_kernel(unsigned long long* __restrict__ h, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) h[i] = ALABI_HIST_EMPTY;
}

__global__ void __launch_bounds__(256)
ens_hist_copy_kernel(double* __restrict__ coords, double* __restrict__ logp, unsigned long long* __restrict__ hist_row,
                     int WT, int d, int to_hist) {
    const int i = blockIdx.x * 256 + threadIdx.x, row = d + 2;
    if (i >= WT * row) return;
    const int w = i / row, k = i % row;
    if (k > d) { if (to_hist) hist_row[i] = 0ull; return; }           // acceptance flag of version 0: unused
    double* src = (k < d) ? coords + (size_t)w * d + k : logp + w;
    if (to_hist) hist_row[i] = (unsigned long long)__double_as_longlong(*src);
    else *src = __longlong_as_double((long long)hist_row[i]);
}

// The one launch in front of a call's first persistent kernel: (coords, logp, n_accept) -> the handle's save area (what a time-out
// is repeated from), row 0 of the history <- (coords, logp) as ens_hist_copy_kernel writes it (hist_row0 == nullptr: the group
// kernel fills its own), and the time-out flag cleared.  One thread per word of a history row.
__global__ void __launch_bounds__(256)
ens_call_prologue_kernel(const double* __restrict__ coords, const double* __restrict__ logp, const long long* __restrict__ n_accept,
                         double* __restrict__ save, unsigned long long* __restrict__ hist_row0, int* __restrict__ err, int WT, int d) {
    const int i = blockIdx.x * 256 + threadIdx.x, row = d + 2;
    if (i == 0) *err = 0;
    if (i >= WT * row) return;
    const int w = i / row, k = i % row;
    if (k > d) {
        if (hist_row0) hist_row0[i] = 0ull;                            // acceptance flag of version 0: unused
        if (n_accept) reinterpret_cast<long long*>(save + (size_t)WT * (d + 1))[w] = n_accept[w];
        return;
    }
    const double v = (k < d) ? coords[(size_t)w * d + k] : logp[w];
    save[(k < d) ? (size_t)w * d + k : (size_t)WT * d + w] = v;
    if (hist_row0) hist_row0[i] = (unsigned long long)__double_as_longlong(v);
}

// After the persistent kernel: versions 1..K of every walker -> the (thinned) chain, and the acceptance counters.
// One thread per (version, walker, word); a few MB at HBM speed per launch of K steps.
__global__ void __launch_bounds__(256)
ens_hist_chain_kernel(const unsigned long long* __restrict__ hist, int K, int WT, int d, int thin_by,
                      const long long* __restrict__ run_state, const int* __restrict__ err, double* __restrict__ chain,
                      double* __restrict__ chain_logp, unsigned long long* __restrict__ n_accept) {
    if (*err) return;                                  // timed out: the rows are incomplete, the host reruns the chunk
    const int row = d + 2;
    const size_t n = (size_t)K * WT * row;
    const long long done0 = run_state[1];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int k = (int)(i % row);
        const size_t vw = i / row;
        const int w = (int)(vw % WT), v = (int)(vw / WT) + 1;
        const unsigned long long word = hist[(size_t)WT * row + i];
        if (k == d + 1) { if (word == 1ull && n_accept) atomicAdd(n_accept + w, 1ull); continue; }
        const long long done = done0 + v;
        if (done % thin_by != 0) continue;
        const size_t slot = (size_t)(done / thin_by - 1);
        if (k < d) { if (chain) chain[(slot * WT + w) * d + k] = __longlong_as_double((long long)word); }
        else if (chain_logp) chain_logp[slot * WT + w] = __longlong_as_double((long long)word);
    }
}

// Fused epilogue of a persistent launch of K steps (ens_stream_kernel): ONE pass over rows 1..K of the history that writes the
// thinned chain and chain_logp, counts the acceptances, writes (coords, logp) from row K, carries row K over to row 0 for the
// next chunk, puts the sentinel back into every word it has read (the history is ready for the next launch without a fill
// kernel) and advances run_state.  blockDim = (RP >= d + 2 words of a row, 256 / RP walkers); grid = (blocks of walkers,
// groups of VG versions): the row position is the thread index, the thinning phase is divided out once per workgroup, and the
// acceptance flags are summed per thread over its VG versions -- one atomic per (walker, workgroup).  After a time-out (*err)
// nothing but run_state is touched: the rows are incomplete, the host restores the walkers and refills the history.
// prop (pair variant, else nullptr): the published proposals have the history's shape, and the sentinel goes back into the same
// words of it, so that no chunk needs a fill kernel for it either.  state_out (last chunk of a call, else nullptr): the walkers
// after the chunk also go to [coords [WT, d] | logp [WT]] there, the block the call reads back.
#define ALABI_EPI_VG 16
__global__ void __launch_bounds__(256)
ens_hist_epilogue_kernel(unsigned long long* __restrict__ hist, int K, int WT, int d, int thin_by, long long step_next, long long done0,
                         const int* __restrict__ err, double* __restrict__ coords, double* __restrict__ logp, double* __restrict__ chain,
                         double* __restrict__ chain_logp, unsigned long long* __restrict__ n_accept, long long* __restrict__ run_state,
                         unsigned long long* __restrict__ prop, double* __restrict__ state_out) {
    const int k = threadIdx.x, row = d + 2;
    const int w = blockIdx.x * blockDim.y + threadIdx.y;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) { run_state[0] = step_next; run_state[1] = done0 + K; }
    if (*err) return;
    if (k >= row || w >= WT) return;
    const int v0 = 1 + blockIdx.y * ALABI_EPI_VG;
    const int v1 = (v0 + ALABI_EPI_VG - 1 < K) ? v0 + ALABI_EPI_VG - 1 : K;
    long long slot = (done0 + v0) / thin_by;          // version v is stored iff (done0 + v) % thin_by == 0, in slot (done0 + v) / thin_by - 1
    int phase = (int)((done0 + v0) % thin_by);
    const size_t vstride = (size_t)WT * row;
    const size_t first = (size_t)v0 * vstride + (size_t)w * row + k;
    unsigned long long* hp = hist + first;
    unsigned long long* pp = prop ? prop + first : nullptr;
    unsigned long long nacc = 0;
    for (int v = v0; v <= v1; v += 4, hp += 4 * vstride) {
        unsigned long long word[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) word[j] = (v + j <= v1) ? hp[j * vstride] : 0ull;   // four rows in flight
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (v + j > v1) break;
            hp[j * vstride] = ALABI_HIST_EMPTY;
            if (pp) pp[(size_t)(v - v0 + j) * vstride] = ALABI_HIST_EMPTY;
            if (k == d + 1) nacc += (word[j] == 1ull) ? 1ull : 0ull;
            else {
                const double val = __longlong_as_double((long long)word[j]);
                if (phase == 0) {
                    const size_t sw = (size_t)(slot - 1) * WT + w;
                    if (k < d) { if (chain) chain[sw * d + k] = val; }
                    else if (chain_logp) chain_logp[sw] = val;
                }
                if (v + j == K) {                     // the walkers after the chunk, and version 0 of the next one
                    hist[(size_t)w * row + k] = word[j];
                    if (k < d) coords[(size_t)w * d + k] = val; else logp[w] = val;
                    if (state_out) state_out[(k < d) ? (size_t)w * d + k : (size_t)WT * d + w] = val;
                }
            }
            if (++phase == thin_by) { phase = 0; ++slot; }
        }
    }
    if (k == d + 1 && n_accept && nacc) atomicAdd(n_accept + w, nacc);
}

// Version history around a persistent launch of K steps: rows 1..K <- sentinel (`fill`: when the rows are polled), row 0 <- (coords, logp) before it;
// (coords, logp) <- row K, chain / counters <- rows 1..K after it.  Shared by ens_stream_kernel and ens_group_kernel.
int launch_ens_hist_prologue(alabi_ens* e, double* coords, double* logp, int K, bool fill, hipStream_t s) {
    const int WT = e->W * e->E, row = e->d + 2;
    if (fill) hipLaunchKernelGGL(ens_hist_fill_kernel, dim3(1024), dim3(256), 0, s, e->hist + (size_t)WT * row, (size_t)K * WT * row);
    hipLaunchKernelGGL(ens_hist_copy_kernel, dim3((WT * row + 255) / 256), dim3(256), 0, s, coords, logp, e->hist, WT, e->d, 1);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_hist_epilogue(alabi_ens* e, double* coords, double* logp, int K, int thin_by, double* chain, double* chain_logp,
                             long long* n_accept, hipStream_t s) {
    const int WT = e->W * e->E, row = e->d + 2;
    hipLaunchKernelGGL(ens_hist_copy_kernel, dim3((WT * row + 255) / 256), dim3(256), 0, s, coords, logp,
                       e->hist + (size_t)K * WT * row, WT, e->d, 0);
    if (chain || chain_logp || n_accept)
        hipLaunchKernelGGL(ens_hist_chain_kernel, dim3(2048), dim3(256), 0, s, e->hist, K, WT, e->d, thin_by, e->run_state,
                           e->err, chain, chain_logp, reinterpret_cast<unsigned long long*>(n_accept));
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_hist_fill(unsigned long long* rows, size_t words, hipStream_t s) {
    hipLaunchKernelGGL(ens_hist_fill_kernel, dim3(1024), dim3(256), 0, s, rows, words);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

// What stands in front of a call's first persistent launch (ens_stream_kernel, ens_pair_kernel, ens_group_kernel): the walkers
// saved, the flag cleared and, with `row0`, row 0 of the history (later chunks find it there, left by the previous chunk's epilogue)
int launch_ens_call_prologue(alabi_ens* e, const double* coords, const double* logp, const long long* n_accept, bool row0, hipStream_t s) {
    const int WT = e->W * e->E, row = e->d + 2;
    hipLaunchKernelGGL(ens_call_prologue_kernel, dim3((WT * row + 255) / 256), dim3(256), 0, s, coords, logp, n_accept, e->save,
                       row0 ? e->hist : nullptr, e->err, WT, e->d);
    ALABI_LAUNCH_CHECK();
    e->save_valid = true; e->save_accept = n_accept != nullptr;
    return ALABI_OK;
}

StreamArgs ens_stream_args(alabi_ens* e, const DrawBuffers& rec, int K, const EnsSwitches& sw) {
    alabi_gp* gp = e->gp;
    StreamArgs a{};
    a.hist = e->hist; a.err = e->err; a.rec = rec; a.consts = e->consts;
    const bool se = gp->kf.type == 0;                 // squared exponential: centred inputs and h (se_pair_terms), built by ens_se_prepare
    a.Xt = se ? gp->Xc : gp->Xt; a.alpha = se ? gp->ens_h : gp->alpha; a.centre = gp->xa_centre;
    a.K = K; a.W = e->W; a.n0 = (e->W + 1) / 2; a.d = e->d; a.Npad = gp->Npad;
    a.spin_limit = ens_spin_limit_stream(sw);         // (ALABI_ENS_SPIN_LIMIT: tests force a time-out)
    a.amp = e->lp_scale * exp(gp->log_amp); a.mean = fma(e->lp_scale, gp->mean, e->lp_shift); a.kf = gp->kf;
    a.has_prior = e->has_prior; a.prior_const = e->prior_const;
    return a;
}

// One chunk of K steps on the persistent kernel, proposal records from `rec`.  Row 0 of the history holds the walkers (from
// ens_call_prologue_kernel or the previous chunk's epilogue); fill_rows > 0: rows 1..fill_rows cannot be trusted to hold the
// sentinel (first use of the handle, after a time-out or the group kernel) and are refilled.
int launch_ens_stream_kernel(alabi_ens* e, const DrawBuffers& rec, int K, int fill_rows, const EnsSwitches& sw, hipStream_t s) {
    int st;
    if (fill_rows > 0) {
        const size_t WT = (size_t)e->W * e->E, row = e->d + 2;
        if ((st = launch_ens_hist_fill(e->hist + WT * row, (size_t)fill_rows * WT * row, s)) != ALABI_OK) return st;
        e->boundary_stats[3]++;
    }
    const StreamArgs a = ens_stream_args(e, rec, K, sw);
    e->last_path = 1;
    st = ens_stream_dispatch(e, [&](auto D, auto PPT, auto TMAX, auto GENERIC) {
        hipLaunchKernelGGL((ens_stream_kernel<D(), PPT(), TMAX(), GENERIC()>), dim3(e->stream_grid, e->E), dim3(TMAX()), 0, s, a);
    });
    if (st != ALABI_OK) return st;
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

// The chunk's fused epilogue.  step_next / done0: the global step after the chunk and the steps of this call done before it,
// by value (nothing on the device is read to launch a chunk).  clean_prop: the chunk ran on ens_pair_kernel, whose proposals get the
// sentinel back; last: the call's last chunk, whose walkers also go to the block the call reads back.
int launch_ens_stream_epilogue(alabi_ens* e, double* coords, double* logp, int K, int thin_by, double* chain, double* chain_logp,
                               long long* n_accept, long long step_next, long long done0, bool clean_prop, bool last, hipStream_t s) {
    const int WT = e->W * e->E, row = e->d + 2;
    int rp = 16;                                      // words of a row rounded up to a power of two: threadIdx.x is the row position
    while (rp < row) rp <<= 1;
    const int wb = 256 / rp;
    hipLaunchKernelGGL(ens_hist_epilogue_kernel, dim3((WT + wb - 1) / wb, (K + ALABI_EPI_VG - 1) / ALABI_EPI_VG), dim3(rp, wb), 0, s,
                       e->hist, K, WT, e->d, thin_by, step_next, done0, e->err, coords, logp, chain, chain_logp,
                       reinterpret_cast<unsigned long long*>(n_accept), e->run_state, clean_prop ? e->prop : nullptr,
                       last ? reinterpret_cast<double*>(e->state_dev + 1) : nullptr);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // namespace alabi
