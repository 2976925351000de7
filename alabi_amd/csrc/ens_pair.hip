// Persistent ensemble kernel, pair variant: both outcomes of a pending update on two CUs.
//
// ens_stream_kernel (ens_stream.hip) runs one workgroup per list position on half of the CUs, and a half step is a hand-off hop
// followed by a kernel sum, one after the other.  A proposal of half step h + 1 does not need the verdict of the half step-h
// update it reads, only the state of that walker, and that state is one of two rows which are both known early: the walker's
// previous row (in the history) and the proposal of half step h (known on its CU a whole kernel sum before its verdict).  Here
// every list position has a PAIR of workgroups, 2b ("R") and 2b + 1 ("A"), and every proposal is published when it is known
// to be the real one (`prop`, the same row layout and sentinel as `hist`).  For an input row produced in the immediately
// preceding half step ("fresh") R assumes that update was rejected and reads the previous version's row, A assumes it was
// accepted and reads the published proposal; both evaluate while the verdict is computed and travels, both poll the verdict
// (the acceptance flag of the fresh row; A with a fresh own row takes the old log-probability from the same row), and the one
// that assumed right does the accept test and the row store exactly as ens_stream_kernel does.  The other drops its sum.
//
// Freshness follows from the draws alone (class = number of fresh input rows):
//   second half of a step   the partner row (version t + 1) is fresh, the own row is not                       -> class 1
//   first half, t >= 1      a row is fresh iff its walker was in the second list of step t - 1 (pos_of >= n0)   -> class 0, 1, 2
//   step 0 of a launch      row 0 is complete before the launch                                               -> class 0
// class 0: R evaluates as ens_stream_kernel does, A skips the item.   class 1: as above.   class 2: no speculation (two of
// four outcomes would buy nothing): R polls both rows as ens_stream_kernel does, A skips.
// Exactly one workgroup of a pair writes prop and the history row of an item: R at formation for classes 0 and 2, the
// workgroup whose assumption held on the verdict's arrival for class 1 -- always, for an out-of-bounds proposal too, so that
// no reader waits for it.  Every dependency points to an earlier half step, so the oldest unfinished item can always run
// while all 2 G E workgroups are resident (the host launches at most one per CU).
// Arithmetic, lane -> point map, accumulation order, accept expression and row layout are those of ens_stream_kernel: the
// surviving sum is that kernel's sum, so the chains agree bit for bit.
// Fetch-ahead: between barrier A and barrier B of an item the hand-off wave has decoded the next item, so it loads that
// item's input words there (with every look of the verdict poll, or once) and keeps them in registers; the next item starts
// with a test of those registers and polls only if a lane still holds the sentinel.  R's rows are at least one verdict old, so
// the round trip of its first load no longer stands in front of every item.  A word goes from the sentinel to its value
// once per launch, so a fetched value is final; the last item of a launch fetches row 0.
#include <cstdlib>
#include "ens_stream.hpp"

namespace alabi {

struct PairArgs {
    StreamArgs s;
    unsigned long long* prop;    // [(K+1)][E*W][d+2] published proposals (words [0, d) of a row are read); rows 1..K pre-filled with ALABI_HIST_EMPTY
    unsigned long long* stats;   // nullptr, or [3 classes][3]: items, rows stored by R, rows stored by A, then [2 roles][2]: items, items
                                 // whose inputs the fetch-ahead had complete, then 2 words kept for the slot counters of alabi_ens_pair_stats2
                                 // then [2 roles][10]: the look counters of alabi_ens_pair_stats3, by lane of st_look (debug; accumulated outside the chain)
    int xmap;                    // 1: workgroup -> (pair, role) by XCD class (below); the records are those ens_place_kernel has permuted
};

#ifdef ALABI_PAIR_PROF
// hand-off wave of pair 3, [0..7] R, [8..15] A: [0] input poll, [1] rows detected -> barrier A, [2] A -> B (the verdict poll included),
// [3] B -> row store issued, [4] items, [5] ticks of the launch, [6] verdict-poll ticks of the class-1 items, [7] class-1 items;
// [16..19] R, [20..23] A: publish -> detect ticks of the prop rows read and their number, row store -> verdict detected and their number
// (the publisher leaves its clock in g_pair_pub, by row index modulo its size: [0] at the prop store, [1] at the row store);
// [24] R, [25] A: items whose inputs were complete at the first look (the fetch-ahead of the previous item)
__device__ long long g_pair_prof[26];
#define ALABI_PAIR_PUB_MASK ((1 << 19) - 1)
__device__ long long g_pair_pub[2][ALABI_PAIR_PUB_MASK + 1];
__device__ inline void pair_pub_stamp(int which, size_t row_index) {
    __hip_atomic_store(&g_pair_pub[which][row_index & ALABI_PAIR_PUB_MASK], wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline long long pair_pub_age(int which, size_t row_index, long long now) {
    const long long dt = now - __hip_atomic_load(&g_pair_pub[which][row_index & ALABI_PAIR_PUB_MASK], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (dt > 0 && dt < 100000) ? dt : -1;     // (a stamp of another launch, or one not yet visible: not counted)
}
#endif

// blockDim.x = TMAX = 64 + compute threads + 64; roles and barriers as in ens_stream_kernel, the set-up, the item iterator, the
// compute waves' loop and the bounded poll are that kernel's (ens_stream.hpp).
template <int D, int PPT, int TMAX, bool GENERIC>
__global__ void __launch_bounds__(TMAX)
ens_pair_kernel(PairArgs pa) {
    const StreamArgs& p = pa.s;
    __shared__ __attribute__((aligned(16))) double scratch[2][16];   // wave partials, by proposal parity
    __shared__ unsigned long long rec_s[4][6];                       // proposal-record ring: the packed record, own row fresh, partner row fresh
    __shared__ __attribute__((aligned(16))) double qs_s[2][ALABI_MAX_DIM];   // scaled proposal [0, D) and its in-bounds flag [D], by proposal parity
    __shared__ double consts_s[6][ALABI_MAX_DIM];
    __shared__ int abort_s;
    static_assert(D < ALABI_MAX_DIM && TMAX >= 192 && TMAX % 64 == 0, "ens_pair_kernel: shape");
    constexpr int TC = TMAX - 128, nwc = TC >> 6;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool comm = wv == 0, service = wv == nwc + 1, compute = !comm && !service;
    // Workgroups are dealt round-robin over the eight XCDs, so i % 8 labels the workgroups that share one.  With the XCD map
    // (n0 % 8 == 0) both roles of a pair, and all pairs with equal pair % 8, carry one label: ens_place_kernel hands an item to
    // a pair of the class that made its fresh input row.  For speed only: any map that is a bijection computes the same chain.
    const int xk = blockIdx.x >> 3;
    const int b = pa.xmap ? (xk >> 1) * 8 + (int)(blockIdx.x & 7) : (int)(blockIdx.x >> 1), e = blockIdx.y, E = gridDim.y;
    const int role_a = pa.xmap ? xk & 1 : blockIdx.x & 1;            // 1: this workgroup assumes "accepted"
    const int WT = p.W * E, row = p.d + 2;
#ifdef ALABI_PAIR_PROF
    long long prof[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const long long prof_begin = wall_clock64();
#endif
    f64x2 xa[PPT][D], aa[PPT];
    stream_setup<D, PPT, TC, GENERIC>(p, compute, xa, aa, consts_s, scratch, abort_s);

    // The pair's proposals: list position b of every half step that has one (G = n0 pairs per ensemble, so at most one item
    // per half step), in (step, split) order.
    const StreamItems items{p, (int)(gridDim.x >> 1), b};
    // Record wave: the packed record is fetched four items ahead (lane l < 4 loads word l); one item later, when its walker ids
    // are in registers, lanes 4 and 5 fetch the list positions of the two walkers in step t - 1, which say whether the rows
    // the proposal reads are fresh.  Both are in the ring two items before the hand-off wave decodes them.
    const int* pos_of = p.rec.pos_of;
    // lane 4: the own row is fresh, lane 5: the partner row is fresh (`rec`: the item's packed record, walker ids in lane 0)
    auto fresh_load = [&](int t, int split, unsigned long long rec) -> unsigned long long {
        const int w = __builtin_amdgcn_readlane((int)(unsigned)(rec & 0xffffffffull), 0);
        const int cw = __builtin_amdgcn_readlane((int)(unsigned)(rec >> 32), 0);
        if (t >= p.K || (lane != 4 && lane != 5)) return 0ull;
        if (split) return lane == 5 ? 1ull : 0ull;
        if (t == 0) return 0ull;
        return pos_of[(size_t)(t - 1) * WT + (lane == 4 ? w : cw)] >= p.n0 ? 1ull : 0ull;
    };
    unsigned long long rec_a = 0, fresh_a = 0, rec_b = 0;   // record and freshness of item + 2, record of item + 3
    int bt = 0, bsplit = 0;                                 // (step, split) of rec_b's item
    int pt = 0, psplit = 0, pbb = b, pslot = 0;             // the item the next record load is for
    if (service) {                                    // prologue: items 0 and 1 into the ring, item 2 in registers, item 3 in flight
        for (int i = 0; i < 2; ++i) {
            const unsigned long long r = stream_record_load(p, E, e, lane, pt, psplit, pbb);
            const unsigned long long f = fresh_load(pt, psplit, r);
            if (lane < 6) rec_s[pslot & 3][lane] = lane < 4 ? r : f;
            items.next(pt, psplit, pbb); ++pslot;
        }
        rec_a = stream_record_load(p, E, e, lane, pt, psplit, pbb);
        fresh_a = fresh_load(pt, psplit, rec_a);
        items.next(pt, psplit, pbb);
        bt = pt; bsplit = psplit;
        rec_b = stream_record_load(p, E, e, lane, pt, psplit, pbb);
        items.next(pt, psplit, pbb);
    }
    __syncthreads();
    int t = 0, split = 0, bb = b, item = 0;           // b < G = n0: the first item is valid

    if (comm) {
        // ---- hand-off wave: poll -> proposal -> LDS -> A -> (prior term, next decode, VERDICT poll + next inputs, candidate rows) -> B -> accept -> store
        const int n0_lane = lane < p.d ? lane : p.d, n1_lane = lane < p.d ? lane : p.d - 1;
        const int out_lane = lane <= p.d ? lane : p.d + 1, ver_lane = lane == p.d ? p.d : p.d + 1;
        long long prop_off = (long long)(pa.prop - p.hist);         // one base pointer: every address stays a global one
        // The generic kernels carry KernelFn in scalar registers and have none to spare, while this wave has vector registers to
        // spare: there, two wave-uniform values that the items only add to lane addresses are parked in vector registers -- the
        // offset of prop, and the counters' address, which also says whether they are on.  (The squared-exponential kernels
        // hold more of the training set per lane and have the scalar registers instead.)
        unsigned long long* stats_v = pa.stats;
        if (GENERIC) asm volatile("" : "+v"(prop_off), "+v"(stats_v));
        auto stats_on = [&] { return __builtin_amdgcn_readfirstlane((int)((unsigned long long)stats_v >> 32)) != 0; };   // (a device address)
        // the next item, decoded ahead
        int n_mode = 0, n_own_a = 0;                  // mode 0 evaluate (the winner is known), 1 speculate, 2 skip; A reads a fresh own row
        double n_zz = 0.0;
        size_t n_out = 0;                             // this lane's word of the new row (in hist, and in prop)
#ifdef ALABI_PAIR_PROF
        size_t n_fidx = 0;                            // row index of the fresh input row
#endif
        int n_cls = 0;                                // class of the item, in a vector register (read by the debug counters only)
        const unsigned long long *n_hw = p.hist, *n_hc = p.hist, *n_ver = p.hist;
        auto decode_next = [&](int it, int tt, int sp) {
            const unsigned long long* rs = rec_s[it & 3];
            const unsigned long long ids = rs[0];
            const int w = (int)(unsigned)(ids & 0xffffffffull);
            const int cw = (int)(unsigned)(ids >> 32);
            n_zz = __longlong_as_double((long long)rs[1]);
            n_cls = (int)rs[4] + (int)rs[5];
            const int fo = __builtin_amdgcn_readfirstlane((int)rs[4]), fp = __builtin_amdgcn_readfirstlane((int)rs[5]);
            const int spec = (fo + fp) == 1;
            n_mode = spec ? 1 : role_a ? 2 : 0;
            n_own_a = spec & role_a & fo;
            // own row at version t, partner row at version t (+1 when the partner's half went first).  R, class 1: the previous
            // version of the fresh row.  A, class 1: the fresh row from prop (words [0, d) only).  A, skipped item: row 0 (complete).
            const int vo = tt, vp = tt + sp;
            const int rv_o = vo - (spec & !role_a & fo), rv_p = vp - (spec & !role_a & fp);
            const size_t row_o = ((size_t)rv_o * WT + w) * row, row_p = ((size_t)rv_p * WT + cw) * row;
            const bool prop_o = spec && role_a && fo, prop_p = spec && role_a && fp;
            n_hw = p.hist + (row_o + (prop_o ? n1_lane : n0_lane)) + (prop_o ? prop_off : 0ll);
            n_hc = p.hist + (row_p + n1_lane) + (prop_p ? prop_off : 0ll);
            if (n_mode == 2) { n_hw = p.hist + n0_lane; n_hc = p.hist + n1_lane; }
            n_ver = p.hist + ((size_t)(fo ? vo : vp) * WT + (fo ? w : cw)) * row + ver_lane;
            n_out = ((size_t)(tt + 1) * WT + w) * row + out_lane;
#ifdef ALABI_PAIR_PROF
            n_fidx = (size_t)(fo ? vo : vp) * WT + (fo ? w : cw);
#endif
        };
        const double il_r = consts_s[0][lane], lo_r = consts_s[1][lane], hi_r = consts_s[2][lane], c_r = consts_s[5][lane];
        const bool needc = lane < p.d;
        const unsigned long long coord_lanes = (1ull << p.d) - 1;
        int st_items = 0, st_rows = 0;                // debug counters: lane c counts the items of class c
        int st_look = 0;                              // ... by lane (one compare per counter: the kernel has no scalar register for more masks).  Lane 0: looks of the verdict polls, lanes 2, 3, 4: polls decided at look 1, 2, 3 or
                                                      //     later; lane 5: looks (reloads) of the input polls, lanes 6..9: polls decided
                                                      //     without a reload, at look 1, 2, 3 or later
        // The next item's input words, fetched ahead in this item's idle window (item 0: nothing fetched, the sentinel).  Every
        // word of hist and prop goes from the sentinel to its value once per launch, so a fetched word that is not the sentinel
        // is final; a lane that still holds the sentinel sends the wave to the poll below.
        unsigned long long a_ws = ALABI_HIST_EMPTY, a_wc = ALABI_HIST_EMPTY;
        decode_next(0, 0, 0);
        while (t < p.K) {
            const int par = item & 1;
#ifdef ALABI_PAIR_PROF
            const long long c0 = wall_clock64();
#endif
            unsigned long long ws = a_ws, wc = a_wc;
            int loads = 0;
            const bool pending = stream_poll_ahead(p, loads, [&] {
                return __builtin_amdgcn_ballot_w64(ws == ALABI_HIST_EMPTY || wc == ALABI_HIST_EMPTY) != 0;
            }, [&] {
                ws = ld_sc1(n_hw);
                wc = ld_sc1(n_hc);
                asm volatile("" : "+v"(ws), "+v"(wc));   // waited for here, not in front of the first test
            });
            // debug counters, in registers (here: the count does not stay live in a scalar register)
            if (stats_on()) {
                int lv = loads;
                asm volatile("" : "+v"(lv));
                st_look += (lane == 5 ? lv : 0) + (lane == min(lv, 3) + 6);
            }
#ifdef ALABI_PAIR_PROF
            prof[11] += (loads == 0);
#endif
            // Bounded spin ran out: as in ens_stream_kernel the cold block rejoins the fast path -- a NaN stretch factor puts
            // the proposal out of bounds, this is the last proposal, nothing of it is stored or published.
            if (__builtin_expect(pending, 0)) {
                n_zz = __builtin_nan("");
                abort_s = 1;
                __hip_atomic_store(p.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#ifdef ALABI_PAIR_PROF
            const long long c1 = wall_clock64();
            const size_t fidx = n_fidx;
            if (n_mode == 1 && role_a && !pending) { const long long dt = pair_pub_age(0, fidx, c1); if (dt > 0) { prof[7] += dt; prof[8] += 1; } }
#endif
            const int mode = n_mode, own_a = n_own_a, cls = n_cls;
            const size_t out_word = n_out;
            const unsigned long long* ver = n_ver;
            const double sv = __longlong_as_double((long long)ws), cv = __longlong_as_double((long long)wc);
            const double qv = cv - (cv - sv) * n_zz;
            const bool all_in = mode != 2 && (__builtin_amdgcn_ballot_w64(qv > lo_r) & __builtin_amdgcn_ballot_w64(qv < hi_r) & coord_lanes)
                                                 == coord_lanes;
            double qs = qv * il_r;
            if (!GENERIC) qs -= c_r;
            qs_s[par][lane] = needc ? qs : 0.0;
            reinterpret_cast<int*>(&qs_s[par][D])[1] = all_in ? 0x3ff00000 : 0;
            // classes 0 and 2: this workgroup (R) holds the real proposal -- published at formation (the lanes behind the
            // coordinates write words d and d + 1 of the prop row, which nobody reads)
#ifdef ALABI_PAIR_PROF
            if (mode == 0 && !pending) pair_pub_stamp(0, out_word / row);
#endif
            if (mode == 0 && !pending) st_sc1(p.hist + (out_word + prop_off), (unsigned long long)__double_as_longlong(qv));
            __syncthreads();                          // barrier A: the proposal is in LDS
            __builtin_amdgcn_sched_barrier(0);
#ifdef ALABI_PAIR_PROF
            const long long c2 = wall_clock64();
#endif
            int t2 = t, s2 = split, b2 = bb;
            items.next(t2, s2, b2);
            if (pending) t2 = p.K;
            double prior_q = 0.0;
            if (p.has_prior) {
                const double u = (qv - consts_s[3][lane]) * consts_s[4][lane];
                prior_q = lane_bcast(wave_sum_dpp(needc ? -0.5 * u * u : 0.0), 63) + p.prior_const;
            }
            double lnfac = __longlong_as_double((long long)rec_s[item & 3][2]);
            double lnu = __longlong_as_double((long long)rec_s[item & 3][3]);
            double lp_old = lane_bcast(sv, p.d);      // lane d loaded logp (not so for A with a fresh own row: see below)
            int part = par * (int)sizeof(scratch[0]);
            if (t2 < p.K) decode_next(item + 1, t2, s2);
            else { n_hw = p.hist + n0_lane; n_hc = p.hist + n1_lane; }   // no next item: the fetch-ahead reads row 0
            // The verdict of the fresh row: its acceptance flag (every lane but lane d) and its log-probability (lane d).  Polled
            // here, in the window in which this wave is idle; the workgroup whose assumption holds publishes its proposal at once.
            // The next item's input words (decoded above) are fetched in the same window: with every look of the verdict poll,
            // else once -- a round trip that would otherwise stand in front of the next item although its rows are long there.
            int win = mode == 0;
            int v_looks = 0;                          // looks of this item's verdict poll, counted in a vector register (debug counters)
            asm volatile("" : "+v"(v_looks));
#ifdef ALABI_PAIR_PROF
            const long long c2v = wall_clock64();
#endif
            if (mode == 1 && !pending) {
                unsigned long long vw;
                const bool vpend = stream_poll(p, [&] {
                    vw = ld_sc1(ver);
                    a_ws = ld_sc1(n_hw);
                    a_wc = ld_sc1(n_hc);
                    v_looks += 1;
                    return __builtin_amdgcn_ballot_w64(vw == ALABI_HIST_EMPTY) != 0;
                });
                if (__builtin_expect(vpend, 0)) {     // time-out: the last proposal, nothing stored
                    abort_s = 1;
                    __hip_atomic_store(p.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    t2 = p.K;
                }
                // the fetched words arrive right behind the verdict (one vmcnt, in issue order).  They are waited for HERE: a wait
                // behind the prop store below would wait for that store's acknowledgement as well, in front of barrier B
                asm volatile("" : "+v"(a_ws), "+v"(a_wc));
                const int flag = __builtin_amdgcn_readfirstlane((int)(unsigned)(vw & 0xffffffffull));   // lane 0 polls the flag word (d >= 1)
                win = !vpend && flag == role_a;
#ifdef ALABI_PAIR_PROF
                if (win) pair_pub_stamp(0, out_word / row);
#endif
                if (win) st_sc1(p.hist + (out_word + prop_off), (unsigned long long)__double_as_longlong(qv));
                if (own_a) lp_old = lane_bcast(__longlong_as_double((long long)vw), p.d);
            } else {
                a_ws = ld_sc1(n_hw);
                a_wc = ld_sc1(n_hc);
                asm volatile("" : "+v"(a_ws), "+v"(a_wc));   // waited for in front of barrier B, in this branch
            }
#ifdef ALABI_PAIR_PROF
            const long long c2w = wall_clock64();
            if (mode == 1 && !pending) { const long long dt = pair_pub_age(1, fidx, c2w); if (dt > 0) { prof[9] += dt; prof[10] += 1; } }
#endif
            // the new row as it is written if the proposal is rejected / accepted (ens_stream_kernel's w_rej, w_acc)
            unsigned long long w_rej = needc ? ws : lane == p.d ? (unsigned long long)__double_as_longlong(lp_old) : 0ull;
            unsigned long long w_acc = !all_in ? w_rej : needc ? (unsigned long long)__double_as_longlong(qv) : 1ull;
            const bool takes_lp = all_in && lane == p.d;
            if (pending) win = 0;
            // debug counters, in registers; R sees every item
            if (stats_on()) {
                st_items += (cls == lane); st_rows += (cls == lane && win);
                st_look += (lane == 0 ? v_looks : 0) + (lane == min(v_looks, 3) + 1);   // (no verdict poll: lane 1, which nobody reads)
            }
            size_t ow = out_word;
            asm volatile("" : "+v"(ow), "+v"(w_rej), "+v"(w_acc), "+v"(lp_old), "+v"(lnfac), "+v"(lnu), "+v"(prior_q), "+v"(part));
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();                          // barrier B: the wave partials are in LDS
#ifdef ALABI_PAIR_PROF
            const long long c3 = wall_clock64();
#endif
            const double* partials = reinterpret_cast<const double*>(reinterpret_cast<const char*>(&scratch[0][0]) + part);
            const double lp_new = fma(p.amp, wave_partials_tree<nwc>(partials), p.mean) + prior_q;
            const bool acc = lnfac + lp_new - lp_old > lnu;
            if (takes_lp) w_acc = (unsigned long long)__double_as_longlong(lp_new);
#ifdef ALABI_PAIR_PROF
            if (win) pair_pub_stamp(1, ow / row);
#endif
            if (win) st_sc1(p.hist + ow, acc ? w_acc : w_rej);
            t = t2; split = s2; bb = b2; ++item;
#ifdef ALABI_PAIR_PROF
            { const long long c4 = wall_clock64();
              prof[0] += c1 - c0; prof[1] += c2 - c1; prof[2] += c3 - c2; prof[3] += c4 - c3; prof[4] += 1;
              if (mode == 1) { prof[5] += c2w - c2v; prof[6] += 1; } }
#endif
        }
        if (stats_on() && lane < 3) {
            if (!role_a) atomicAdd(stats_v + 3 * lane, (unsigned long long)st_items);
            atomicAdd(stats_v + 3 * lane + 1 + role_a, (unsigned long long)st_rows);
        }
        if (stats_on() && lane < 10) {
            atomicAdd(stats_v + 16 + 10 * role_a + lane, (unsigned long long)st_look);
            // alabi_ens_pair_stats2: every item is in one of the input poll's bins, the items fetched complete are the first of them
            if (lane >= 6) atomicAdd(stats_v + 9 + 2 * role_a, (unsigned long long)st_look);
            if (lane == 6) atomicAdd(stats_v + 10 + 2 * role_a, (unsigned long long)st_look);
        }
#ifdef ALABI_PAIR_PROF
        if (tid == 0 && b == 3 && blockIdx.y == 0) {
            long long* g = g_pair_prof + 8 * role_a;
            for (int i = 0; i < 5; ++i) g[i] = prof[i];
            g[5] = wall_clock64() - prof_begin;
            g[6] = prof[5]; g[7] = prof[6];
            for (int i = 0; i < 4; ++i) g_pair_prof[16 + 4 * role_a + i] = prof[7 + i];
            g_pair_prof[24 + role_a] = prof[11];
        }
#endif
    } else if (compute) {
        stream_compute_loop<D, PPT, GENERIC>(p, items, xa, aa, qs_s, scratch, abort_s, lane, wv);
    } else {
        // ---- record wave: ring slot item + 2 <- (record, freshness) in registers; freshness of item + 3; record of item + 4
        while (t < p.K) {
            items.next(t, split, bb);
            __syncthreads();                          // barrier A
            if (lane < 6) rec_s[pslot & 3][lane] = lane < 4 ? rec_a : fresh_a;
            ++pslot;
            rec_a = rec_b;
            fresh_a = fresh_load(bt, bsplit, rec_a);
            bt = pt; bsplit = psplit;
            rec_b = stream_record_load(p, E, e, lane, pt, psplit, pbb);
            items.next(pt, psplit, pbb);
            __syncthreads();                          // barrier B
            if (abort_s) return;
        }
    }
}

#ifdef ALABI_PAIR_PROF
extern "C" int alabi_debug_pair_prof(long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pair_prof), sizeof(long long) * 26);
}
#endif

// The pair variant can run this handle: the route finds it eligible (ens_plan.hip: one workgroup per CU for 2 ceil(W/2) E
// workgroups, not switched off by ALABI_ENS_PAIR=0), prop allocated (lazily, here), no earlier time-out of this handle.  Decided at
// the first call that asks and kept.  The caller has checked that the route is the persistent kernel.
bool ens_pair_ready(alabi_ens* e, bool eligible) {
    if (e->pair_state < 0) return false;
    if (e->pair_state == 0) {
        e->pair_state = -1;
        if (!eligible) return false;
        const size_t WT = (size_t)e->W * e->E, row = e->d + 2;
        const size_t words = ((size_t)e->chunk_cap + 1) * WT * row;
        if (hipMalloc(&e->prop, words * sizeof(unsigned long long)) != hipSuccess) { (void)hipGetLastError(); e->prop = nullptr; return false; }
        e->prop_clean = 0;
        e->pair_state = 1;
    }
    return true;
}

void ens_pair_release(alabi_ens* e) {
    if (e->prop) (void)hipFree(e->prop);
    if (e->pair_stats) (void)hipFree(e->pair_stats);
    if (e->place_stats) (void)hipFree(e->place_stats);
    e->prop = nullptr; e->pair_stats = nullptr; e->place_stats = nullptr;
}

// One chunk of K steps on the pair kernel; the arguments of launch_ens_stream_kernel, and prop_fill_rows > 0: rows
// 1..prop_fill_rows of prop cannot be trusted to hold the sentinel and are refilled (the chunk's epilogue puts it back, as in hist).
// placed: ens_place_kernel has run on this chunk's records; the kernel then reads rec.packed_x under the XCD map.
int launch_ens_pair_kernel(alabi_ens* e, const DrawBuffers& rec, int K, int fill_rows, int prop_fill_rows, bool placed, const EnsSwitches& sw,
                           hipStream_t s) {
    const int n0 = (e->W + 1) / 2;
    const size_t WT = (size_t)e->W * e->E, row = e->d + 2;
    int st;
    if (fill_rows > 0) {
        if ((st = launch_ens_hist_fill(e->hist + WT * row, (size_t)fill_rows * WT * row, s)) != ALABI_OK) return st;
        e->boundary_stats[3]++;
    }
    if (prop_fill_rows > 0) {
        if ((st = launch_ens_hist_fill(e->prop + WT * row, (size_t)prop_fill_rows * WT * row, s)) != ALABI_OK) return st;
        e->boundary_stats[2]++;
    }
    PairArgs a{};
    a.s = ens_stream_args(e, rec, K, sw);
    a.prop = e->prop; a.stats = e->pair_stats;
    if (placed) { a.s.rec.packed = rec.packed_x; a.xmap = 1; }
    e->last_path = 1;
    st = ens_stream_dispatch(e, [&](auto D, auto PPT, auto TMAX, auto GENERIC) {
        hipLaunchKernelGGL((ens_pair_kernel<D(), PPT(), TMAX(), GENERIC()>), dim3(2 * n0, e->E), dim3(TMAX()), 0, s, a);
    });
    if (st != ALABI_OK) return st;
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // namespace alabi
