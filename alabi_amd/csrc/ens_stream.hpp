// What the persistent ensemble kernels (ens_stream_kernel in ens_stream.hip, ens_pair_kernel in ens_pair.hip) share: the version
// history's sentinel, the kernel arguments, the write-through hand-off accessors, the ordered sum of the wave partials, the
// parts of the kernel body that are the same in both -- per-launch set-up, item iterator, record load, compute-wave loop,
// bounded sentinel poll -- and the launch table.  The hand-off waves and the record waves differ on purpose and stay with
// their kernels.  ens_group.hip takes the sentinel and the accessors from here.
#pragma once
#include <type_traits>
#include "ens_device.hpp"

namespace alabi {

#define ALABI_HIST_EMPTY 0x7FF8A1AB1D15EA5Eull   // quiet NaN with a payload no computation produces

struct StreamArgs {
    unsigned long long* hist;    // [(K+1)][E*W][d+1] as raw 64-bit words; rows 1..K pre-filled with ALABI_HIST_EMPTY
    int* err;                    // [1], zeroed before the launch
    DrawBuffers rec;             // chunk base
    const double* consts;
    const double* Xt;            // squared exponential: gp->Xc (inputs relative to their mean) ...
    const double* alpha;         // ... and gp->ens_h (se_pair_terms)
    const double* centre;        // mean of the scaled training inputs (squared exponential)
    int K, W, n0, d, Npad, spin_limit, has_prior;
    double amp, mean, prior_const;
    KernelFn kf;
};

StreamArgs ens_stream_args(alabi_ens* e, const DrawBuffers& rec, int K, const EnsSwitches& sw);   // ens_stream.hip: the arguments of one chunk of K steps

__device__ inline unsigned long long ld_sc1(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void st_sc1(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Sum of the wave partials s[0..15] (zeros beyond the last compute wave) in exactly the order wave_sum_dpp adds
// lanes 0..15 of a row -- a balanced binary tree -- so this path and ens_half_kernel agree bit for bit.  Only the pairs that
// hold a partial are read; a pair beyond them is the +0.0 it holds, and the additions of such zeros that reach a live
// value stay in the code: x + 0.0 is +0.0 for x = -0.0, so they are not the identity.
template <int NW>
__device__ inline double wave_partials_tree(const double* s) {
    const f64x2* v = reinterpret_cast<const f64x2*>(s);
    auto pair = [&](int i) { return 2 * i < NW ? v[i].y + v[i].x : 0.0; };
    const double lo8 = (pair(3) + pair(2)) + (pair(1) + pair(0));
    if (NW <= 8) return lo8;
    const double hi8 = (pair(7) + pair(6)) + (pair(5) + pair(4));
    return hi8 + lo8;
}

// Per-launch set-up, every thread of the workgroup: the training-set share of this lane, resident for the whole launch (same
// lane -> point map as ens_half_kernel; zeros, or the squared exponential's padding, outside the compute waves and behind the
// training set), the six constant rows (1/length scale, lower, upper bound, prior mean, prior 1/std, centre), the partial
// slots and the abort word.  TC: compute threads.
template <int D, int PPT, int TC, bool GENERIC>
__device__ __forceinline__ void stream_setup(const StreamArgs& p, bool compute, f64x2 (&xa)[PPT][D], f64x2 (&aa)[PPT],
                                             double (&consts_s)[6][ALABI_MAX_DIM], double (&scratch)[2][16], int& abort_s) {
    const int tid = threadIdx.x;
    const int half = p.Npad >> 1, ct = tid - 64;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int idx = ct + j * TC;
        const bool v = compute && idx < half;
#pragma unroll
        for (int k = 0; k < D; ++k)
            xa[j][k] = v ? reinterpret_cast<const f64x2*>(p.Xt + (size_t)k * p.Npad)[idx] : f64x2{0.0, 0.0};
        aa[j] = v ? reinterpret_cast<const f64x2*>(p.alpha)[idx] : (GENERIC ? f64x2{0.0, 0.0} : f64x2{ALABI_SE_PAD, ALABI_SE_PAD});
    }
    if (tid < ALABI_MAX_DIM) {
        consts_s[0][tid] = (tid < p.d) ? p.consts[tid] : 0.0;
        consts_s[1][tid] = (tid < p.d) ? p.consts[ALABI_MAX_DIM + tid] : 0.0;
        consts_s[2][tid] = (tid < p.d) ? p.consts[2 * ALABI_MAX_DIM + tid] : 0.0;
        consts_s[3][tid] = (tid < p.d) ? p.consts[3 * ALABI_MAX_DIM + tid] : 0.0;
        consts_s[4][tid] = (tid < p.d) ? p.consts[4 * ALABI_MAX_DIM + tid] : 0.0;
        consts_s[5][tid] = (!GENERIC && tid < p.d) ? p.centre[tid] : 0.0;
    }
    if (tid < 32) scratch[tid >> 4][tid & 15] = 0.0;
    if (tid == 0) abort_s = 0;
}

// A workgroup's proposals: list positions b, b + G, b + 2G, ... of every half step, in (step, split, position) order
// (ens_stream_kernel: G = gridDim.x workgroups per ensemble; ens_pair_kernel: G = n0 pairs, so at most one per half step).
// Every role of a workgroup steps through them with this function, so all waves execute the same number of barriers.
struct StreamItems {
    const StreamArgs& p;
    int G, b;
    __device__ __forceinline__ void next(int& t, int& split, int& bb) const {
        bb += G;
        for (;;) {
            if (t >= p.K) return;
            if (bb < (split ? p.W - p.n0 : p.n0)) return;
            bb = b;
            if (split == 0) split = 1; else { split = 0; ++t; }
        }
    }
};

// Word `lane` < 4 of the packed proposal record of item (t, split, bb) of ensemble e; records depend on nothing, so the
// record wave fetches them ahead.
__device__ __forceinline__ unsigned long long stream_record_load(const StreamArgs& p, int E, int e, int lane, int t, int split, int bb) {
    if (t >= p.K || lane >= 4) return 0ull;
    const size_t pos = ((size_t)t * E + e) * p.W + (split ? p.n0 : 0) + bb;
    return p.rec.packed[4 * pos + lane];
}

// Bounded sentinel poll of the hand-off wave.  `look` loads this lane's words with ld_sc1 and says whether any lane of the wave
// still sees the sentinel; it is repeated until none does, the spin limit runs out or -- looked at every 64 spins -- another
// workgroup has reported a time-out.  Returns "still pending": the caller then marks the time-out and rejoins its fast path.
// (readfirstlane: a loaded value counts as divergent, and a divergent exit is threaded through exec-mask ladders)
template <class Look>
__device__ __forceinline__ bool stream_poll(const StreamArgs& p, Look&& look) {
    int spins = 0;
    bool pending;
    for (;;) {
        pending = look();
        if (!pending) break;
        if (__builtin_expect(++spins > p.spin_limit || ((spins & 63) == 0 && __builtin_amdgcn_readfirstlane(
                __hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0), 0)) break;
    }
    return pending;
}

// The same poll for words that were fetched ahead and are in registers: `test` says whether any lane's word is still the
// sentinel, `load` loads the words again AND waits for them (a pin on the loaded registers).  The first test is of the
// registers, so a complete fetch costs no load -- and no wait: were the loop's loads waited for at their first use, the wait
// would stand in the loop's header, in front of the first test too, and there it would (one vmcnt) wait for the row store the
// wave has just issued.  `loads` counts the repeats.  Spin limit and abort look as in stream_poll.
template <class Test, class Load>
__device__ __forceinline__ bool stream_poll_ahead(const StreamArgs& p, int& loads, Test&& test, Load&& load) {
    bool pending;
    for (;;) {
        pending = test();
        if (!pending) break;
        if (__builtin_expect(++loads > p.spin_limit || ((loads & 63) == 0 && __builtin_amdgcn_readfirstlane(
                __hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0), 0)) break;
        load();
    }
    return pending;
}

// Compute waves 1..nwc, from barrier A to barrier B of every proposal: A -> q -> sum -> DPP -> partial -> B.  They look at the
// abort word after barrier B, where they delay nobody.
template <int D, int PPT, bool GENERIC>
__device__ __forceinline__ void stream_compute_loop(const StreamArgs& p, const StreamItems& items, const f64x2 (&xa)[PPT][D],
                                                    const f64x2 (&aa)[PPT], const double (&qs_s)[2][ALABI_MAX_DIM],
                                                    double (&scratch)[2][16], const int& abort_s, int lane, int wv) {
    int t = 0, split = 0, bb = items.b, item = 0;
    while (t < p.K) {
        items.next(t, split, bb);
        const int par = item & 1;
        __syncthreads();                          // barrier A: the proposal is in LDS
        // ONE batch of LDS reads brings the proposal and its in-bounds flag: the broadcasts to SGPRs stand in front of the
        // test (a convergent operation is not sunk into the branch, so neither are the reads that feed it)
        double q[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double r = qs_s[par][k];
            q[k] = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(r)),
                                    __builtin_amdgcn_readfirstlane(__double2loint(r)));
        }
        const int inb = __builtin_amdgcn_readfirstlane(__double2hiint(qs_s[par][D]));
        // every LDS read is issued before the first is waited for: the reads (at most D + 1), then the broadcasts
        __builtin_amdgcn_sched_group_barrier(0x100, D + 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x2, 2 * D + 1, 0);
        if (inb != 0) {
            double acc = 0.0;
            if (!GENERIC) {
                const double nhq = se_neg_half_norm<D>(q);
#pragma unroll
                for (int j = 0; j < PPT; ++j) {
                    double fa, fb;
                    se_pair_terms<D>(xa[j], aa[j], q, nhq, fa, fb);
                    acc += fa; acc += fb;
                    if ((j & 1) == 1) __builtin_amdgcn_sched_barrier(0);   // four points in flight at a time
                }
            } else
#pragma unroll
            for (int j = 0; j < PPT; ++j) {
                double r2a = 0.0, r2b = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const double da = xa[j][k].x - q[k], db = xa[j][k].y - q[k];
                    r2a = fma(da, da, r2a);
                    r2b = fma(db, db, r2b);
                }
                // same operation order as ens_half_kernel's lane (first pair by multiply, the rest by fma)
                acc = (j == 0) ? aa[j].x * radial<GENERIC>(r2a, p.kf) : fma(aa[j].x, radial<GENERIC>(r2a, p.kf), acc);
                acc = fma(aa[j].y, radial<GENERIC>(r2b, p.kf), acc);
                if ((j & 1) == 1) __builtin_amdgcn_sched_barrier(0);   // four points in flight at a time: enough independent
                                                                       // chains to cover the fp64 latency, bounded temporaries
            }
            const double wsum = wave_sum_dpp(acc);
            if (lane == 63) scratch[par][wv - 1] = wsum;
        }
        __syncthreads();                          // barrier B: the wave partials are in LDS
        if (abort_s) return;
        ++item;
    }
}

// ---- launch table (host) ----------------------------------------------------------------------------------------------
// The fit rule of a (T, PPT, kernel family) row is ens_stream_max_db (ens_shared.hpp): ens_stream_ppt and the dispatch both read
// it, so an instantiation that can never be chosen is not compiled.

// One (T, PPT) row of the table: dimension bucket x kernel family.  launch(D, PPT, TMAX, GENERIC) gets the instantiation's
// template arguments as integral constants.
template <int T, int PPT, class Launch>
int ens_stream_dispatch_row(int db, int kernel_type, Launch& launch) {
    ALABI_DISPATCH_DIM16(db, ALABI_DISPATCH_KERNEL(kernel_type,
        if constexpr (D <= ens_stream_max_db(T, PPT, GENERIC))
            launch(std::integral_constant<int, D>(), std::integral_constant<int, PPT>(), std::integral_constant<int, T + 128>(),
                   std::integral_constant<bool, GENERIC>());
        else return ALABI_BAD_ARGUMENT));
    return ALABI_OK;
}

// Calls `launch` for the instantiation of this handle; ALABI_BAD_ARGUMENT when the handle does not fit (ens_stream_ppt == 0).
// Lanes x pairs-per-lane cover Npad/2 point pairs; the launch-per-half-step kernel's lane -> point map (and so its summation
// order) is reproduced exactly because both run with e->threads compute lanes.
template <class Launch>
int ens_stream_dispatch(const alabi_ens* e, Launch launch) {
    const int db = dim_bucket(e->d), kt = e->gp->kf.type;
    const int T = e->threads, ppt = ens_stream_ppt(ens_shape(e));
    if (T == 256 && ppt == 1) return ens_stream_dispatch_row<256, 1>(db, kt, launch);
    if (T == 256 && ppt == 2) return ens_stream_dispatch_row<256, 2>(db, kt, launch);
    if (T == 256 && ppt == 3) return ens_stream_dispatch_row<256, 3>(db, kt, launch);
    if (T == 256 && ppt == 4) return ens_stream_dispatch_row<256, 4>(db, kt, launch);
    if (T == 512 && ppt == 1) return ens_stream_dispatch_row<512, 1>(db, kt, launch);
    if (T == 512 && ppt == 2) return ens_stream_dispatch_row<512, 2>(db, kt, launch);
    return ALABI_BAD_ARGUMENT;
}

}  // namespace alabi
