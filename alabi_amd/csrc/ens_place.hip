// Placement pre-pass of the pair ensemble kernel: which pair runs which item, chosen so that an item runs on the XCD that
// made its fresh input row.
//
// ens_pair_kernel's half step is paced by hand-off hops, and a hop between two workgroups of one XCD is shorter than one
// across XCDs (tools/micro/pingpong_many.hip).  Nothing but the packed record ties list position b to pair b -- rows, prop and
// the chain are addressed by walker id -- so an item is handed to another pair by permuting the packed records of its half step
// in memory.  The persistent kernel then executes exactly the instructions it executes anyway, on `packed_x`.
//
// Pairs p with equal p % 8 share an XCD class (ens_pair_kernel's XCD map).  For the items of a half step, in list order:
//   preference   one fresh input row: the class that made it; both fresh: the class that made the partner's; none fresh: none.
//                A row is fresh iff its walker was updated in the half step just before (fresh_load's rule in ens_pair_kernel);
//   greedy       an item gets its preferred class while that class has fewer than n0 / 8 items, and there the lowest free pair;
//   leftovers    the items left over take the remaining pairs in ascending pair order.
// A half step's choice depends on the one before, so the half steps are a chain; the draws it reads are complete only when the
// previous chunk's persistent kernel ends (the draw kernel finds no free CU beside it), so the chain stands in the gap in front
// of the next persistent launch and has to be short.  Two things keep it so.  It is cut into SEGMENTS of ALABI_PLACE_SEG steps,
// one workgroup each, all at the same time: the first half step of a segment has no preference (ascending pairs), which costs
// 1 / (2 ALABI_PLACE_SEG) of the local hops.  And no memory access stands on it: the workgroup first brings the walker ids of
// the whole segment into LDS, wave 0 then walks the half steps from LDS to LDS, and the records are copied to their places
// at the end, by all waves.  Placement is for speed only: every permutation gives the same chain, bit for bit.
#include <cstdlib>
#include "common.hpp"

namespace alabi {

// Wave 0 needs about 1.6 us per half step (some 500 instructions of one wave), so 16 steps stood 52 us in the gap, 2 % of a
// 1024-step chunk; four steps stand 13 us there and give up an eighth of the first half steps' preferences.
#define ALABI_PLACE_SEG 4
#define ALABI_PLACE_THREADS 256

__device__ inline int place_rank(unsigned long long m) {      // set bits of m below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// grid (segments, E).  n0 % 8 == 0, n0 <= 128, W == 2 n0.  Every index fits 32 bits (at most 4 Mi records per chunk).
__global__ void __launch_bounds__(ALABI_PLACE_THREADS)
ens_place_kernel(DrawBuffers b, int K, int W, int n0, unsigned long long* stats) {
    __shared__ unsigned ids_s[2 * ALABI_PLACE_SEG][128];         // by half step and list position: walker | partner << 16 (ids within the ensemble)
    __shared__ unsigned char place_s[2 * ALABI_PLACE_SEG][128];  // ... the pair of the item
    __shared__ int tab_s[256];              // by walker: (local half step of its newest row + 1) << 8 | class that made it
    __shared__ unsigned char slot_s[128];   // the free pairs, ascending
    const int tid = threadIdx.x, lane = tid & 63, e = blockIdx.y, E = gridDim.y;
    const int t0 = blockIdx.x * ALABI_PLACE_SEG;
    const int nh = 2 * (min(t0 + ALABI_PLACE_SEG, K) - t0), cap = n0 >> 3, w0 = e * W;
    const int sh = 31 - __builtin_clz(n0) + ((n0 & (n0 - 1)) ? 1 : 0), per = 1 << sh;   // items of a half step, rounded up to a power of two
    const ulonglong2* src = reinterpret_cast<const ulonglong2*>(b.packed);
    ulonglong2* dst = reinterpret_cast<ulonglong2*>(b.packed_x);
    auto half_base = [&](int hl) { return (unsigned)(((t0 + (hl >> 1)) * E + e) * W + (hl & 1) * n0); };
    for (int i = tid; i < W; i += ALABI_PLACE_THREADS) tab_s[i] = -1;
    for (int k = tid; k < nh * per; k += ALABI_PLACE_THREADS) {
        const int hl = k >> sh, i = k & (per - 1);
        if (i < n0) {
            const unsigned long long ids = b.packed[4 * (half_base(hl) + i)];
            // (& 255: tab_s's size, whatever the record holds)
            ids_s[hl][i] = (((unsigned)(ids & 0xffffffffull) - w0) & 255) | ((((unsigned)(ids >> 32) - w0) & 255) << 16);
        }
    }
    __syncthreads();
    if (tid < 64) {                         // wave 0: the chain.  One wave in lockstep: its LDS accesses take effect in program order
        int n_pref = 0, n_hit = 0;
        for (int hl = 0; hl < nh; ++hl) {
            int w[2], pref[2], pair[2];
            bool valid[2], got[2];
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                valid[ps] = ps * 64 + lane < n0;
                const unsigned ids = valid[ps] ? ids_s[hl][ps * 64 + lane] : 0u;
                w[ps] = (int)(ids & 0xffff);
                const int to = tab_s[w[ps]], tp = tab_s[ids >> 16];
                const bool fo = (to >> 8) == hl, fp = (tp >> 8) == hl;
                pref[ps] = !valid[ps] ? 8 : fp ? tp & 255 : fo ? to & 255 : 8;
                got[ps] = false; pair[ps] = 0;
            }
            // greedy by class, list order = pass, then lane: `cnt` holds the eight class counts, one byte each
            unsigned long long cnt = 0;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(pref[ps] == c);
                    const int have = (int)((cnt >> (8 * c)) & 0xff), room = cap - have, r = place_rank(m);
                    if (pref[ps] == c && r < room) { got[ps] = true; pair[ps] = c + 8 * (have + r); }
                    cnt += (unsigned long long)min(__popcll(m), room) << (8 * c);
                }
                n_pref += __popcll(__builtin_amdgcn_ballot_w64(pref[ps] < 8));
                n_hit += __popcll(__builtin_amdgcn_ballot_w64(got[ps]));
            }
            int nfree = 0;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                const int p = ps * 64 + lane;
                const bool fr = p < n0 && (p >> 3) >= (int)((cnt >> (8 * (p & 7))) & 0xff);
                const unsigned long long m = __builtin_amdgcn_ballot_w64(fr);
                if (fr) slot_s[nfree + place_rank(m)] = (unsigned char)p;
                nfree += __popcll(m);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            int nleft = 0;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                const bool lo = valid[ps] && !got[ps];
                const unsigned long long m = __builtin_amdgcn_ballot_w64(lo);
                if (lo) pair[ps] = slot_s[nleft + place_rank(m)];
                nleft += __popcll(m);
            }
#pragma unroll
            for (int ps = 0; ps < 2; ++ps)
                if (valid[ps]) {
                    tab_s[w[ps]] = ((hl + 1) << 8) | (pair[ps] & 7);
                    place_s[hl][ps * 64 + lane] = (unsigned char)pair[ps];
                }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if (stats && lane == 0) { atomicAdd(stats, (unsigned long long)n_pref); atomicAdd(stats + 1, (unsigned long long)n_hit); }
    }
    __syncthreads();
    for (int k = tid; k < nh * per; k += ALABI_PLACE_THREADS) {   // every record to its pair's position
        const int hl = k >> sh, i = k & (per - 1);
        if (i < n0) {
            const unsigned base = half_base(hl);
            const int pair = place_s[hl][i];
            const ulonglong2 ra = src[2 * (base + i)], rc = src[2 * (base + i) + 1];
            dst[2 * (base + pair)] = ra;
            dst[2 * (base + pair) + 1] = rc;
            b.place[base + i] = pair;
        }
    }
}

// Placement is on for this handle: the route finds it eligible (ens_plan.hip: both halves of a step have n0 items, n0 % 8 == 0,
// at most 128 pairs, not switched off by ALABI_ENS_PLACE=0) and the counters could be had.  Decided at the first call that asks
// and kept.  The caller has checked ens_pair_ready.
bool ens_place_ready(alabi_ens* e, bool eligible) {
    if (e->place_state == 0) {
        e->place_state = -1;
        if (!eligible) return false;
        if (hipMalloc(&e->place_stats, 2 * sizeof(unsigned long long)) != hipSuccess ||
            hipMemset(e->place_stats, 0, 2 * sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        e->place_state = 1;
    }
    return e->place_state > 0;
}

// The pre-pass over the first K steps of a buffer set, behind the draws on the stream that made them.  count: add to the
// handle's counters (alabi_ens_place_stats).
int launch_ens_place(alabi_ens* e, DrawBuffers& set, int K, bool count, hipStream_t s) {
    const size_t n = (size_t)e->chunk_cap * e->W * e->E;
    if (!set.packed_x) ALABI_HIP_CHECK(hipMalloc(&set.packed_x, 4 * n * sizeof(unsigned long long)));
    if (!set.place) ALABI_HIP_CHECK(hipMalloc(&set.place, n * sizeof(int)));
    hipLaunchKernelGGL(ens_place_kernel, dim3((K + ALABI_PLACE_SEG - 1) / ALABI_PLACE_SEG, e->E), dim3(ALABI_PLACE_THREADS), 0, s, set, K, e->W,
                       (e->W + 1) / 2, count ? e->place_stats : nullptr);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // namespace alabi
