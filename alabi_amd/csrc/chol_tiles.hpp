// Tile primitives of the Cholesky factorisation, shared by the launch-per-step kernels (chol_steps.hpp) and the task queue
// (chol_queue.hpp): the rank-16 matrix-core update of a 16 x 16 tile in LDS, the 16-column slab recurrence of a diagonal block and
// the factorisation of a 64 x 64 diagonal tile built from them (one wave / a whole workgroup), one row's panel-solve recurrence.
// Device code only; compiled as part of gp_cholesky.hip (one translation unit for all Cholesky device code, see there).
#pragma once
#include "gp_device.hpp"

namespace alabi {

typedef double v4f64 __attribute__((ext_vector_type(4)));

// One fp64 MFMA rank-16 update of a 16x16 tile held in LDS:  C -= P Q^T, with P = rows pr.. and Q = rows qr.. of the
// same 16-column slab (columns c0..c0+15) of `M`.  One wavefront; lane l: A[m=l&15][k=l>>4], B[k=l>>4][n=l&15],
// C/D row (l>>4)+4i, column l&15.
template <int LD>
__device__ inline void tile_update_16(double (*C)[LD], int cr, int cc, double (*Pm)[LD], int pr, double (*Qm)[LD], int qr,
                                      int c0, int lane) {
    const int lr = lane & 15, lk = lane >> 4;
    v4f64 acc;
    double a[4], b[4];                                      // all twelve LDS reads in flight at once (one round trip, not five)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) { a[kk] = Pm[pr + lr][c0 + 4 * kk + lk]; b[kk] = Qm[qr + lr][c0 + 4 * kk + lk]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = C[cr + lk + 4 * i][cc + lr];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) asm volatile("" : "+v"(a[kk]), "+v"(b[kk]));
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[kk], b[kk], acc, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) C[cr + lk + 4 * i][cc + lr] = acc[i];
}

// 1/sqrt(piv) from the hardware estimate r0 (relative error <= 5.2e-8, tools/micro/rsq_accuracy) and ONE third-order step:
// with e = 1 - piv r0^2, 1/sqrt(piv) = r0 (1 + e/2 + 3 e^2/8 + O(e^3)), the dropped term is ~1e-22; measured 1.4e-16.
// Four dependent operations after the estimate (two Newton steps are six); the slab recurrence scales its column by this
// value, so it sits on the critical chain of every pivot.
__device__ inline double pivot_rsqrt(double piv) {
    const double r0 = __builtin_amdgcn_rsq(piv);
    const double e = fma(-(piv * r0), r0, 1.0);
    return fma(r0 * e, fma(0.375, e, 0.5), r0);
}

// One 16-column slab of the diagonal block's factorisation; lane = row, a[j] = the row's entry in slab column j.  Right-
// looking: pivot j is broadcast from its lane, the column is scaled by 1/sqrt(pivot) in EVERY lane -- the diagonal lane
// thereby gets L_jj = piv / sqrt(piv) (1.1 ulp) without a select -- and the row's remaining slab columns take their rank-1
// update at once, L[c0+k][c0+j] arriving by v_readlane from the lane that owns row c0+k.  The wave runs one instruction per
// ~5 cycles whatever its kind, so the slab costs what it issues: nothing per pivot but the chain itself -- no branch, no
// diagonal select, no bookkeeping of the reciprocals (potrf_dinv forms them from the finished diagonal) and no test of the
// pivot: a non-positive or non-finite pivot turns its own and every later column into NaN (rsq of it is NaN or inf, 0 * inf
// = NaN), the earlier columns stay finite, so the FIRST diagonal entry that is not > 0 afterwards is LAPACK's `info`
// (potrf_first_bad).
// (Round 3, measured and not kept: (i) the multipliers L[c0+k][c0+j], k >= j + 2, as uniform-address LDS reads of the just-scaled
// column instead of v_readlane pairs, with the reciprocal square root of pivot j + 1 interleaved by hand with the updates of
// pivot j -- bit-identical, no faster; (ii) the trailing columns updated from the UNSCALED column and 1 / pivot, which shortens
// the dependent chain from pivot to pivot from two cross-lane hops + eight operations to one hop + six but adds four
// instructions per pivot -- 7.6 -> 8.0 us for the 64-pivot factorisation.  Data-dependent s_memrealtime stamps (ALABI_CHOL_PROF)
// then put wave 0's slab recurrence at 1.1-1.2 us per 16 pivots = 172 cycles per pivot for ~31 instructions: a lone wave issues
// one instruction per ~5.5 cycles and the recurrence is bound by that COUNT, as the round-2 text says; the four recurrences are
// 4.6 of the factorisation's 7.5 us, the rank-16 updates between them, their barriers and the slab's LDS traffic the rest.
// (iii) EIGHT-column slabs in the task queue's diagonal factorisation (38 % fewer recurrence instructions: 8 x 156 instead of
// 4 x 504; rank-8 tile updates on all waves, the tile column that holds the slab written back in its second half only):
// the recurrences fell from 5.2 to 3.6 us and the seven instead of three slab boundaries (two barriers + an LDS round trip +
// two dependent matrix-core instructions each, ~0.45 us) took it back -- N = 2000 0.527 vs 0.527 ms on one box.)
__device__ inline void potrf_slab(double (&a)[16], int c0) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const double rinv = pivot_rsqrt(lane_bcast(a[j], c0 + j));
        a[j] *= rinv;
        double bc[16];                                      // all broadcasts of the column first: distinct SGPR pairs, so no
#pragma unroll                                              // readlane -> use wait states between them and the FMAs
        for (int k = j + 1; k < 16; ++k) bc[k] = lane_bcast(a[j], c0 + k);
#pragma unroll
        for (int k = j + 1; k < 16; ++k) a[k] = fma(-a[j], bc[k], a[k]);
    }
}

// 1-based index of the first diagonal entry of the finished tile that is not > 0 (NaN included), 0 if there is none; `lll` =
// L[lane][lane], one full wave.
__device__ inline int potrf_first_bad(double lll) {
    const unsigned long long m = __ballot(!(lll > 0.0));
    return m ? __ffsll((long long)m) : 0;
}

// 1 / L_ll for the row of `lane` from the finished diagonal: hardware reciprocal (4.5e-8) + two Newton steps.
__device__ inline double potrf_dinv(double lll) {
    double r = __builtin_amdgcn_rcp(lll);
    r = fma(fma(-lll, r, 1.0), r, r);
    r = fma(fma(-lll, r, 1.0), r, r);
    return r;
}

// Diagonal block held in LDS (row stride LD doubles), factorised in place by ONE wavefront in 16-column slabs.  Inside a
// slab every lane (= row) keeps its 16 entries in registers and the recurrence is right-looking: after pivot j the row's
// remaining slab columns take their rank-1 update at once, L[c0+k][c0+j] arriving by v_readlane from the lane that owns
// row c0+k, so the dependent chain per column is readlane -> rsqrt/Newton -> scale -> readlane -> one FMA and the other
// updates fill its shadow.  After a slab the trailing tiles get its rank-16 update on the matrix cores.  A non-positive
// pivot is reported as LAPACK's potrf `info` (1-based).  Returns 1/L_ii of row `lane`.  `__syncthreads` here is executed
// by one wave only when the caller's other waves wait at a later barrier, so plain wave-level ordering is used instead.
template <int LD>
__device__ inline double potrf_tile_lds(double (*Ls)[LD], int lane, int kb, int* __restrict__ info) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int c0 = 16 * s;
        double a[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = Ls[lane][c0 + j];      // row `lane`, this slab (rows < c0 carry unused values)
        potrf_slab(a, c0);
#pragma unroll
        for (int j = 0; j < 16; ++j) Ls[lane][c0 + j] = a[j];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                       // one wave: LDS writes above are ordered before the reads below
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // rank-16 update of the tiles right of / below the slab (lower triangle of the 16x16 tile grid)
#pragma unroll
        for (int ti = s + 1; ti < 4; ++ti)
#pragma unroll
            for (int tk = s + 1; tk <= ti; ++tk) tile_update_16<LD>(Ls, 16 * ti, 16 * tk, Ls, 16 * ti, Ls, 16 * tk, c0, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    const double lll = Ls[lane][lane];
    const int bad = potrf_first_bad(lll);
    if (bad != 0 && lane == 0) atomicCAS(info, 0, kb * 64 + bad);
    return potrf_dinv(lll);
}

// The same factorisation by a whole 256-thread workgroup: wave 0 runs the slab recurrences, the rank-16 tile updates
// between slabs (6, 3, 1 tiles) are dealt to the four waves.  Every thread must call it; returns 1/L_ii in wave 0.
template <int LD>
__device__ inline double potrf_tile_lds_wg(double (*Ls)[LD], int tid, int kb, int* __restrict__ info) {
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int c0 = 16 * s;
        if (w == 0) {
            double a[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) a[j] = Ls[lane][c0 + j];
            potrf_slab(a, c0);
#pragma unroll
            for (int j = 0; j < 16; ++j) Ls[lane][c0 + j] = a[j];
        }
        if (s == 3) break;
        __syncthreads();
        int t = 0;
#pragma unroll
        for (int ti = s + 1; ti < 4; ++ti)
#pragma unroll
            for (int tk = s + 1; tk <= ti; ++tk, ++t)
                if ((t & 3) == w) tile_update_16<LD>(Ls, 16 * ti, 16 * tk, Ls, 16 * ti, Ls, 16 * tk, c0, lane);
        __syncthreads();
    }
    __syncthreads();
    if (w != 0) return 1.0;
    const double lll = Ls[lane][lane];
    const int bad = potrf_first_bad(lll);
    if (bad != 0 && lane == 0) atomicCAS(info, 0, kb * 64 + bad);
    return potrf_dinv(lll);
}

// One row's recurrence over a 16-column slab of X L_kk^T = B (right-looking along the row: two dependent operations per
// column -- scale, first update -- and the other updates fill their shadow).  The 120 strictly-lower entries of the slab's
// triangle and the 16 reciprocals are wave-uniform LDS broadcasts; they are fetched in four column groups (3, 3, 4, 6
// columns: 42, 33, 30, 15 entries), each while the group before it is being applied, so the chain never waits for LDS and at
// most two groups are live: ~215 registers instead of 364 for fetching all 120 up front.  That matters beyond this kernel:
// a workgroup of the panel chain has to fit into the hole one retired workgroup of the bulk trailing update leaves on a SIMD
// (512 - 232 registers), or the chain cannot overlap that update at all.  sched_barrier keeps the compiler from sinking a
// group's reads next to their uses.
template <int J0, int J1, int LD>
__device__ inline void trsm_group_fetch(double (*lkk)[LD], const double* di, int c0, double* lg, double* dg) {
    int q = 0;
#pragma unroll
    for (int j = J0; j < J1; ++j) {
        dg[j - J0] = di[c0 + j];
#pragma unroll
        for (int k = j + 1; k < 16; ++k) lg[q++] = lkk[c0 + k][c0 + j];
    }
}
template <int J0, int J1>
__device__ inline void trsm_group_apply(double* b, const double* lg, const double* dg) {
    int q = 0;
#pragma unroll
    for (int j = J0; j < J1; ++j) {
        b[j] *= dg[j - J0];
#pragma unroll
        for (int k = j + 1; k < 16; ++k) b[k] = fma(-b[j], lg[q++], b[k]);
    }
}
template <int LD>
__device__ inline void trsm_slab_row(double (*lkk)[LD], double (*bs)[LD], const double* di, int row, int c0) {
    double b[16], l0[42], l1[33], l2[30], l3[15], d0[3], d1[3], d2[4], d3[6];
#pragma unroll
    for (int j = 0; j < 16; ++j) b[j] = bs[row][c0 + j];
    trsm_group_fetch<0, 3, LD>(lkk, di, c0, l0, d0);
    __builtin_amdgcn_sched_barrier(0);
    trsm_group_fetch<3, 6, LD>(lkk, di, c0, l1, d1);
    trsm_group_apply<0, 3>(b, l0, d0);
    __builtin_amdgcn_sched_barrier(0);
    trsm_group_fetch<6, 10, LD>(lkk, di, c0, l2, d2);
    trsm_group_apply<3, 6>(b, l1, d1);
    __builtin_amdgcn_sched_barrier(0);
    trsm_group_fetch<10, 16, LD>(lkk, di, c0, l3, d3);
    trsm_group_apply<6, 10>(b, l2, d2);
    __builtin_amdgcn_sched_barrier(0);
    trsm_group_apply<10, 16>(b, l3, d3);
#pragma unroll
    for (int j = 0; j < 16; ++j) bs[row][c0 + j] = b[j];
}

}  // namespace alabi
