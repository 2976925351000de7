// Predictive variance var* = k** - |L^-1 k*|^2 by blocked forward substitution: the first-generation kernel and the
// wave-specialised one with its K* pre-pass (launch_predict_var, launch_factor_inverse_into in gp_predict.hip).
//
// variance       : per tile of 64 queries a blocked forward substitution V = L^-1 K*^T.  For
//                  each 64-row block kb: the K* block is evaluated on the fly, the
//                  off-diagonal part  C = K*_kb - sum_{j<kb} L[kb,j] V_j  runs on the fp64
//                  matrix cores (v_mfma_f64_16x16x4_f64, L block and V block staged in LDS),
//                  the 64x64 diagonal solve runs as 16 columns per wave with 4 lanes per
//                  column exchanging the solved entry by wave shuffle.  V_j tiles live in a
//                  per-workgroup HBM workspace (they do not fit in 160 KB of LDS) and are
//                  re-read through L2.  N^2 flops per query (MFMA bound), L streamed once per
//                  64-query tile.
// The module-scope LDS stages ws_As / ws_Vs / ws_dis declared here are shared with the kernels of predict_var_winv.hpp, which
// must follow this header.  Device code only; compiled as part of gp_predict.hip (one translation unit, see there).
#pragma once
#include "gp_device.hpp"

namespace alabi {

typedef double v4f64 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// IDENT = true turns the same blocked forward substitution into a triangular inversion: the right-hand side of
// tile t is columns 64t..64t+63 of the identity, the V tiles are the OUTPUT (ws[t] = L^-1[:, 64t:64t+64] as
// [Npad][64], rows above block t are never written nor read), and nothing else is produced.
template <int D, bool IDENT = false>
__global__ void __launch_bounds__(256, 2)
predict_var_kernel(const double* __restrict__ L, const double* __restrict__ dinv, const double* __restrict__ Xt,
                   const double* __restrict__ alpha, int N, int Npad, const double* __restrict__ Xs, int d, long long M, DimVec inv_len,
                   double amp, double mean, double* __restrict__ ws, double* __restrict__ mu,
                   double* __restrict__ var, int split, KernelFn kf) {
    // `split` is always 0.  The `split != k` tests below are opaque to the compiler and put the GEMM step and the
    // unrolled diagonal solve into basic blocks of their own: as ONE block the register allocator hoists the
    // solve's LDS reads into the GEMM phase and spills 100 VGPRs to scratch inside the hot loop
    // (measured on MI355X: 11.3 ms -> 6.9 ms per 65536 queries at N=2000).
    __shared__ double As[64][66];   // L[kb,j] block, then L[kb,kb]
    __shared__ double Vs[64][80];   // V_j tile (MFMA B operand), then the C tile
    __shared__ double xtr[D][64];   // scaled coordinates of training block kb
    __shared__ double alb[64];
    __shared__ double dis[64];      // 1 / L_rr of block kb
    const int tid = threadIdx.x, c = tid & 63, w = tid >> 6;
    const int lr = c & 15, lk = c >> 4;  // MFMA lane decomposition within the wave
    const int nb = Npad / 64, ld = Npad;
    double* V = ws + (size_t)blockIdx.x * Npad * 64;
    const long long ntiles = (M + 63) / 64;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long m = tile * 64 + c;
        if (IDENT) V = ws + (size_t)tile * Npad * 64;
        const int kb0 = IDENT ? (int)tile : 0;       // first block row with a non-zero right-hand side
        double q[D];
#pragma unroll
        for (int k = 0; k < D; ++k) q[k] = (!IDENT && m < M && k < d) ? Xs[m * d + k] * inv_len.v[k] : 0.0;
        double mu_acc = 0.0, ss = 0.0;
        for (int kb = kb0; kb < nb; ++kb) {
            __syncthreads();   // the previous block's solve has finished with As / Vs / xtr / alb / dis
            // Software pipeline: the 64x64 L block and V tile of step j+1 travel HBM/L2 -> registers (16 B per
            // lane, 8 + 8 loads) while step j runs on the matrix cores; the first stage is issued here so
            // that the K* evaluation below hides it.
            f64x2 pa[8], pv[8];
            {
                const double* Lb = L + (size_t)(kb * 64) * ld + (kb > kb0 ? kb0 * 64 : kb * 64);
                const double* V0 = V + (size_t)(kb0 * 64) * 64;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int e = tid + 256 * i, r = e >> 5, c2 = e & 31;
                    pa[i] = *reinterpret_cast<const f64x2*>(Lb + (size_t)r * ld + 2 * c2);
                    if (kb > kb0 && split != 1) pv[i] = reinterpret_cast<const f64x2*>(V0)[e];
                }
            }
            for (int e = tid; e < D * 64; e += 256) xtr[e >> 6][e & 63] = Xt[(size_t)(e >> 6) * Npad + kb * 64 + (e & 63)];
            if (tid < 64) { alb[tid] = alpha[kb * 64 + tid]; dis[tid] = dinv[kb * 64 + tid]; }
            __syncthreads();
            // K* block: thread (column c, wave w) evaluates rows 16w .. 16w+15
#pragma unroll 4
            for (int i = 0; i < 16; ++i) {
                const int r = w * 16 + i;
                double r2 = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    double df = xtr[k][r] - q[k];
                    r2 = fma(df, df, r2);
                }
                double kv = (kb * 64 + r < N) ? amp * radial(r2, kf) : 0.0;
                if (IDENT) kv = (kb == kb0 && r == c) ? 1.0 : 0.0;
                mu_acc = fma(kv, alb[r], mu_acc);
                Vs[r][c] = kv;
            }
            __syncthreads();
            v4f64 acc[4];
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[n][i] = Vs[16 * w + lk + 4 * i][16 * n + lr];
            for (int j = kb0; j < kb; ++j) {
                __syncthreads();       // every wave is done reading As / Vs
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int e = tid + 256 * i, r = e >> 5, c2 = e & 31;
                    *reinterpret_cast<f64x2*>(&As[r][2 * c2]) = pa[i];
                    *reinterpret_cast<f64x2*>(&Vs[r][2 * c2]) = pv[i];
                }
                __syncthreads();
                {   // next stage: L[kb, j+1] and V_{j+1}, or the diagonal block L[kb, kb] after the last step
                    const int jn = j + 1;
                    const double* Lb = L + (size_t)(kb * 64) * ld + jn * 64;
                    const double* Vj = V + (size_t)(jn * 64) * 64;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int e = tid + 256 * i, r = e >> 5, c2 = e & 31;
                        if (split != 2) pa[i] = *reinterpret_cast<const f64x2*>(Lb + (size_t)r * ld + 2 * c2);
                        if (jn < kb && split != 1) pv[i] = reinterpret_cast<const f64x2*>(Vj)[e];
                    }
                }
                if (split != 3)
#pragma unroll
                for (int ks = 0; ks < 16; ++ks) {
                    double a = -As[16 * w + lr][4 * ks + lk];
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        double b = Vs[4 * ks + lk][16 * n + lr];
                        acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[n], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int i = 0; i < 4; ++i) Vs[16 * w + lk + 4 * i][16 * n + lr] = acc[n][i];
#pragma unroll
            for (int i = 0; i < 8; ++i) {   // pa holds L[kb,kb]; only its lower triangle is read below
                const int e = tid + 256 * i, r = e >> 5, c2 = e & 31;
                *reinterpret_cast<f64x2*>(&As[r][2 * c2]) = pa[i];
            }
            __syncthreads();
            // diagonal solve: wave w owns columns 16w..16w+15; lane (col lr, group lk) holds rows == lk (mod 4)
            const int col = 16 * w + lr;
            double v[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) v[t] = Vs[4 * t + lk][col];
            if (split != 4)
#pragma unroll
            for (int r = 0; r < 64; ++r) {
                const int owner = r & 3, t = r >> 2;
                double x = v[t] * dis[r];
                x = __shfl(x, lr + 16 * owner, 64);
                if (lk == owner) v[t] = x;
#pragma unroll
                for (int t2 = 0; t2 < 16; ++t2) {
                    if (4 * t2 + 3 > r) {
                        const int r2 = 4 * t2 + lk;
                        if (r2 > r) v[t2] = fma(-As[r2][r], x, v[t2]);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                V[(size_t)(kb * 64 + 4 * t + lk) * 64 + col] = v[t];
                ss = fma(v[t], v[t], ss);
            }
        }
        ss += __shfl_xor(ss, 16, 64);
        ss += __shfl_xor(ss, 32, 64);
        if (IDENT) continue;
        {
            const long long mc = tile * 64 + 16 * w + lr;
            if (lk == 0 && mc < M) var[mc] = amp - ss;
        }
        __syncthreads();
        Vs[w][c] = mu_acc;
        __syncthreads();
        if (tid < 64 && m < M) mu[m] = ((Vs[0][c] + Vs[1][c]) + (Vs[2][c] + Vs[3][c])) + mean;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Wave-specialised variance kernel (the one launch_predict_var uses for d <= 32 when the cached L^-1 is not used).  Same algorithm and data layout as
// predict_var_kernel above -- per 64-query tile a blocked forward substitution V = L^-1 K*^T, off-diagonal updates on the
// fp64 matrix cores -- but the workgroup is split into producers and consumers so that memory traffic and MFMA work overlap
// (ablation of the kernel above at N=2000, M=65536: MFMA alone 3.3 ms, loads + LDS staging + solves alone 4.15 ms,
// together 7.0 ms: they were serialised by the two barriers of every step).
//
//   768 threads, ONE workgroup per CU (LDS: two full stages, 155 KB).
//   waves 0-3 (consumers)  run the 64 MFMAs of a stage out of LDS buffer b&1, and the 64x64 diagonal solve at the end of a
//                          block row; nothing else.
//   waves 4-11 (producers) stream the flattened stage sequence (kb, s), s = kb0..kb (s == kb: the diagonal block):
//                          global -> registers two stages ahead, registers -> LDS buffer (b+1)&1 while the consumers work on
//                          stage b; during a diagonal solve they evaluate the K* block of block row kb+2 and park it in
//                          the workspace rows where V_{kb+2} will later be written (the consumers fetch it as their next
//                          accumulator while they solve).
//   One barrier per stage (two in a diagonal stage).  V_s must exist before a producer loads it: a stage whose V block is
//   not finished yet gets its V part issued late; the one stage that needs V the moment it is produced (block row kb0+1)
//   receives it from the consumers through LDS directly.
// Pointer parameters of a (non-inlined) device function are generic: loads through them are FLAT instructions, which
// count on the LDS counter as well and would serialise the prefetch pipeline with every LDS access.  The role functions
// therefore cast their buffer pointers to the global address space first.
typedef const double __attribute__((address_space(1)))* ws_gcptr;
typedef double __attribute__((address_space(1)))* ws_gptr;
typedef const f64x2 __attribute__((address_space(1)))* ws_gcptr2;
// Module-scope LDS (two full stages): named directly by the role functions, so every access stays an LDS instruction
// (passed as pointer arguments they degrade to generic pointers: 64-bit address arithmetic and a null check per access).
__shared__ double ws_As[2][64][66];
__shared__ double ws_Vs[2][64][80];
__shared__ double ws_dis[2][64];

// Producer waves of one tile.  Separate noinline functions per role: compiled as one body, the register allocator
// merges the live ranges of both roles and spills hundreds of VGPRs.  No store and no spill may sit in the stage loop: on
// gfx950 loads and stores share one counter, and with both kinds pending the compiler can only wait for ALL of them
// (vmcnt(0)), which would drain the stage that is meant to stay in flight.
template <int TM>
__device__ __attribute__((noinline)) void
ws_produce_tile(const double* L_, const double* dinv_, int Npad, const double* V_, int kb0) {
    const ws_gcptr L = (ws_gcptr)L_, dinv = (ws_gcptr)dinv_, V = (ws_gcptr)V_;
    const int t8 = threadIdx.x - 256;          // 256 producer threads: 8 + 8 loads per stage each
    // kb0: first block row with a non-zero right-hand side (0 for predictions; the tile's own block row when the columns of
    // the identity are pushed through to build L^-1): the stage sequence is (kb, s), kb0 <= s <= kb < nb
    const int nb = Npad / 64, ld = Npad, nr = nb - kb0, nstages = nr * (nr + 1) / 2;
    // Two register sets; every stage issues exactly 8 + TM/8 + 1 loads (a diagonal stage loads a V block it does not use), so
    // the wait for the OLDER set is a constant vmcnt and the younger set stays in flight.
    f64x2 pa[2][8], pv[2][TM / 8];
    double pd[2];
    // Thread t8 owns row t8 >> 2 of a 64 x 64 block and the 16-byte chunks (t8 & 3) + 4 i, i = 0..7, of that row: one base
    // address per block, the eight loads and LDS writes differ by immediates (64 B apart; a wave covers 16 rows x 64 B).
    const int prow = t8 >> 2, pch = t8 & 3;
#define ALABI_WS_ISSUE(SET, KB, S)                                                                            \
    {                                                                                                         \
        const ws_gcptr2 Lb_ = (ws_gcptr2)(L + ((size_t)((KB) * 64 + prow)) * ld + (S) * 64) + pch;            \
        const ws_gcptr2 Vj_ = (ws_gcptr2)(V + ((size_t)(((S) < (KB) ? (S) : kb0) * 64 + prow)) * TM) + pch;   \
        _Pragma("unroll") for (int i = 0; i < 8; ++i) pa[SET][i] = Lb_[4 * i];                                \
        _Pragma("unroll") for (int i = 0; i < TM / 8; ++i) pv[SET][i] = Vj_[4 * i];                           \
        pd[SET] = dinv[(KB) * 64 + (t8 & 63)];                                                                \
    }
#define ALABI_WS_TO_LDS(SET, BUF, WITH_V)                                                                     \
    {                                                                                                         \
        f64x2* as_ = reinterpret_cast<f64x2*>(&ws_As[BUF][prow][0]) + pch;                                    \
        f64x2* vs_ = reinterpret_cast<f64x2*>(&ws_Vs[BUF][prow][0]) + pch;                                    \
        _Pragma("unroll") for (int i = 0; i < 8; ++i) as_[4 * i] = pa[SET][i];                                \
        if (WITH_V) { _Pragma("unroll") for (int i = 0; i < TM / 8; ++i) vs_[4 * i] = pv[SET][i]; }           \
        if (t8 < 64) ws_dis[BUF][t8] = pd[SET];                                                               \
    }
#define ALABI_WS_ADVANCE(KB, S) { if (++(S) > (KB)) { ++(KB); (S) = kb0; } }
    // ---- phase A: block rows kb0..kb0+3, one stage at a time (a V block may be needed a stage or two after it is produced) ----
    int b = 0, kb = kb0, sj = kb0;             // the stage the consumers are working on
    ALABI_WS_ISSUE(0, kb0, kb0)
    ALABI_WS_TO_LDS(0, 0, false)
    __syncthreads();                           // stage 0 is in LDS
    int k1 = kb0, s1 = kb0;                    // stage b + 1
    ALABI_WS_ADVANCE(k1, s1)
    while (b < nstages && kb < kb0 + 4) {
        const int nbuf = (b & 1) ^ 1;
        const bool diag = sj == kb;
        if (b > 0) __syncthreads();            // stage b is in LDS buffer b & 1; buffer nbuf is free
        if (diag) __syncthreads();             // the consumers' mid-stage barrier
        if (b + 1 < nstages) {
            ALABI_WS_ISSUE(0, k1, s1)
            // stage (kb0 + 1, kb0) needs V_kb0 the moment it is produced: the consumers hand it over in LDS themselves
            ALABI_WS_TO_LDS(0, nbuf, (s1 < k1 && b > 0))
        }
        ++b;
        ALABI_WS_ADVANCE(kb, sj)
        ALABI_WS_ADVANCE(k1, s1)
    }
    // ---- phase B: block rows >= kb0 + 4, two stages ahead.  Set 1 holds stage b + 1 for even b - bA, set 0 for odd. ----
    if (b < nstages) {
        // here (kb, sj) = (kb0 + 4, kb0) = stage b (already in LDS), (k1, s1) = stage b + 1
        int k2 = k1, s2 = s1;
        ALABI_WS_ADVANCE(k2, s2)               // stage b + 2
        ALABI_WS_ISSUE(1, k1, s1)
        ALABI_WS_ISSUE(0, k2, s2)
        int k3 = k2, s3 = s2;                  // stage b + 3, clamped to the last stage (harmless reloads at the very end)
#define ALABI_WS_STAGE(NSET)                                                                                  \
        {                                                                                                     \
            const int nbuf = (b & 1) ^ 1;                                                                     \
            const bool diag = sj == kb;                                                                       \
            __syncthreads();               /* stage b is in LDS buffer b & 1; buffer nbuf is free */          \
            if (diag) __syncthreads();     /* the consumers' mid-stage barrier */                             \
            ALABI_WS_TO_LDS(NSET, nbuf, true)                                                                 \
            if (k3 < nb - 1 || s3 < k3) ALABI_WS_ADVANCE(k3, s3)                                              \
            ALABI_WS_ISSUE(NSET, k3, s3)                                                                      \
            ++b;                                                                                              \
            ALABI_WS_ADVANCE(kb, sj)                                                                          \
        }
        while (b < nstages) {
            ALABI_WS_STAGE(1)
            if (b >= nstages) break;
            ALABI_WS_STAGE(0)
        }
#undef ALABI_WS_STAGE
    }
#undef ALABI_WS_ISSUE
#undef ALABI_WS_TO_LDS
#undef ALABI_WS_ADVANCE
}

// Consumer waves of one tile: returns this lane's share of |L^-1 k*|^2 (before the cross-lane fold).
template <int TM>
__device__ __attribute__((noinline)) double
ws_consume_tile(int Npad, double* V_, int kb0) {
    constexpr int NT = TM / 16;            // MFMA column tiles per wave
    constexpr int CPW = TM / 4;            // solve: columns per wave ...
    constexpr int LPC = 64 / CPW;          // ... lanes per column (lane group g holds rows g, g + LPC, ...)
    constexpr int RPL = 64 / LPC;          // ... rows per lane
    const ws_gptr V = (ws_gptr)V_;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;
    const int lr = lane & 15, lk = lane >> 4;  // MFMA lane decomposition
    const int cl = lane % CPW, g = lane / CPW;
    const int nb = Npad / 64;
    double ss = 0.0;
    __syncthreads();                   // stage 0 is in LDS
    v4f64 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[n][i] = V[(size_t)(kb0 * 64 + 16 * w + lk + 4 * i) * TM + 16 * n + lr];
    int b = 0;
    for (int kb = kb0; kb < nb; ++kb)
        for (int sj = kb0; sj <= kb; ++sj, ++b) {
            const int buf = b & 1, nbuf = buf ^ 1;
            if (b > 0) __syncthreads();    // stage b is in LDS buffer buf
            if (sj < kb) {
#pragma unroll
                for (int ks = 0; ks < 16; ++ks) {
                    const double a = -ws_As[buf][16 * w + lr][4 * ks + lk];
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const double bb = ws_Vs[buf][4 * ks + lk][16 * n + lr];
                        acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[n], 0, 0, 0);
                    }
                }
                continue;
            }
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int i = 0; i < 4; ++i) ws_Vs[buf][16 * w + lk + 4 * i][16 * n + lr] = acc[n][i];
            if (kb + 1 < nb) {             // next block row's accumulator seed (the K* pre-pass left it in the workspace)
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc[n][i] = V[(size_t)((kb + 1) * 64 + 16 * w + lk + 4 * i) * TM + 16 * n + lr];
            }
            __syncthreads();
            // diagonal solve: wave w owns columns CPW w .. CPW w + CPW - 1; lane (col cl, group g) holds rows == g (mod LPC)
            const int col = CPW * w + cl;
            double v[RPL];
#pragma unroll
            for (int t = 0; t < RPL; ++t) v[t] = ws_Vs[buf][LPC * t + g][col];
#pragma unroll
            for (int r = 0; r < 64; ++r) {
                const int owner = r % LPC, t = r / LPC;
                double x = v[t] * ws_dis[buf][r];
                x = __shfl(x, cl + CPW * owner, 64);
                // rows of the pivot's own group: lanes below the pivot are done (select, no branch: straight-line code);
                // every later group takes the update unconditionally
                const double a_own = ws_As[buf][LPC * t + g][r];
                v[t] = (g == owner) ? x : ((g > owner) ? fma(-a_own, x, v[t]) : v[t]);
#pragma unroll
                for (int t2 = t + 1; t2 < RPL; ++t2) v[t2] = fma(-ws_As[buf][LPC * t2 + g][r], x, v[t2]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < RPL; ++t) {
                V[(size_t)(kb * 64 + LPC * t + g) * TM + col] = v[t];
                if (kb == kb0) ws_Vs[nbuf][LPC * t + g][col] = v[t];   // the next stage needs this block at once: LDS hand-over
                ss = fma(v[t], v[t], ss);
            }
        }
    return ss;
}

// K* pre-pass of the wave-specialised variance path: one workgroup per 64-query tile writes the tile's K* block
// (Npad x 64, the accumulator seeds of every block row) into the tile's workspace and the predictive mean; the training
// points are staged 256 at a time in LDS exactly as in predict_mean_tile_kernel.
template <int D, bool GENERIC>
__global__ void __launch_bounds__(256)
predict_kstar_tile_kernel(const double* __restrict__ Xt, const double* __restrict__ alpha, int N, int Npad,
                          const double* __restrict__ Xs, int d, long long M, DimVec inv_len, double amp, double mean,
                          KernelFn kf, double* __restrict__ ws, double* __restrict__ mu, int TM,
                          double* __restrict__ mu_part, long long mu_stride) {
    __shared__ double xt[D][256];
    __shared__ double al[256];
    __shared__ double part[4][64];
    const int tid = threadIdx.x, c = tid & 63, w = tid >> 6;
    const long long m = (long long)blockIdx.x * 64 + c;
    // gridDim.y > 1: the training points are split into gridDim.y ranges of whole 256-point stages (few query tiles cannot fill
    // the chip otherwise); every range writes its K* rows and its part of the mean sum, predict_var_w_final_kernel adds the parts
    const int stages = (Npad + 255) / 256;
    const int st_lo = (int)((long long)stages * blockIdx.y / gridDim.y), st_hi = (int)((long long)stages * (blockIdx.y + 1) / gridDim.y);
    // 64 queries per workgroup = 64 / TM variance tiles of TM queries, each [Npad][TM] in the workspace
    double* V = ws + ((size_t)blockIdx.x * (64 / TM) + c / TM) * Npad * TM + (c % TM);
    double q[D];
#pragma unroll
    for (int k = 0; k < D; ++k) q[k] = (m < M && k < d) ? Xs[m * d + k] * inv_len.v[k] : 0.0;
    double acc = 0.0;
    for (int n0 = st_lo * 256; n0 < st_hi * 256; n0 += 256) {
        __syncthreads();
        const int n = n0 + tid;
#pragma unroll
        for (int k = 0; k < D; ++k) xt[k][tid] = (n < Npad) ? Xt[(size_t)k * Npad + n] : 0.0;
        al[tid] = (n < Npad) ? alpha[n] : 0.0;
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < 64; ++j) {
            const int nn = w * 64 + j;
            if (n0 + nn >= Npad) break;                    // workgroup-uniform per wave
            double r2 = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double df = xt[k][nn] - q[k];
                r2 = fma(df, df, r2);
            }
            const double kv = (n0 + nn < N) ? amp * radial<GENERIC>(r2, kf) : 0.0;
            acc = fma(kv, al[nn], acc);
            V[(size_t)(n0 + nn) * TM] = kv;
        }
    }
    part[w][c] = acc;
    __syncthreads();
    if (tid < 64 && m < M) {
        const double t = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
        if (gridDim.y == 1) mu[m] = t + mean;
        else mu_part[(size_t)blockIdx.y * mu_stride + m] = t;
    }
}

// One workgroup per CU walks over the tiles of TM queries; tile t owns workspace rows ws[t] (K* seeds in, V out).
// TM = 64 for throughput; TM = 16 when there are too few queries to give every CU a 64-wide tile (a tile's latency is
// its 528 dependent stages at N = 2000, and a 16-wide stage is four times less MFMA work).
template <int TM>
__global__ void __launch_bounds__(512)
predict_var_ws_kernel(const double* __restrict__ L, const double* __restrict__ dinv, int Npad, long long M, double amp,
                      double* __restrict__ ws, double* __restrict__ var, int ident) {
    constexpr int CPW = TM / 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long ntiles = (M + TM - 1) / TM;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        double* V = ws + (size_t)tile * Npad * TM;
        __syncthreads();                       // the previous tile is completely finished with the LDS stages
        // identity right-hand sides (building L^-1): query m is column m, zero above its own block row
        const int kb0 = ident ? (int)((tile * TM) / 64) : 0;
        if (wv >= 4) {
            ws_produce_tile<TM>(L, dinv, Npad, V, kb0);
        } else {
            double ss = ws_consume_tile<TM>(Npad, V, kb0);   // lane (column lane % CPW, row group lane / CPW) of wave wv's columns
#pragma unroll
            for (int off = CPW; off < 64; off <<= 1) ss += __shfl_xor(ss, off, 64);
            const long long mc = tile * TM + CPW * wv + (lane % CPW);
            if (lane < CPW && mc < M) var[mc] = amp - ss;
        }
    }
}

}  // namespace alabi
