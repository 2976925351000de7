// Predictive variance as a product with the cached W = L^-1 (gp_predict.hip: ensure_winv): the tile kernels with one and two
// matrix-core waves per SIMD behind the K* pre-pass (launch_predict_var), and the small-batch kernel that evaluates K* in place
// (launch_predict_var_small).  They stage through ws_As / ws_Vs of predict_var_subst.hpp, which must precede this header.
// Device code only; compiled as part of gp_predict.hip (one translation unit for all predict device code, see there).
#pragma once
#include "predict_var_subst.hpp"

namespace alabi {

// ---------------------------------------------------------------------------------------------------------------
// Variance as a plain product with the cached W = L^-1:  var = amp - colnorm^2(W K*^T).  Same producer / consumer
// pipeline and the same stage sequence (kb, s), s <= kb, as predict_var_ws_kernel, but a stage is now
// acc += W[kb,s] K*_s with NO dependency between stages: nothing waits for a V block, there is no diagonal solve and no
// mid-stage barrier, and the block rows of one query tile can be split over several workgroups (`parts`) when there are
// fewer tiles than CUs.  K* comes from the pre-pass (never overwritten here).  Agrees with the substitution kernels to
// ~1e-14 amp at nugget e^-12 (tools/prof_small_batch.py).
__device__ inline void wg_row_range(int nb, int part, int parts, int& r0, int& r1) {
    // contiguous block rows with about the same number of stages: rows [r0, r1), stages of row r = r + 1
    const long long S = (long long)nb * (nb + 1) / 2;
    auto bound = [&](int p) {
        if (p <= 0) return 0;
        if (p >= parts) return nb;
        const long long target = S * p / parts;
        int r = (int)((sqrt(8.0 * (double)target + 1.0) - 1.0) * 0.5);
        while ((long long)r * (r + 1) / 2 < target) ++r;
        while (r > 0 && (long long)(r - 1) * r / 2 >= target) --r;
        return r < nb ? r : nb;
    };
    r0 = bound(part); r1 = bound(part + 1);
}

__device__ __attribute__((noinline)) void
wg_produce_tile(const double* W_, const double* K_, int Npad, int r0, int r1) {
    const ws_gcptr W = (ws_gcptr)W_, Kst = (ws_gcptr)K_;
    const int t8 = threadIdx.x - 256;          // 256 producer threads: 8 + 8 loads per stage each
    const int prow = t8 >> 2, pch = t8 & 3;
    const long long nst = (long long)r1 * (r1 + 1) / 2 - (long long)r0 * (r0 + 1) / 2;
    if (nst <= 0) return;
    f64x2 pa[2][8], pv[2][8];
#define ALABI_WG_ISSUE(SET, KB, S)                                                                            \
    {                                                                                                         \
        const ws_gcptr2 Wb_ = (ws_gcptr2)(W + (size_t)(S) * Npad * 64 + ((size_t)((KB) * 64 + prow)) * 64) + pch; \
        const ws_gcptr2 Kb_ = (ws_gcptr2)(Kst + ((size_t)((S) * 64 + prow)) * 64) + pch;                      \
        _Pragma("unroll") for (int i = 0; i < 8; ++i) { pa[SET][i] = Wb_[4 * i]; pv[SET][i] = Kb_[4 * i]; }   \
    }
#define ALABI_WG_TO_LDS(SET, BUF)                                                                             \
    {                                                                                                         \
        f64x2* as_ = reinterpret_cast<f64x2*>(&ws_As[BUF][prow][0]) + pch;                                    \
        f64x2* vs_ = reinterpret_cast<f64x2*>(&ws_Vs[BUF][prow][0]) + pch;                                    \
        _Pragma("unroll") for (int i = 0; i < 8; ++i) { as_[4 * i] = pa[SET][i]; vs_[4 * i] = pv[SET][i]; }   \
    }
#define ALABI_WG_ADVANCE(KB, S) { if (++(S) > (KB)) { ++(KB); (S) = 0; } }
    // stage b + 1 sits in set (b + 1) & 1; (k3, s3) is the next stage to issue, clamped to the last one
    int k3 = r0, s3 = 0;
    const int klast = r1 - 1;
    ALABI_WG_ISSUE(0, k3, s3)                  // stage 0
    if (k3 < klast || s3 < k3) ALABI_WG_ADVANCE(k3, s3)
    ALABI_WG_ISSUE(1, k3, s3)                  // stage 1
    ALABI_WG_TO_LDS(0, 0)
    if (k3 < klast || s3 < k3) ALABI_WG_ADVANCE(k3, s3)
    ALABI_WG_ISSUE(0, k3, s3)                  // stage 2
    __syncthreads();                           // stage 0 is in LDS
#define ALABI_WG_STAGE(NSET)                                                                                  \
    {                                                                                                         \
        __syncthreads();               /* stage b is in LDS buffer b & 1; the other buffer is free */         \
        ALABI_WG_TO_LDS(NSET, (int)((b & 1) ^ 1))                                                             \
        if (k3 < klast || s3 < k3) ALABI_WG_ADVANCE(k3, s3)                                                   \
        ALABI_WG_ISSUE(NSET, k3, s3)                                                                          \
        ++b;                                                                                                  \
    }
    long long b = 0;
    // the consumers run one barrier per stage after the first; stage 0 needs none here beyond the one above
    if (nst > 1) {
        // iteration for stage b writes stage b + 1: executed for b = 0 .. nst - 2, preceded by that stage's barrier
        // (stage 0's barrier is the __syncthreads above, so the first iteration skips it)
        ALABI_WG_TO_LDS(1, 1)
        if (k3 < klast || s3 < k3) ALABI_WG_ADVANCE(k3, s3)
        ALABI_WG_ISSUE(1, k3, s3)
        b = 1;
        while (b < nst - 1) {
            ALABI_WG_STAGE(0)
            if (b >= nst - 1) break;
            ALABI_WG_STAGE(1)
        }
        __syncthreads();                       // the barrier of the last stage
    }
#undef ALABI_WG_STAGE
#undef ALABI_WG_ISSUE
#undef ALABI_WG_TO_LDS
#undef ALABI_WG_ADVANCE
}

// Consumer waves: returns this lane's partial sums of squares for its four columns 16 n + lr (rows 16w + lk + 4i).
__device__ __attribute__((noinline)) v4f64
wg_consume_tile(int r0, int r1) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;
    const int lr = lane & 15, lk = lane >> 4;
    v4f64 ss = v4f64{0.0, 0.0, 0.0, 0.0};
    if (r1 <= r0) return ss;
    __syncthreads();                           // stage 0 is in LDS
    v4f64 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = v4f64{0.0, 0.0, 0.0, 0.0};
    long long b = 0;
    for (int kb = r0; kb < r1; ++kb)
        for (int sj = 0; sj <= kb; ++sj, ++b) {
            const int buf = (int)(b & 1);
            if (b > 0) __syncthreads();        // stage b is in LDS buffer buf
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                const double a = ws_As[buf][16 * w + lr][4 * ks + lk];
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const double bb = ws_Vs[buf][4 * ks + lk][16 * n + lr];
                    acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[n], 0, 0, 0);
                }
            }
            if (sj == kb) {
#pragma unroll
                for (int n = 0; n < 4; ++n) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) ss[n] = fma(acc[n][i], acc[n][i], ss[n]);
                    acc[n] = v4f64{0.0, 0.0, 0.0, 0.0};
                }
            }
        }
    return ss;
}

// grid = (tiles in flight, parts); partial[(tile * parts + part) * 64 + column]
__global__ void __launch_bounds__(512)
predict_var_w_kernel(const double* __restrict__ W, const double* __restrict__ Kst, int Npad, long long ntiles, int parts,
                     double* __restrict__ partial) {
    __shared__ double red[4][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lk = lane >> 4;
    const int nb = Npad / 64, part = blockIdx.y;
    int r0, r1;
    wg_row_range(nb, part, parts, r0, r1);
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const double* K = Kst + (size_t)tile * Npad * 64;
        __syncthreads();                       // the previous tile is completely finished with the LDS stages
        if (wv >= 4) {
            wg_produce_tile(W, K, Npad, r0, r1);
        } else {
            v4f64 ss = wg_consume_tile(r0, r1);
#pragma unroll
            for (int n = 0; n < 4; ++n) {      // over the row groups lk, then over the four waves (rows 16w ..)
                ss[n] += __shfl_xor(ss[n], 16, 64);
                ss[n] += __shfl_xor(ss[n], 32, 64);
                if (lk == 0) red[wv][16 * n + lr] = ss[n];
            }
        }
        __syncthreads();
        if (tid < 64) partial[((size_t)tile * parts + part) * 64 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The same product with TWO matrix-core waves per SIMD: 128 queries per workgroup (two neighbouring 64-query K* tiles),
// eight consumer waves (row group c & 3, query half c >> 2: waves c and c + 4 share a SIMD and cover each other's LDS
// latency and barrier waits) and four producer waves.  A stage is half a 64 x 64 block of W (32 columns) against 32 rows
// of both K* tiles, so the LDS holds 2 x (64 x 33 + 32 x 144) doubles = 108 KB and every byte of W read from L2 / HBM feeds
// twice as many queries as in predict_var_w_kernel.  The accumulation order per output is unchanged (k ascending inside
// a block, blocks s ascending), so both kernels return the same bits.  tools/micro/mfma_f64_rate: 66-70 TFLOP/s with two
// MFMA waves per SIMD against 56-59 with one.
__shared__ double w2_As[2][64][33];
__shared__ double w2_Vs[2][32][144];

// Uniform values arrive in VGPRs through the call ABI of a noinline function: readfirstlane moves them back to SGPRs so
// that the stage counters, the address arithmetic and the loop branches are scalar.
__device__ inline const double* w2_uniform_ptr(const double* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (const double*)(((unsigned long long)hi << 32) | lo);
}

__device__ __attribute__((noinline)) void
w2_produce_tile(const double* W_, const double* K0_, const double* K1_, int Npad, int r0, int r1) {
    const ws_gcptr W = (ws_gcptr)w2_uniform_ptr(W_), K0 = (ws_gcptr)w2_uniform_ptr(K0_), K1 = (ws_gcptr)w2_uniform_ptr(K1_);
    Npad = __builtin_amdgcn_readfirstlane(Npad); r0 = __builtin_amdgcn_readfirstlane(r0); r1 = __builtin_amdgcn_readfirstlane(r1);
    const int t8 = threadIdx.x - 512;          // 256 producer threads
    const int wrow = t8 >> 2, wch = t8 & 3;    // W: row of the block, 8 of its 32 columns (4 x 16-byte loads)
    const int krow = t8 >> 3, kch = t8 & 7;    // K*: row of the 32, 8 of the 64 queries of each tile (4 + 4 loads)
    const long long nst = 2 * ((long long)r1 * (r1 + 1) / 2 - (long long)r0 * (r0 + 1) / 2);
    if (nst <= 0) return;
    f64x2 pw[2][4], pk[2][8];
    int kb = r0, sj = 0, hf = 0;               // the next stage to issue; stays on the last stage once it is reached, so
    const int klast = r1 - 1;                  // that the issue is unconditional (straight-line code keeps vmcnt exact:
                                               // the wait before a set is written leaves the other set's loads in flight)
    const size_t wlane = (size_t)wrow * 64 + 8 * wch, klane = (size_t)krow * 64 + 8 * kch;
#define ALABI_W2_ISSUE(SET)                                                                                          \
    {                                                                                                                \
        const ws_gcptr2 Wb_ = (ws_gcptr2)(W + ((size_t)sj * Npad + (size_t)kb * 64) * 64 + 32 * hf + wlane);         \
        const size_t ko_ = ((size_t)(sj * 64 + 32 * hf)) * 64 + klane;                                               \
        const ws_gcptr2 Ka_ = (ws_gcptr2)(K0 + ko_), Kb_ = (ws_gcptr2)(K1 + ko_);                                    \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) { pw[SET][i] = Wb_[i]; pk[SET][i] = Ka_[i]; pk[SET][4 + i] = Kb_[i]; } \
        const int adv_ = (kb < klast || sj < kb || hf == 0) ? 1 : 0;                                                 \
        const int nh_ = hf ^ adv_, carry_ = adv_ & hf;                                                               \
        const int wrap_ = carry_ & (sj >= kb ? 1 : 0);                                                               \
        hf = nh_; sj = wrap_ ? 0 : sj + carry_; kb += wrap_;                                                         \
    }
#define ALABI_W2_TO_LDS(SET)                                                                                         \
    {                                                                                                                \
        double* as_ = &w2_As[SET][wrow][8 * wch];                                                                    \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) { as_[2 * i] = pw[SET][i][0]; as_[2 * i + 1] = pw[SET][i][1]; } \
        f64x2* va_ = reinterpret_cast<f64x2*>(&w2_Vs[SET][krow][8 * kch]);                                           \
        f64x2* vb_ = reinterpret_cast<f64x2*>(&w2_Vs[SET][krow][64 + 8 * kch]);                                      \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) { va_[i] = pk[SET][i]; vb_[i] = pk[SET][4 + i]; }              \
    }
    // Step j (after barrier #j, while the consumers work on stage j): stage j + 1 goes from register set (j + 1) & 1 to LDS
    // buffer (j + 1) & 1 -- free since barrier #j -- and the set is refilled with stage j + 3; then barrier #(j + 1).
    // Two steps per loop iteration with no branch between them: the wait before a set is written is vmcnt(12), the other
    // set's twelve loads stay in flight across the barrier.
#define ALABI_W2_STEP(SET) { ALABI_W2_TO_LDS(SET) ALABI_W2_ISSUE(SET) __syncthreads(); }
    ALABI_W2_ISSUE(0)                          // stage 0
    ALABI_W2_ISSUE(1)                          // stage 1
    ALABI_W2_TO_LDS(0)
    ALABI_W2_ISSUE(0)                          // stage 2
    __syncthreads();                           // barrier #0: stage 0 is in LDS
    long long j = 0;
    for (; j + 2 <= nst - 1; j += 2) {
        ALABI_W2_STEP(1)
        ALABI_W2_STEP(0)
    }
    if (j < nst - 1) ALABI_W2_STEP(1)
#undef ALABI_W2_TO_LDS
#undef ALABI_W2_STEP
#undef ALABI_W2_ISSUE
}

// Consumer wave c: rows 32 (c & 1) .. +31 of the block row (two 16-row groups), queries 32 (c >> 1) .. +31 (two 16-query
// groups): two A and two B operands feed four MFMAs per k-step (1.0 LDS read per MFMA instead of 1.25 for a 16 x 64
// wave tile -- the LDS bandwidth, not the matrix cores, is the tighter budget with eight consumer waves).  Returns the
// partial sums of squares ss[2 ri + n] of row group ri, query group n (rows lk + 4 i of the row group), accumulated in
// the same order as predict_var_w_kernel does for its row group 2 (c & 1) + ri.
__device__ __attribute__((noinline)) v4f64
w2_consume_tile(int r0, int r1) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int c = __builtin_amdgcn_readfirstlane(tid >> 6) & 7;
    r0 = __builtin_amdgcn_readfirstlane(r0); r1 = __builtin_amdgcn_readfirstlane(r1);
    const int row0 = 32 * (c & 1), q0 = 32 * (c >> 1);
    const int lr = lane & 15, lk = lane >> 4;
    v4f64 ss = v4f64{0.0, 0.0, 0.0, 0.0};
    v4f64 acc[2][2];
#pragma unroll
    for (int ri = 0; ri < 2; ++ri)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[ri][n] = v4f64{0.0, 0.0, 0.0, 0.0};
    int buf = 0;
    for (int kb = r0; kb < r1; ++kb)
        for (int sj = 0; sj <= kb; ++sj)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                __syncthreads();               // this stage is in LDS buffer buf
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) {
                    const double a0 = w2_As[buf][row0 + lr][4 * ks + lk], a1 = w2_As[buf][row0 + 16 + lr][4 * ks + lk];
                    const double b0 = w2_Vs[buf][4 * ks + lk][q0 + lr], b1 = w2_Vs[buf][4 * ks + lk][q0 + 16 + lr];
                    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
                }
                buf ^= 1;
                if (sj == kb && hf == 1) {
#pragma unroll
                    for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                        for (int n = 0; n < 2; ++n) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) ss[2 * ri + n] = fma(acc[ri][n][i], acc[ri][n][i], ss[2 * ri + n]);
                            acc[ri][n] = v4f64{0.0, 0.0, 0.0, 0.0};
                        }
                }
            }
    return ss;
}

// grid = (groups of two K* tiles in flight, parts); partial[(tile * parts + part) * 64 + column] as predict_var_w_kernel
__global__ void __launch_bounds__(768)
predict_var_w2_kernel(const double* __restrict__ W, const double* __restrict__ Kst, int Npad, long long ntiles, int parts,
                      double* __restrict__ partial) {
    __shared__ double red[4][128];             // [row group of the block row][query of the 128]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lk = lane >> 4;
    const int nb = Npad / 64, part = blockIdx.y;
    int r0, r1;
    wg_row_range(nb, part, parts, r0, r1);
    const long long ngroups = (ntiles + 1) / 2;
    for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const long long t0 = 2 * g, t1 = (2 * g + 1 < ntiles) ? 2 * g + 1 : t0;    // an odd last tile is paired with itself
        __syncthreads();                       // the previous group is completely finished with the LDS stages
        if (wv >= 8) {
            w2_produce_tile(W, Kst + (size_t)t0 * Npad * 64, Kst + (size_t)t1 * Npad * 64, Npad, r0, r1);
        } else {
            v4f64 ss = w2_consume_tile(r0, r1);
#pragma unroll
            for (int q = 0; q < 4; ++q) {      // q = 2 ri + n
                ss[q] += __shfl_xor(ss[q], 16, 64);
                ss[q] += __shfl_xor(ss[q], 32, 64);
                if (lk == 0) red[2 * (wv & 1) + (q >> 1)][32 * (wv >> 1) + 16 * (q & 1) + lr] = ss[q];
            }
        }
        __syncthreads();
        if (tid < 128) {
            const long long tile = 2 * g + (tid >> 6);
            if (tile < ntiles)
                partial[((size_t)tile * parts + part) * 64 + (tid & 63)] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        }
    }
}

__global__ void __launch_bounds__(256)
predict_var_w_final_kernel(const double* __restrict__ partial, int parts, long long M, double amp, double* __restrict__ var,
                           const double* __restrict__ mu_part, int nsplit, long long mu_stride, double mean, double* __restrict__ mu) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const double* p = partial + (size_t)(m / 64) * parts * 64 + (m % 64);
    double s = 0.0;
    for (int k = 0; k < parts; ++k) s += p[(size_t)k * 64];
    var[m] = amp - s;
    if (nsplit > 1) {                                      // the mean sum arrived in nsplit ranges of training points
        double t = 0.0;
        for (int k = 0; k < nsplit; ++k) t += mu_part[(size_t)k * mu_stride + m];
        mu[m] = t + mean;
    }
}

// Variance of at most 16 queries from the cached W = L^-1: v = W k*, var = amp - |v|^2.  One workgroup per block row kb
// forms v_kb = sum_{j <= kb} W[kb,j] K*_j on the matrix cores (the K* blocks are re-evaluated per workgroup: 64 x 16
// kernel values per block) and leaves its 16 partial sums of squares; a second tiny kernel adds them in block order.
template <int D, bool GENERIC>
__global__ void __launch_bounds__(256)
predict_var_small_kernel(const double* __restrict__ W, const double* __restrict__ Xt, int N, int Npad,
                         const double* __restrict__ Xs, int d, int M, DimVec inv_len, double amp, KernelFn kf,
                         double* __restrict__ partial) {
    __shared__ double Wt[64][66];
    __shared__ double Ks[64][18];
    __shared__ double qs[16][D];
    __shared__ double red[4][16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int kb = blockIdx.x;
    // blockIdx.y selects a group of 16 queries (up to 512 queries go through this kernel: one round of nb x groups
    // workgroups costs less than the K* pre-pass of the tile kernels, which only fills M / 64 CUs)
    Xs += (size_t)blockIdx.y * 16 * d;
    M -= (int)blockIdx.y * 16;
    if (M > 16) M = 16;
    for (int e = tid; e < 16 * D; e += 256) {
        const int m = e / D, k = e % D;
        qs[m][k] = (m < M && k < d) ? Xs[(size_t)m * d + k] * inv_len.v[k] : 0.0;
    }
    v4f64 acc = v4f64{0.0, 0.0, 0.0, 0.0};
    // Block j + 1 (its W tile and the training coordinates of its 64 points) is requested while block j is multiplied: the
    // loop is a chain of kb + 1 dependent stages and a global round trip per stage would dominate it.  The request is
    // unconditional (the last block is simply asked for again) so that the waits stay counted.
    f64x2 wreg[8];
    double x[D];
#define ALABI_SMALL_REQUEST(J)                                                                               \
    {                                                                                                        \
        const f64x2* Wb_ = reinterpret_cast<const f64x2*>(W + (size_t)(J) * Npad * 64 + (size_t)(kb * 64) * 64); \
        _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) wreg[e_] = Wb_[tid + 256 * e_];                     \
        _Pragma("unroll") for (int k = 0; k < D; ++k) x[k] = Xt[(size_t)k * Npad + (J) * 64 + lane];         \
    }
    ALABI_SMALL_REQUEST(0)
    for (int j = 0; j <= kb; ++j) {
        __syncthreads();                                   // the previous block's MFMAs are done with Wt / Ks (and qs is set)
#pragma unroll
        for (int e_ = 0; e_ < 8; ++e_) {
            const int e = tid + 256 * e_;
            *reinterpret_cast<f64x2*>(&Wt[e >> 5][2 * (e & 31)]) = wreg[e_];
        }
        {   // K*_j: thread (point p = lane, queries 4w .. 4w+3)
            const int n = j * 64 + lane;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = 4 * w + i;
                double r2 = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) { const double df = x[k] - qs[m][k]; r2 = fma(df, df, r2); }
                Ks[lane][m] = (n < N && m < M) ? amp * radial<GENERIC>(r2, kf) : 0.0;
            }
        }
        const int jn = (j < kb) ? j + 1 : kb;
        ALABI_SMALL_REQUEST(jn)
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 16; ++ks)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Wt[16 * w + lr][4 * ks + lk], Ks[4 * ks + lk][lr], acc, 0, 0, 0);
    }
#undef ALABI_SMALL_REQUEST
    // acc[i] = v[row 16w + lk + 4i][query lr]: squares summed over the rows of this wave, then over the waves
    double ss = fma(acc[0], acc[0], fma(acc[1], acc[1], fma(acc[2], acc[2], acc[3] * acc[3])));
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    if (lane < 16) red[w][lane] = ss;
    __syncthreads();
    if (tid < 16) partial[((size_t)blockIdx.y * gridDim.x + kb) * 16 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

__global__ void __launch_bounds__(64)
predict_var_small_final_kernel(const double* __restrict__ partial, int nb, int M, double amp, double* __restrict__ var) {
    const int m = blockIdx.x * 64 + threadIdx.x;           // query; group m / 16, slot m % 16
    if (m >= M) return;
    const double* pg = partial + (size_t)(m >> 4) * nb * 16 + (m & 15);
    double s = 0.0;
    for (int kb = 0; kb < nb; ++kb) s += pg[(size_t)kb * 16];
    var[m] = amp - s;
}

}  // namespace alabi
