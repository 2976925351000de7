// Predictive mean mu* = k(X*,X) alpha + m: the vector kernels and the matrix-core kernel (launch_predict_mean, gp_predict.hip).
//
// mean, small M  : one workgroup per query, lanes along the training points (the same device
//                  function the ensemble sampler uses for a walker's log-probability).
// mean, large M  : 64 queries per workgroup, lanes along queries (no cross-lane reduction);
//                  256 training points at a time staged in LDS and broadcast to the lanes.
//                  Bound by the fp64 vector/transcendental rate: N (2d+2) flops + N exp per
//                  query, ~8(d+1) bytes of HBM per query.
// matrix cores   : from 2048 queries on (d + 2 <= 32), see the note in front of xa_centre_kernel below.
// Device code only; compiled as part of gp_predict.hip (one translation unit for all predict device code, see there).
#pragma once
#include "gp_device.hpp"

namespace alabi {

typedef double v4f64 __attribute__((ext_vector_type(4)));

template <int D>
__global__ void __launch_bounds__(256)
predict_mean_rowwise_kernel(const double* __restrict__ Xt, const double* __restrict__ alpha, int Npad,
                            const double* __restrict__ Xs, int d, DimVec inv_len, double amp, double mean,
                            KernelFn kf, double* __restrict__ mu) {
    __shared__ double q[ALABI_MAX_DIM];
    __shared__ double scratch[16];
    const long long m = blockIdx.x;
    if (threadIdx.x < D) q[threadIdx.x] = (threadIdx.x < d) ? Xs[m * d + threadIdx.x] * inv_len.v[threadIdx.x] : 0.0;
    __syncthreads();
    double s = gp_kernel_dot_block<D>(Xt, alpha, Npad, q, scratch, kf);
    if (threadIdx.x == 0) mu[m] = fma(amp, s, mean);
}

template <int D, bool GENERIC>
__global__ void __launch_bounds__(256)
predict_mean_tile_kernel(const double* __restrict__ Xt, const double* __restrict__ alpha, int Npad,
                         const double* __restrict__ Xs, int d, long long M, DimVec inv_len, double amp,
                         double mean, KernelFn kf, double* __restrict__ mu, double* __restrict__ mu_part, long long mu_stride) {
    __shared__ double xt[D][256];
    __shared__ double al[256];
    __shared__ double part[4][64];
    __shared__ double etab[32];                                  // 2^(j/32) for exp_tab32 (first barrier of the loop orders it)
    const int tid = threadIdx.x, c = tid & 63, w = tid >> 6;
    if (tid < 32) etab[tid] = exp2((double)tid * 0.03125);
    const long long m = (long long)blockIdx.x * 64 + c;
    double q[D];
#pragma unroll
    for (int k = 0; k < D; ++k) q[k] = (m < M && k < d) ? Xs[m * d + k] * inv_len.v[k] : 0.0;
    double acc = 0.0;
    // gridDim.y > 1: whole 256-point stages of the training set are dealt to gridDim.y workgroups per query tile (too few
    // tiles to fill the chip otherwise); mean_combine_kernel adds the parts in order
    const int stages = (Npad + 255) / 256;
    const int st_lo = (int)((long long)stages * blockIdx.y / gridDim.y), st_hi = (int)((long long)stages * (blockIdx.y + 1) / gridDim.y);
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
            double r2 = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                double df = xt[k][nn] - q[k];
                r2 = fma(df, df, r2);
            }
            acc = fma(al[nn], GENERIC ? radial<true>(r2, kf) : exp_tab32(-0.5 * r2, etab), acc);
        }
    }
    part[w][c] = acc;
    __syncthreads();
    if (tid < 64 && m < M) {
        const double t = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
        if (gridDim.y == 1) mu[m] = fma(amp, t, mean);
        else mu_part[(size_t)blockIdx.y * mu_stride + m] = t;
    }
}

__global__ void __launch_bounds__(256)
mean_combine_kernel(const double* __restrict__ mu_part, int nsplit, long long mu_stride, long long M, double amp, double mean,
                    double* __restrict__ mu) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    double t = 0.0;
    for (int k = 0; k < nsplit; ++k) t += mu_part[(size_t)k * mu_stride + m];
    mu[m] = fma(amp, t, mean);
}

// ---- predict-mean with the dot products on the matrix cores (large batches) -------------------------------------
// mu*(q) = amp sum_n alpha_n f(r2(q, x_n)) + m (reference call sites alabi/core.py:85, :1812).  With the rows
// x' = (x, -|x|^2/2, 1) and q' = (q, 1, -|q|^2/2) the product q'.x' IS -r2/2, the argument of the squared-exponential:
// v_mfma_f64_16x16x4 forms it for 16 queries x 16 training points per instruction (ceil((d+2)/4) of them per tile) while the
// vector unit only evaluates exp and the alpha FMA -- 21 instead of 41 fp64 VALU instructions per kernel evaluation, and
// the two pipes run side by side.  One wavefront owns 64 queries (four 16-row A operands kept in registers) and walks over
// the training points 16 at a time (B operand and alpha: one double per lane per k-step, L2-resident); a lane ends with
// the partial sums of 16 queries over its point column, folded across the 16 lanes of its row with DPP adds.
// Centre of the scaled training inputs, one workgroup per dimension: r2 is translation invariant, and the augmented dot
// product q'.x' = q.x - |x|^2/2 - |q|^2/2 loses eps * (|x|^2 + |q|^2) / 2 absolutely, so both sides are taken relative to the
// training mean (inputs that sit thousands of length scales from the origin would otherwise cost digits of the exponent).
__global__ void __launch_bounds__(256)
xa_centre_kernel(const double* __restrict__ Xt, int Npad, int N, double* __restrict__ centre) {
    __shared__ double scratch[16];
    const int k = blockIdx.x;
    double t = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) t += Xt[(size_t)k * Npad + n];
    t = block_sum(t, scratch);
    if (threadIdx.x == 0) centre[k] = t / (double)N;
}

__global__ void __launch_bounds__(256)
build_xa_kernel(const double* __restrict__ Xt, int Npad, int d, int rows, const double* __restrict__ centre,
                double* __restrict__ Xa) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= Npad) return;
    double xx = 0.0;
    for (int k = 0; k < d; ++k) {
        const double v = Xt[(size_t)k * Npad + n] - centre[k];
        Xa[(size_t)k * Npad + n] = v;
        xx = fma(v, v, xx);
    }
    Xa[(size_t)d * Npad + n] = -0.5 * xx;
    Xa[(size_t)(d + 1) * Npad + n] = 1.0;
    for (int k = d + 2; k < rows; ++k) Xa[(size_t)k * Npad + n] = 0.0;
}

template <int KS, bool GENERIC>
__global__ void __launch_bounds__(256)
predict_mean_mfma_kernel(const double* __restrict__ Xa, const double* __restrict__ alpha, int Npad,
                         const double* __restrict__ Xs, int d, long long M, DimVec inv_len, const double* __restrict__ centre,
                         double amp, double mean, KernelFn kf, double* __restrict__ mu, double* __restrict__ mu_part, long long mu_stride,
                         int pts_per_part) {
    __shared__ double etab[256];                                 // 2^(j/256) for exp2s_tab256
    etab[threadIdx.x] = exp2((double)threadIdx.x * 0.00390625);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // squared exponential: the query operand carries the factor 256 / ln2, so the product arrives as the argument of 2^(./256)
    const double qs = GENERIC ? 1.0 : ALABI_EXP2S256_SCALE;
    const int lr = lane & 15, lk = lane >> 4;
    const long long q0 = ((long long)blockIdx.x * 4 + wv) * 64;
    if (q0 >= M) return;
    // A operands: query row lr of tile qt, coordinate 4 s + lk of k-step s (the augmented row q' = (q / l - c, 1, -|q / l - c|^2 / 2),
    // c = centre of the scaled training inputs, the same shift build_xa_kernel applied to the rows of Xa)
    double a[4][KS];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
        const long long m = q0 + 16 * qt + lr;
        const bool valid = m < M;
        double qq = 0.0;
        for (int k = 0; k < d; ++k) {
            const double v = valid ? Xs[m * d + k] * inv_len.v[k] - centre[k] : 0.0;
            qq = fma(v, v, qq);
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int c = 4 * s + lk;
            double v = 0.0;
            if (valid) v = (c < d) ? Xs[m * d + c] * inv_len.v[c] - centre[c] : (c == d) ? 1.0 : (c == d + 1) ? -0.5 * qq : 0.0;
            a[qt][s] = v * qs;
        }
    }
    double sum[4][4];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt)
#pragma unroll
        for (int i = 0; i < 4; ++i) sum[qt][i] = 0.0;
    const double* xb = Xa + (size_t)lk * Npad + lr;       // B operand: point column lr of the tile, coordinate 4 s + lk
    // gridDim.y > 1 (medium batches: too few 256-query workgroups to fill the chip): the training points are dealt to gridDim.y
    // workgroups per query block in runs of pts_per_part (a multiple of 16); mean_combine_kernel adds the parts in order
    const int n_lo = blockIdx.y * pts_per_part, n_hi = (n_lo + pts_per_part < Npad) ? n_lo + pts_per_part : Npad;
    for (int n0 = n_lo; n0 < n_hi; n0 += 16) {
        double b[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) b[s] = xb[(size_t)(4 * s) * Npad + n0];
        const double al = alpha[n0 + lr];
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            v4f64 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[qt][s], b[s], acc, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {                 // C/D layout: row (query) lk + 4 i, column (point) lr
                const double f = GENERIC ? radial<true>(fmax(-2.0 * acc[i], 0.0), kf) : exp2s_tab256(acc[i], etab);
                sum[qt][i] = fma(al, f, sum[qt][i]);
            }
        }
    }
    // fold the 16 point columns of every query: the 16 lanes of a DPP row share lk
#pragma unroll
    for (int qt = 0; qt < 4; ++qt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double v = sum[qt][i];
            v += dpp_move<0x111, 0xf>(v);
            v += dpp_move<0x112, 0xf>(v);
            v += dpp_move<0x114, 0xf>(v);
            v += dpp_move<0x118, 0xf>(v);
            const long long m = q0 + 16 * qt + lk + 4 * i;
            if (lr == 15 && m < M) {
                if (mu_part) mu_part[(size_t)blockIdx.y * mu_stride + m] = v;
                else mu[m] = fma(amp, v, mean);
            }
        }
}

}  // namespace alabi
