// Device helpers of ens_map.hip: the second derivatives of the ensemble's fused log-probability and the small wave-0 products of
// the dense BFGS optimiser.  ens_grad_device.hpp is included read-only: nothing of the HMC kernels is instantiated differently.
#pragma once
#include "ens_grad_device.hpp"

namespace alabi {

// f(r2), f'(r2) and f''(r2) of the four radial families; value and slope as radial_value_slope writes them.
//   squared exponential f / 4;  Matern-3/2 (9/4) e^-s / s, s = sqrt(3 r2);  Matern-5/2 (25/12) e^-s, s = sqrt(5 r2);
//   rational quadratic (a + 1) / (4 a) (1 + u)^(-a - 2), u = r2 / (2 a).
// Matern-3/2 at r2 = 0: f'' is unbounded while f'' d_a d_b tends to 0, and a query may sit on a training point, so d2f = 0 there.
template <bool GENERIC>
__device__ inline void radial_value_slope_curv(double r2, const KernelFn& kf, double& f, double& df, double& d2f) {
    if (!GENERIC || kf.type == 0) { f = exp_neg_half(r2); df = -0.5 * f; d2f = 0.25 * f; return; }
    if (kf.type == 1) {
        const double r = sqrt(3.0 * r2), e = exp(-r);
        f = (1.0 + r) * e; df = -1.5 * e; d2f = r2 > 0.0 ? 2.25 * e / r : 0.0; return;
    }
    if (kf.type == 2) {
        const double r = sqrt(5.0 * r2), e = exp(-r);
        f = (1.0 + r + r * r / 3.0) * e; df = -(5.0 / 6.0) * (1.0 + r) * e; d2f = (25.0 / 12.0) * e; return;
    }
    const double u = 0.5 * r2 / kf.alpha, opu = 1.0 + u;
    f = exp(-kf.alpha * log1p(u));
    df = -0.5 * f / opu;
    d2f = (kf.alpha + 1.0) / (4.0 * kf.alpha) * f / (opu * opu);
}

// index of the pair (a, b), a <= b < d, in the row-major upper triangle
__device__ __forceinline__ int hess_pair_index(int a, int b, int d) { return a * d - a * (a - 1) / 2 + (b - a); }

// The sums behind the Hessian of the GP mean at ONE point, by the whole workgroup (any multiple of 64 lanes).  With s the scaled
// coordinates, dl = s_q - s_n, r2 = |dl|^2 and k = amp f(r2):
//     d2 mu / dx_a dx_b = amp inv_a inv_b sum_n alpha_n [4 f''(r2_n) dl_na dl_nb + 2 f'(r2_n) 1(a = b)]
//   pass A: a lane takes the points tid, tid + T, ...: r2, the value term alpha f, and the weights u1 = 2 alpha f' and
//           u2 = 4 alpha f'', which go to LDS;
//   pass B: the d (d + 1) / 2 pairs a <= b and then the d gradient sums are dealt over the waves, lanes along n (contiguous reads of
//           rows a and b of Xt), one DPP reduction per item: S_ab = sum_n [(u2_n dl_na) dl_nb + u1_n 1(a = b)], G_a = sum_n u1_n dl_na.
//           The difference is formed per point, never as sum u x x - ...: inputs far from the origin would cancel.
// Lane k < d of wave 0 passes coordinate k of the point and its 1 / length scale.  Leaves S [d (d + 1) / 2] and G [d] in LDS and the
// wave partials of sum_n alpha_n f in scratch [T / 64]; ends with a barrier, after which every thread may read them.  Every sum runs
// in a fixed order.  LDS: u1_s and u2_s [Npad] each, qs_s [64], S_s [d (d + 1) / 2], G_s [64], scratch [16].
template <int D, bool GENERIC>
__device__ __forceinline__ void lp_hess_eval(const LpGradArgs& a, double* u1_s, double* u2_s, double* qs_s, double* S_s, double* G_s,
                                             double* scratch, double qc, double inv_len) {
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = T >> 6, d = a.d;
    if (tid < D) qs_s[tid] = (tid < d) ? qc * inv_len : 0.0;
    __syncthreads();
    {
        double q[D];
#pragma unroll
        for (int k = 0; k < D; ++k) q[k] = qs_s[k];
        double val = 0.0;
        for (int n = tid; n < a.Npad; n += T) {
            double r2 = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double df = q[k] - a.Xt[(size_t)k * a.Npad + n];
                r2 = fma(df, df, r2);
            }
            double f, fp, fpp;
            radial_value_slope_curv<GENERIC>(r2, a.kf, f, fp, fpp);
            const double al = a.alpha[n];
            val = fma(al, f, val);
            u1_s[n] = 2.0 * al * fp;
            u2_s[n] = 4.0 * al * fpp;
        }
        const double ws = wave_sum_dpp(val);
        if (lane == 63) scratch[wv] = ws;
    }
    __syncthreads();
    const int npairs = d * (d + 1) / 2;
    for (int i = wv; i < npairs + d; i += nw) {   // wave-uniform
        int ka = 0, kb = 0;
        const bool pair = i < npairs;
        if (pair) {
            int rem = i;
            while (rem >= d - ka) { rem -= d - ka; ++ka; }
            kb = ka + rem;
        } else {
            ka = kb = i - npairs;
        }
        const double* xa = a.Xt + (size_t)ka * a.Npad;
        const double* xb = a.Xt + (size_t)kb * a.Npad;
        const double qa = qs_s[ka], qb = qs_s[kb];
        double s = 0.0;
        if (pair) {
            const bool diag = ka == kb;
            for (int n = lane; n < a.Npad; n += 64) {
                double t = (u2_s[n] * (qa - xa[n])) * (qb - xb[n]);
                if (diag) t += u1_s[n];
                s += t;
            }
        } else {
            for (int n = lane; n < a.Npad; n += 64) s = fma(u1_s[n], qa - xa[n], s);
        }
        s = wave_sum_dpp(s);
        if (lane == 63) { if (pair) S_s[i] = s; else G_s[ka] = s; }
    }
    __syncthreads();
}

// ---- wave-0 helpers of the optimiser: the 64 lanes of one wave together, lane k coordinate k (lanes >= d pass zeros)
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}
// (B v)_k = sum_j B[k][j] v_j, j ascending, by fma from 0: a lane reads its own row of B (row stride ld) and nothing else
__device__ __forceinline__ double bfgs_row_times(const double* Bs, int d, int ld, int lane, double v) {
    double s = 0.0;
    for (int j = 0; j < d; ++j) {
        const double vj = lane_bcast(v, j);
        if (lane < d) s = fma(Bs[lane * ld + j], vj, s);
    }
    return s;
}
__device__ __forceinline__ void bfgs_row_diagonal(double* Bs, int d, int ld, int lane, double v) {
    if (lane < d)
        for (int j = 0; j < d; ++j) Bs[lane * ld + j] = (j == lane) ? v : 0.0;
}

}  // namespace alabi
