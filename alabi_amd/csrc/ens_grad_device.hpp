// Device helpers of the gradient-based ensemble kernels (ens_hmc.hip): the fused value and gradient of the ensemble's
// log-probability, and the products with a move's scale factor that the leapfrog integrator needs.  Nothing here is instantiated by
// the red-blue or Metropolis kernels: ens_device.hpp, ens_stream.hpp and gp_device.hpp are included read-only.
#pragma once
#include "ens_device.hpp"

namespace alabi {

// f(r2) and f'(r2) of the four radial families (gp_device.hpp: radial; the slopes are those of gp_predict_grad.hip)
template <bool GENERIC>
__device__ inline void radial_value_slope(double r2, const KernelFn& kf, double& f, double& df) {
    if (!GENERIC || kf.type == 0) { f = exp_neg_half(r2); df = -0.5 * f; return; }
    if (kf.type == 1) { const double r = sqrt(3.0 * r2), e = exp(-r); f = (1.0 + r) * e; df = -1.5 * e; return; }
    if (kf.type == 2) {
        const double r = sqrt(5.0 * r2), e = exp(-r);
        f = (1.0 + r + r * r / 3.0) * e; df = -(5.0 / 6.0) * (1.0 + r) * e; return;
    }
    const double u = 0.5 * r2 / kf.alpha;
    f = exp(-kf.alpha * log1p(u));
    df = -0.5 * f / (1.0 + u);
}

// What the value-and-gradient evaluation reads of the ensemble and its GP.
struct LpGradArgs {
    const double* Xt;            // [D, Npad] scaled inputs, coordinate-major (rows beyond d are zero)
    const double* alpha;         // [Npad], zero in the padding
    const double* consts;        // device [5][ALABI_MAX_DIM]: inv_len, lo, hi, prior mean, prior 1 / std
    int d, Npad, has_prior, ymap;
    double prior_const, amp, mean;   // amp, mean: the affine map of the log-probability folded in (ens_run.hip: base_args)
    KernelFn kf;
};

// lnp and its gradient at ONE point, by the whole workgroup (any multiple of 64 lanes): the ensemble's log-probability WITHOUT the
// box gate -- GP mean through the folded scalers, the y map, the normal priors.  Lane k < d of wave 0 passes coordinate k of the
// point (qc) and its 1 / length scale; wave 0 gets lp in every lane and d lnp / d q_k in lane k (0 in lanes >= d); what the other
// waves get means nothing.  Three barriers; every thread of the workgroup must call it.
//   pass A: a lane takes the points tid, tid + T, ...: r2, the value term alpha f and the weight w = -2 alpha f'(r2), which goes to
//           LDS (squared exponential: w = alpha k);
//   pass B: wave v takes the coordinates v, v + T / 64, ...: sum_n w_n (x_nk - q_k), lanes along n (contiguous reads of row k of
//           Xt), one DPP reduction per coordinate.  The difference is formed per point, not as sum w x - q sum w: inputs far from
//           the origin would cancel there.
// Every sum runs in a fixed order, so a point gives the same bits whenever and wherever it is evaluated.
// LDS: w_s [Npad], qs_s and g_s [64], scratch [16].
template <int D, bool GENERIC>
__device__ __forceinline__ void lp_grad_eval(const LpGradArgs& a, double* w_s, double* qs_s, double* g_s, double* scratch, double qc,
                                             double inv_len, double& lp, double& grad) {
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
                const double df = a.Xt[(size_t)k * a.Npad + n] - q[k];
                r2 = fma(df, df, r2);
            }
            double f, fp;
            radial_value_slope<GENERIC>(r2, a.kf, f, fp);
            const double al = a.alpha[n];
            val = fma(al, f, val);
            w_s[n] = -2.0 * al * fp;
        }
        const double ws = wave_sum_dpp(val);
        if (lane == 63) scratch[wv] = ws;
    }
    __syncthreads();
    for (int k = wv; k < d; k += nw) {   // wave-uniform
        const double* xr = a.Xt + (size_t)k * a.Npad;
        const double qk = qs_s[k];
        double s = 0.0;
        for (int n = lane; n < a.Npad; n += 64) s = fma(w_s[n], xr[n] - qk, s);
        s = wave_sum_dpp(s);
        if (lane == 63) g_s[k] = s;
    }
    __syncthreads();
    lp = 0.0; grad = 0.0;
    if (tid >= 64) return;
    double part = (lane < nw) ? scratch[lane] : 0.0;
    part = wave_sum_dpp(part);
    const double mu = fma(a.amp, lane_bcast(part, 63), a.mean);
    const bool in = lane < d;
    double gk = in ? a.amp * inv_len * g_s[lane] : 0.0;
    lp = mu;
    if (a.ymap) {                        // L = -+10^mu: dL = ln10 L dmu
        lp = apply_ymap(mu, a.ymap);
        gk = 2.302585092994046 * lp * gk;
    }
    if (a.has_prior) {
        const double* pmean = a.consts + 3 * ALABI_MAX_DIM;
        const double* pistd = a.consts + 4 * ALABI_MAX_DIM;
        lp += normal_prior_sum(pmean, pistd, lane, d, qc) + a.prior_const;
        if (in) { const double is = pistd[lane]; gk -= (qc - pmean[lane]) * is * is; }
    }
    grad = gk;
}

// Products with a move's lower-triangular scale factor, called by the 64 lanes of one wave together (lanes >= d pass zeros and get
// zero).  Cs: the factor in LDS, row-major with row stride ld (odd, so that the reads down a column spread over the banks).
// (C z)_k = sum_{i <= k} C[k][i] z_i and (C^T g)_k = sum_{i >= k} C[i][k] g_i, i ascending, by fma from 0; a diagonal factor has
// the single term.
__device__ __forceinline__ double scale_times(const double* Cs, int diagonal, int d, int ld, int lane, double z) {
    const bool in = lane < d;
    double s = 0.0;
    if (diagonal) {
        if (in) s = Cs[lane * ld + lane] * z;
    } else {
        for (int m = 0; m < d; ++m) {
            const double zm = lane_bcast(z, m);
            if (in && m <= lane) s = fma(Cs[lane * ld + m], zm, s);
        }
    }
    return s;
}
__device__ __forceinline__ double scale_transposed_times(const double* Cs, int diagonal, int d, int ld, int lane, double g) {
    const bool in = lane < d;
    double s = 0.0;
    if (diagonal) {
        if (in) s = Cs[lane * ld + lane] * g;
    } else {
        for (int m = 0; m < d; ++m) {
            const double gm = lane_bcast(g, m);
            if (in && m >= lane) s = fma(Cs[m * ld + lane], gm, s);
        }
    }
    return s;
}

// sum over the wave's lanes, valid in every lane
__device__ __forceinline__ double wave_total(double v) { return lane_bcast(wave_sum_dpp(v), 63); }

// p1 of an HMC row of the move table: n_leapfrog + q / 512 with q = ln jitter rounded to a multiple of 2^-36 (0: no jitter; q < 512,
// so both parts are exact in the double and come apart exactly).  hmc_leapfrog_of: ens_shared.hpp (the plan reads it too).
__host__ __device__ inline double hmc_ln_jitter_of(double p1) { return (p1 - floor(p1)) * 512.0; }

}  // namespace alabi
