// Device helpers shared by the ensemble kernels (ensemble.hip, ens_stream.hpp) and the nested-sampling walk kernel (nested.hip):
// the counter-based Philox4x32-10 generator, the inverse y-scaler map and the squared-exponential pair terms.
#pragma once
#include "gp_device.hpp"

namespace alabi {

__device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                     uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ inline double u53(uint32_t a, uint32_t b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}

typedef double f64x2 __attribute__((ext_vector_type(2)));

// Inverse of the y scaler applied to the GP mean (alabi/core.py:1483-1502 un-scales every prediction; the two non-affine
// scalers the reference ships are alabi/utility.py:62-71): 0 identity (affine scalers are folded into amp / mean),
// 1 nlog_scaler (y = -10^x), 2 log_scaler (y = 10^x).  Evaluated once per proposal by the deciding wave.
__device__ inline double apply_ymap(double x, int kind) {
    if (kind == 0) return x;
    const double v = pow(10.0, x);
    return kind == 1 ? -v : v;
}

// ---- squared exponential in the half-step kernels (round 3) -------------------------------------------------------------
// alpha_n exp(-|x_n - q|^2 / 2) = sgn(alpha_n) exp(q.x_n - h_n - |q|^2 / 2) with h_n = |x_n|^2 / 2 - ln|alpha_n| resident instead of
// alpha_n (sign in its lowest mantissa bit) and all coordinates relative to the mean of the training inputs (the products lose
// eps (|x|^2 + |q|^2) / 2 absolutely -- negligible near the centre): ONE fma per point and coordinate instead of a subtraction and
// an fma, no multiply by alpha -- 33 instead of 41 fp64 instructions per kernel evaluation in kernels whose time is their
// instruction count (ens_stream_kernel: 1.96 -> 1.89 us per half step at N = 2000, d = 10, without a register more: h takes
// alpha's place).  ens_stream_kernel, ens_half_kernel and ens_half_multi_kernel share these functions and the accumulation order
// (acc = 0; acc += term_a; acc += term_b per pair), so their chains stay bit-identical.  The other kernel families keep the
// difference form.
template <int D>
__device__ inline double se_neg_half_norm(const double (&q)[D]) {
    double n = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) n = fma(q[k], q[k], n);
    return -0.5 * n;
}
template <int D>
__device__ inline void se_pair_terms(const f64x2 (&x)[D], f64x2 h, const double (&q)[D], double nhq, double& fa, double& fb) {
    double da = nhq - h.x, db = nhq - h.y;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        da = fma(x[k].x, q[k], da);
        db = fma(x[k].y, q[k], db);
    }
    fa = exp_direct(da);
    fb = exp_direct(db);
    fa = __hiloint2double(__double2hiint(fa) ^ (__double2loint(h.x) << 31), __double2loint(fa));
    fb = __hiloint2double(__double2hiint(fb) ^ (__double2loint(h.y) << 31), __double2loint(fb));
}
#define ALABI_SE_PAD 1000.0   // h of a point that contributes nothing: exp(-1000 + ...) underflows to exactly 0

// A standard normal by Box-Muller from one Philox block: sqrt(-2 ln(1 - u53(r0, r1))) cos(2 pi u53(r2, r3)).
__device__ inline double philox_normal(uint32_t s_lo, uint32_t s_hi, uint32_t gid, uint32_t word, uint32_t k0, uint32_t k1) {
    uint32_t r[4];
    philox4x32_10(s_lo, s_hi, gid, word, k0, k1, r);
    const double u1 = u53(r[0], r[1]), u2 = u53(r[2], r[3]);
    return sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2);
}

// Normal-prior term of coordinate `lane` (< d) of a proposal, summed over the wave: lanes >= d contribute 0.
// consts rows 3 / 4: prior mean, 1 / std (0 where there is no normal prior).  Result valid in every lane.
__device__ inline double normal_prior_sum(const double* pmean, const double* pistd, int lane, int d, double x) {
    double t = 0.0;
    if (lane < d) { t = (x - pmean[lane]) * pistd[lane]; t = -0.5 * t * t; }
    return lane_bcast(wave_sum_dpp(t), 63);
}

// A lane's share of the kernel sum of the half-step kernels (ens_half_kernel, ens_mh_kernel): the resident pairs xa / aa (points
// 2 tid, 2 tid + 1; h instead of alpha for the squared exponential) and, where Npad / 2 exceeds the block, the pairs tid + T,
// tid + 2 T, ... streamed from Xsrc / Asrc.  One accumulation order for every caller, so their log-probabilities agree bit for bit.
template <int D, bool GENERIC>
__device__ __forceinline__ double half_lane_sum(const f64x2 (&xa)[D], f64x2 aa, const double (&q)[D], const double* __restrict__ Xsrc,
                                                const double* __restrict__ Asrc, int Npad, int tid, int T, const KernelFn& kf) {
    const int half = Npad >> 1;
    double acc;
    if (!GENERIC) {
        const double nhq = se_neg_half_norm<D>(q);
        double fa, fb;
        se_pair_terms<D>(xa, aa, q, nhq, fa, fb);
        acc = 0.0; acc += fa; acc += fb;
        for (int j = tid + T; j < half; j += T) {
            f64x2 x[D];
#pragma unroll
            for (int k = 0; k < D; ++k) x[k] = reinterpret_cast<const f64x2*>(Xsrc + (size_t)k * Npad)[j];
            se_pair_terms<D>(x, reinterpret_cast<const f64x2*>(Asrc)[j], q, nhq, fa, fb);
            acc += fa; acc += fb;
        }
    } else {
        double r2a = 0.0, r2b = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double da = xa[k].x - q[k], db = xa[k].y - q[k];
            r2a = fma(da, da, r2a);
            r2b = fma(db, db, r2b);
        }
        acc = aa.x * radial<GENERIC>(r2a, kf);
        acc = fma(aa.y, radial<GENERIC>(r2b, kf), acc);
        for (int j = tid + T; j < half; j += T) {
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const f64x2 x = reinterpret_cast<const f64x2*>(Xsrc + (size_t)k * Npad)[j];
                const double d0 = x.x - q[k], d1 = x.y - q[k];
                s0 = fma(d0, d0, s0);
                s1 = fma(d1, d1, s1);
            }
            const f64x2 al = reinterpret_cast<const f64x2*>(Asrc)[j];
            acc = fma(al.x, radial<GENERIC>(s0, kf), acc);
            acc = fma(al.y, radial<GENERIC>(s1, kf), acc);
        }
    }
    return acc;
}

// ---- Gaussian Metropolis move (kind 5; tests/gaussian_move_numpy.py is the CPU statement) -------------------------------------
// q = x + f C z: C the move's lower-triangular scale factor (a scalar or diagonal covariance has the diagonal alone), z standard
// normals, f = exp(v) the scale factor of the step, v ~ U(-ln factor, ln factor) -- ONE draw per step and ensemble -- or 1.
// Mode 0 moves every coordinate, mode 1 one coordinate drawn per walker and step, mode 2 coordinate (step mod d).
// Draws: Philox counter (step, global walker id, stream word S + 16 b), beside streams 0-8 of ensemble.hip:
//   S = 9, b = 0:   v = (2 u53(r0, r1) - 1) ln factor, at the ensemble's walker 0; not drawn without a factor;
//   S = 9, b = 1:   the coordinate of mode 1, (r0 d) >> 32, at the walker;
//   S = 10, b = k:  the normal z_k of coordinate k (philox_normal), at the walker.
// The accept uniform is stream 2 at the walker and the step's move stream 3 at the ensemble's walker 0, as for every move.
__device__ inline void gauss_step_draws(uint32_t s_lo, uint32_t s_hi, uint32_t g0, uint32_t w, uint32_t k0, uint32_t k1, long long step,
                                        double ln_factor, int mode, int d, double& f, int& c) {
    uint32_t r[4];
    f = 1.0;
    if (ln_factor != 0.0) {
        philox4x32_10(s_lo, s_hi, g0, 9u, k0, k1, r);
        f = exp((2.0 * u53(r[0], r[1]) - 1.0) * ln_factor);
    }
    c = -1;
    if (mode == 1) {
        philox4x32_10(s_lo, s_hi, w, 9u + 16u, k0, k1, r);
        c = (int)(((uint64_t)r[0] * (uint64_t)d) >> 32);
    } else if (mode == 2) {
        c = (int)(step % (long long)d);
    }
}

// Coordinate `lane` of the proposal, called by the 64 lanes of one wave together (lanes >= d pass zeros, their result means
// nothing).  Cs: the factor, row-major [d, d], in LDS.  s_k = sum_{i <= k} C[k][i] z_i, i ascending, by fma from 0 (a diagonal
// factor has the single term), q_k = fma(f, s_k, x_k); with a coordinate c >= 0 every other coordinate is the walker's, bit for bit.
__device__ __forceinline__ double gauss_coord(const double* Cs, int diagonal, int d, int lane, double xv, double z, double f, int c) {
    const bool in = lane < d;
    double s = 0.0;
    if (diagonal) {
        if (in) s = fma(Cs[lane * d + lane], z, 0.0);
    } else {
        for (int m = 0; m < d; ++m) {
            const double zm = lane_bcast(z, m);
            if (in && m <= lane) s = fma(Cs[lane * d + m], zm, s);
        }
    }
    const double q = fma(f, s, xv);
    return (c >= 0 && lane != c) ? xv : q;
}

}  // namespace alabi
