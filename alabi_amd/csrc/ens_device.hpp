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

}  // namespace alabi
