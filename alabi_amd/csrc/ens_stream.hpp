// What the persistent ensemble kernels (ens_stream_kernel in ensemble.hip, ens_pair_kernel in ens_pair.hip) share: the version
// history's sentinel, the kernel arguments, the write-through hand-off accessors and the ordered sum of the wave partials.
#pragma once
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

StreamArgs ens_stream_args(alabi_ens* e, const DrawBuffers& rec, int K);   // ensemble.hip: the arguments of one chunk of K steps

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

}  // namespace alabi
