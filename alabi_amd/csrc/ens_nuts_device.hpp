// What ens_nuts_kernel (ens_nuts.hip) and its launchers share: the arguments, the draws' streams, the LDS layout and the small
// helpers of the tree.  ens_hmc_device.hpp (HmcArgs, the step's move and step size) and ens_grad_device.hpp (lp_grad_eval, the
// products with a scale factor) are included read-only: ens_hmc_kernel and ens_hmc_adapt_kernel keep their code and their bits.
#pragma once
#include "ens_hmc_device.hpp"

namespace alabi {

// ALABI_NUTS_MAX_DEPTH, ens_nuts_lds_bytes: ens_shared.hpp / ens_plan.hpp (the plan reads them too)
#define ALABI_NUTS_STREAM_DIR 13u
#define ALABI_NUTS_STREAM_LEAF 14u
#define ALABI_NUTS_STREAM_TREE 15u

// stop reasons of a transition (the trace of alabi_ens_step_with_randoms_nuts)
#define ALABI_NUTS_STOP_DEPTH 0
#define ALABI_NUTS_STOP_TREE 1
#define ALABI_NUTS_STOP_SUBTREE 2
#define ALABI_NUTS_STOP_DIVERGENT 3

struct NutsArgs {
    HmcArgs h;                   // walkers, evaluation, chain, table, factors; inj_z set: the test entry (z0 [W, d], e = inj_e, move inj_k)
    long long* counts;           // [E*W, 3] in/out: leaves, depths reached, divergent transitions
    double* accept_sum;          // [E*W] in/out: the sum of a over all leaves
    const unsigned* inj_dir;     // [W] direction words                  }
    const double* inj_uleaf;     // [W, 2^Dmax - 1] leaf uniforms        } test entry only
    const double* inj_utree;     // [W, Dmax] tree uniforms              }
    int* trace;                  // [W, 4] or null: depth reached, leaves made, stop reason, 1 if a leaf was taken
};

// ln(exp(a) + exp(b)); a or b may be -inf (then the other comes back unchanged), never both
__device__ __forceinline__ double nuts_logaddexp(double a, double b) {
    const double hi = fmax(a, b), lo = fmin(a, b);
    if (lo == -INFINITY) return hi;
    return hi + log1p(exp(lo - hi));
}

__device__ __forceinline__ double nuts_uniform(uint32_t s_lo, uint32_t s_hi, uint32_t w, uint32_t word, uint32_t k0, uint32_t k1) {
    uint32_t r[4];
    philox4x32_10(s_lo, s_hi, w, word, k0, k1, r);
    return u53(r[0], r[1]);
}

// ---- host side
inline size_t nuts_lds_bytes(const alabi_ens* e) { return ens_nuts_lds_bytes(e->moves.n, e->d, e->gp->Npad); }

}  // namespace alabi
