// HMC warm-up for gfx950: ens_hmc_adapt_kernel is ens_hmc_kernel (ens_hmc.hip: launch shape, arithmetic, draws, accept rule -- the
// body is hmc_walker_steps of ens_hmc_device.hpp for both) with a step size per walker that dual averaging adapts (Hoffman & Gelman
// 2014, algorithm 5; tests/hmc_adapt_numpy.py is the CPU statement).  Wave 0 keeps the walker's state (m, H-bar, ln e, ln e-bar, mu)
// beside the walker, every lane the same copy; the state is read when a launch starts and written when it ends, so neither the
// chunk length nor a split of the call changes a bit.  No atomics, no traffic between workgroups.  The mass matrix is adapted on
// the host between calls (alabi_amd/hmc_adapt.py: a pooled covariance per window, alabi_ens_set_move_scale).
// hipcc -Rpass-analysis=kernel-resource-usage for ens_hmc_adapt_kernel, VGPRs / scratch bytes per lane (squared exponential | the
// other families): see the table in ens_hmc.hip's header, row "adapt".
#include <cmath>
#include "ens_hmc_device.hpp"

namespace alabi {

template <int D, bool GENERIC>
__global__ void __launch_bounds__(512)
ens_hmc_adapt_kernel(HmcArgs p, HmcAdaptArgs ad) {
    extern __shared__ __attribute__((aligned(16))) double hmc_lds[];   // [1][d, ld] scale factor | [Npad] weights
    __shared__ double qs_s[ALABI_MAX_DIM], g_s[ALABI_MAX_DIM];
    __shared__ double scratch[16];
    hmc_walker_steps<D, GENERIC, true>(p, ad, hmc_lds, qs_s, g_s, scratch);
}

template <int D, bool GENERIC>
static int launch_hmc_adapt_inst(const HmcArgs& a, const HmcAdaptArgs& ad, int grid, int T, size_t lds, hipStream_t s) {
    if (lds > 32 * 1024) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(ens_hmc_adapt_kernel<D, GENERIC>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, ALABI_HMC_MAX_LDS);
        if (err != hipSuccess) return hip_fail(err, "hipFuncSetAttribute(ens_hmc_adapt_kernel)", __FILE__, __LINE__);
    }
    hipLaunchKernelGGL((ens_hmc_adapt_kernel<D, GENERIC>), dim3(grid), dim3(T), lds, s, a, ad);
    return ALABI_OK;
}

// K steps from global step step0 + done0; par: delta, gamma, t0, kappa (checked by the caller)
int launch_ens_hmc_adapt(alabi_ens* e, double* coords, double* logp, long long step0, long long done0, int K, int thin_by, double* chain,
                         double* chain_logp, long long* n_accept, double* da_state, const double* par, double* accept_stat, hipStream_t s) {
    if (K <= 0) return ALABI_OK;
    const int db = dim_bucket(e->d);
    const size_t lds = hmc_lds_bytes(e);
    if (!e->all_hmc || e->moves.n != 1 || !e->gauss_C || db < 0 || lds > ALABI_HMC_MAX_LDS) return ALABI_BAD_ARGUMENT;
    const HmcArgs a = hmc_args(e, coords, logp, step0, done0, K, thin_by, chain, chain_logp, n_accept);
    if (!a.lg.Xt || !a.lg.alpha) return ALABI_NOT_COMPUTED;
    const HmcAdaptArgs ad{da_state, accept_stat, par[0], par[1], par[2], par[3]};
    const int grid = e->W * e->E, T = hmc_threads(e);
    e->hmc_plan[0] = T; e->hmc_plan[1] = K; e->hmc_plan[2] = (int)lds; e->hmc_plan[3] = e->gp->Npad > T ? 1 : 0;
    int st = ALABI_OK;
    ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, st = (launch_hmc_adapt_inst<D, GENERIC>(a, ad, grid, T, lds, s))));
    if (st != ALABI_OK) return st;
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // namespace alabi
