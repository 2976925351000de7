// NUTS warm-up for gfx950: the two kernels that leave alabi_amd.moves.NUTSMove without a hand-set knob (tests/nuts_adapt_numpy.py is
// the CPU statement of both).
//
// ens_nuts_adapt_kernel is ens_nuts_kernel (ens_nuts.hip: launch shape, arithmetic, draws, tree, checkpoints, four-barrier leaf and
// stop word -- the body is nuts_walker_transitions of ens_nuts_device.hpp for both) with a step size per walker that dual averaging
// adapts (Hoffman & Gelman 2014, algorithm 5 and section 3.2.1) on NUTS's own statistic: a_t, the mean over ALL leaves a transition
// made of a = min(1, exp(H0 - H_leaf)), 0 outside the open box and 0 for the divergent leaf (which counts as a leaf).  a_t has a sum
// of its own, reset per transition; the kernel's running sum of a keeps its order of additions.  The state (m, H-bar, ln e,
// ln e-bar, mu), the sum of a_t and the transition's sum sit in static LDS, one column per lane of wave 0 and every column the same:
// they are touched once per transition and never live across lp_grad_eval, so the tree's registers are ens_nuts_kernel's.  The
// state is read when a launch starts and written when it ends, so neither the chunk length nor a split of the call changes a bit.
// The update sits in the `if (tid < 64)` block behind the leaf loop, which holds no barrier: no thread reaches a barrier on the
// state.  The per-walker sums of leaves, depths, divergences and a go to buffers of the CALLER: warm-up transitions are no part of
// alabi_ens_nuts_stats.  The mass matrix is adapted on the host between calls (alabi_amd/hmc_adapt.py).
//
// ens_step_search_kernel is Stan's find_reasonable heuristic for the initial step size, for a table that is all kind 6 or all kind
// 7 (the same whitened leapfrog).  One workgroup per walker, which does not move.  From ln e in, with lp = the caller's logp and
// g = grad lnp(x), iteration i = 0, 1, ... < 40:
//     z ~ N(0, I) fresh;  H0 = -lp + |z|^2 / 2;  one leaf: z += (e / 2) C^T g;  q = x + e C z;  (lp_q, g_q) at q;  z += (e / 2) C^T g_q
//     dH = H0 - (-lp_q + |z|^2 / 2), -inf for a NaN or a q outside the open box
//     i = 0: dir = +1 if dH > ln 0.8, else -1
//     stop iff (dir = +1 and not dH > ln 0.8) or (dir = -1 and not dH < ln 0.8); otherwise ln e += dir ln 2
// and iters = i of the iteration that stopped the loop = the number of ln 2 steps taken, 40 when the cap ended it (the walker keeps
// its last ln e, 40 steps from the start).  Draws: Philox counter (step, global
// walker id, 11 + 16 (64 (i + 1) + k)) for coordinate k -- stream 11 beyond the b = k < 64 that the moves read, so no draw of a
// move is read twice; no global step is consumed.  Loop control as ens_nuts_kernel: wave 0 decides, lane 0 writes the stop word,
// ONE barrier, every thread reads the same word; the next write lies behind the next evaluation's three barriers.
// LDS: [d, d | 1] factor of move k_move | [Npad] weights, at most 128 KB; static 1.2 KB.
//
// hipcc -Rpass-analysis=kernel-resource-usage, VGPRs / scratch bytes per lane (squared exponential | the other families), two waves
// per SIMD throughout (__launch_bounds__(512)):
//   ens_nuts_adapt_kernel, static LDS 4752 bytes
//   D = 1: 240 / 36 | 243 / 0   D = 5: 243 / 0 | 253 / 0   D = 10: 244 / 0 | 254 / 36
//   D = 16: 254 / 12 | 255 / 52   D = 20: 256 / 36 | 255 / 84   D = 24: 256 / 44 | 256 / 124
//   D = 32: 256 / 96 | 256 / 176   D = 48: 256 / 232 | 256 / 312   D = 64: 256 / 344 | 256 / 440
// (the state in LDS costs the tree nothing: within 8 VGPRs and 24 scratch bytes of ens_nuts_kernel's row at every bucket)
//   ens_step_search_kernel, static LDS 1168 bytes
//   D = 1: 176 / 0 | 174 / 0   D = 5: 169 / 0 | 183 / 0   D = 10: 175 / 0 | 193 / 0
//   D = 16: 187 / 0 | 205 / 0   D = 20: 195 / 0 | 213 / 0   D = 24: 203 / 0 | 221 / 0
//   D = 32: 219 / 0 | 237 / 0   D = 48: 255 / 0 | 256 / 32   D = 64: 256 / 60 | 256 / 156
#include <cmath>
#include "ens_nuts_device.hpp"

namespace alabi {

template <int D, bool GENERIC>
__global__ void __launch_bounds__(512)
ens_nuts_adapt_kernel(NutsArgs a, HmcAdaptArgs ad) {
    extern __shared__ __attribute__((aligned(16))) double nuts_lds[];   // [1][d, ld] scale factor | [Npad] weights | checkpoints
    __shared__ double qs_s[ALABI_MAX_DIM], g_s[ALABI_MAX_DIM];
    __shared__ double scratch[16];
    __shared__ double da_s[ALABI_NUTS_DA_ROWS * 64];
    __shared__ int stop_s;
    nuts_walker_transitions<D, GENERIC, true>(a, ad, nuts_lds, qs_s, g_s, scratch, &stop_s, da_s);
}

#define ALABI_STEP_SEARCH_CAP 40
#define ALABI_STEP_SEARCH_LN_TARGET (-0.22314355131420976)   // ln 0.8

struct StepSearchArgs {
    const double* coords;        // [E*W, d], not written
    const double* logp;          // [E*W], not written
    LpGradArgs lg;
    const double* scale_C;       // [d, d] factor of move k_move
    double* ln_e;                // [E*W] in/out
    int* iters;                  // [E*W] or null
    long long step;
    unsigned long long seed;
    int diagonal;
};

template <int D, bool GENERIC>
__global__ void __launch_bounds__(512)
ens_step_search_kernel(StepSearchArgs p) {
    extern __shared__ __attribute__((aligned(16))) double srch_lds[];   // [d, ld] scale factor | [Npad] weights
    __shared__ double qs_s[ALABI_MAX_DIM], g_s[ALABI_MAX_DIM];
    __shared__ double scratch[16];
    __shared__ int stop_s;
    const int tid = threadIdx.x, T = blockDim.x, d = p.lg.d, ld = d | 1;
    const int w = blockIdx.x;                                       // global walker id
    double* w_s = srch_lds + (size_t)d * ld;
    for (int idx = tid; idx < d * d; idx += T) srch_lds[(idx / d) * ld + (idx % d)] = p.scale_C[idx];
    const bool in = tid < d;
    double xv = 0.0, inv_len = 0.0, lo = 0.0, hi = 0.0;
    if (in) {
        xv = p.coords[(size_t)w * d + tid];
        inv_len = p.lg.consts[tid];
        lo = p.lg.consts[ALABI_MAX_DIM + tid];
        hi = p.lg.consts[2 * ALABI_MAX_DIM + tid];
    }
    const double lp0 = p.logp[w];
    const uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32);
    const uint32_t s_lo = (uint32_t)p.step, s_hi = (uint32_t)((unsigned long long)p.step >> 32);
    double ln_e = tid < 64 ? p.ln_e[w] : 0.0;
    double gx, lp_unused;
    lp_grad_eval<D, GENERIC>(p.lg, w_s, qs_s, g_s, scratch, xv, inv_len, lp_unused, gx);   // its first barrier covers the factor
    int i = 0, dir = 0;
    bool go;
    do {   // one leapfrog step per trip; the trip count is the stop word's, the same for every thread
        double e = 0.0, z = 0.0, q = xv, H0 = 0.0, lpq = 0.0, gq = 0.0;
        if (tid < 64) {
            e = exp(ln_e);
            z = in ? philox_normal(s_lo, s_hi, (uint32_t)w, ALABI_HMC_STREAM_Z + 16u * (uint32_t)(64 * (i + 1) + tid), k0, k1) : 0.0;
            H0 = -lp0 + 0.5 * wave_total(z * z);
            z = fma(0.5 * e, scale_transposed_times(srch_lds, p.diagonal, d, ld, tid, gx), z);
            q = fma(e, scale_times(srch_lds, p.diagonal, d, ld, tid, z), xv);
        }
        lp_grad_eval<D, GENERIC>(p.lg, w_s, qs_s, g_s, scratch, q, inv_len, lpq, gq);
        if (tid < 64) {
            z = fma(0.5 * e, scale_transposed_times(srch_lds, p.diagonal, d, ld, tid, gq), z);
            double dH = H0 - (0.5 * wave_total(z * z) - lpq);
            const bool out = in && !((q > lo) && (q < hi));         // NaN is outside
            if (__ballot(out) != 0ull || dH != dH) dH = -INFINITY;
            if (i == 0) dir = dH > ALABI_STEP_SEARCH_LN_TARGET ? 1 : -1;
            int stop = dir > 0 ? !(dH > ALABI_STEP_SEARCH_LN_TARGET) : !(dH < ALABI_STEP_SEARCH_LN_TARGET);
            if (!stop) {
                ln_e += dir > 0 ? 0.6931471805599453 : -0.6931471805599453;
                if (++i == ALABI_STEP_SEARCH_CAP) stop = 1;
            }
            if (tid == 0) stop_s = stop;
        }
        __syncthreads();
        go = stop_s == 0;
    } while (go);
    if (tid == 0) {
        p.ln_e[w] = ln_e;
        if (p.iters) p.iters[w] = i;
    }
}

template <int D, bool GENERIC>
static int launch_nuts_adapt_inst(const NutsArgs& a, const HmcAdaptArgs& ad, int grid, int T, size_t lds, hipStream_t s) {
    if (lds > 32 * 1024) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(ens_nuts_adapt_kernel<D, GENERIC>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, ALABI_HMC_MAX_LDS);
        if (err != hipSuccess) return hip_fail(err, "hipFuncSetAttribute(ens_nuts_adapt_kernel)", __FILE__, __LINE__);
    }
    hipLaunchKernelGGL((ens_nuts_adapt_kernel<D, GENERIC>), dim3(grid), dim3(T), lds, s, a, ad);
    return ALABI_OK;
}

// K transitions from global step step0 + done0; par: delta, gamma, t0, kappa (checked by the caller); counts, accept_sum: the caller's
int launch_ens_nuts_adapt(alabi_ens* e, double* coords, double* logp, long long step0, long long done0, int K, int thin_by, double* chain,
                          double* chain_logp, long long* n_accept, double* da_state, const double* par, long long* counts,
                          double* accept_sum, double* accept_stat, hipStream_t s) {
    if (K <= 0) return ALABI_OK;
    const int db = dim_bucket(e->d);
    const size_t lds = nuts_lds_bytes(e);
    if (!e->all_nuts || e->moves.n != 1 || !e->gauss_C || db < 0 || lds > ALABI_HMC_MAX_LDS) return ALABI_BAD_ARGUMENT;
    NutsArgs a{};
    a.h = hmc_args(e, coords, logp, step0, done0, K, thin_by, chain, chain_logp, n_accept);
    a.counts = counts; a.accept_sum = accept_sum;
    if (!a.h.lg.Xt || !a.h.lg.alpha) return ALABI_NOT_COMPUTED;
    const HmcAdaptArgs ad{da_state, accept_stat, par[0], par[1], par[2], par[3]};
    const int grid = e->W * e->E, T = hmc_threads(e);
    e->nuts_plan[0] = T; e->nuts_plan[1] = K; e->nuts_plan[2] = (int)lds; e->nuts_plan[3] = e->gp->Npad > T ? 1 : 0;
    int st = ALABI_OK;
    ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, st = (launch_nuts_adapt_inst<D, GENERIC>(a, ad, grid, T, lds, s))));
    if (st != ALABI_OK) return st;
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

template <int D, bool GENERIC>
static int launch_step_search_inst(const StepSearchArgs& a, int grid, int T, size_t lds, hipStream_t s) {
    if (lds > 32 * 1024) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(ens_step_search_kernel<D, GENERIC>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, ALABI_HMC_MAX_LDS);
        if (err != hipSuccess) return hip_fail(err, "hipFuncSetAttribute(ens_step_search_kernel)", __FILE__, __LINE__);
    }
    hipLaunchKernelGGL((ens_step_search_kernel<D, GENERIC>), dim3(grid), dim3(T), lds, s, a);
    return ALABI_OK;
}

int launch_ens_step_search(alabi_ens* e, const double* coords, const double* logp, long long step, int k_move, double* ln_e, int* iters,
                           hipStream_t s) {
    const int db = dim_bucket(e->d);
    if (!(e->all_hmc || e->all_nuts) || !e->gauss_C || db < 0 || k_move < 0 || k_move >= e->moves.n) return ALABI_BAD_ARGUMENT;
    const size_t lds = ens_hmc_lds_bytes(1, e->d, e->gp->Npad);
    if (lds > ALABI_HMC_MAX_LDS) return ALABI_BAD_ARGUMENT;
    StepSearchArgs a{};
    a.coords = coords; a.logp = logp; a.lg = lp_grad_args(e);
    a.scale_C = e->gauss_C + (size_t)k_move * e->d * e->d;
    a.ln_e = ln_e; a.iters = iters; a.step = step; a.seed = e->seed;
    a.diagonal = (e->gauss_diag >> k_move) & 1;
    if (!a.lg.Xt || !a.lg.alpha) return ALABI_NOT_COMPUTED;
    const int grid = e->W * e->E, T = hmc_threads(e);
    int st = ALABI_OK;
    ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, st = (launch_step_search_inst<D, GENERIC>(a, grid, T, lds, s))));
    if (st != ALABI_OK) return st;
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // namespace alabi
