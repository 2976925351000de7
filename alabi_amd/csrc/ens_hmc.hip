// Hamiltonian Monte Carlo ensemble for gfx950: W independent chains that use the surrogate's closed-form gradient (kind 6 of the
// move table, alabi_amd.moves.HMCMove; tests/hmc_numpy.py is the CPU statement).
//
// An HMC proposal reads nothing but the walker itself, like a Metropolis proposal, so ens_hmc_kernel has ens_mh_kernel's shape: ONE
// workgroup per walker (E W of them, any count; no spin loops, no atomics, no traffic between workgroups) and every step of a chunk
// in one launch.  Wave 0 keeps the walker, its log-probability, its gradient and the momentum, lane k coordinate k.  Per step, in
// whitened momentum z (mass matrix cov^-1, C C^T = cov, C the move's lower-triangular scale factor in LDS):
//     z0 ~ N(0, I)            e = step_size f,  f = 1 or exp(v), v ~ U(-ln jitter, ln jitter), one draw per step and ensemble
//     z = z0 + (e / 2) C^T g
//     n_leapfrog times:   q = q + e C z;   (lp_q, g_q) = lnp and its gradient at q;   z = z + e C^T g_q   (e / 2 the last time)
//     accept iff lp_q - |z|^2 / 2 - lp + |z0|^2 / 2 > ln u' and q lies in the open box (NaN anywhere rejects)
// Only the end point is tested against the box: in between, the trajectory follows the GP mean's smooth extension (DESIGN.md
// section 6 has the argument that this leaves exp(lnp) 1[box] invariant).
// Draws: Philox counter (step, global walker id, stream word S + 16 b) -- S = 11, b = k: the momentum normal z0_k at the walker
// (Box-Muller, philox_normal); S = 12, b = 0: v = (2 u53(r0, r1) - 1) ln jitter at the ensemble's walker 0, not drawn without
// jitter; the accept uniform is stream 2 at the walker and the step's move stream 3 at the ensemble's walker 0, as for every move.
//
// The hot loop is lp_grad_eval (ens_grad_device.hpp): two passes over the training set per evaluation, the weights of the gradient
// sum handed from the first to the second through LDS, every sum in a fixed order.  The gradient at the walker is evaluated at the
// start of every launch and after an accept it is the trajectory's last evaluation, carried in registers; both are the same code
// at the same point, so the chunk length changes no bit.  lp comes from the caller's logp and is never recomputed.
//
// LDS: the scale factors [n][d, d | 1] doubles and the weights [Npad] doubles, together at most 128 KB (alabi_ens_run refuses a
// table that needs more: there is no other kernel for it), plus 1.2 KB.  The training set is read from L2 in both passes: the
// second pass reads it by coordinate, which a lane-resident share (ens_mh_kernel) cannot serve.
// hipcc -Rpass-analysis=kernel-resource-usage for ens_hmc_kernel, VGPRs / scratch bytes per lane (squared exponential | the other
// families), two waves per SIMD throughout (__launch_bounds__(512) leaves 256 VGPRs per lane):
//   D = 1: 180 / 0 | 187 / 0     D = 5: 182 / 0 | 196 / 0     D = 10: 187 / 0 | 206 / 0     D = 16: 199 / 0 | 218 / 0
//   D = 20: 207 / 0 | 226 / 0    D = 24: 215 / 0 | 234 / 0    D = 32: 231 / 0 | 250 / 0
//   D = 48: 256 / 28 | 256 / 84  D = 64: 256 / 112 | 256 / 208
// The floor of about 180 is the move table (8 rows by value) and the unrolled point loop, not the dimension; the query point costs
// 2 D of them, and from the D = 48 bucket on a part of it lives in scratch.
// (With the body in ens_hmc_device.hpp every figure is what it was before, but D = 48 of the other families: 255 -> 256 VGPRs.)
// adapt: ens_hmc_adapt_kernel (ens_hmc_adapt.hip), the same body with the dual-averaging state in wave 0: 12 to 14 VGPRs more,
//   D = 1: 194 / 0 | 200 / 0     D = 5: 194 / 0 | 209 / 0     D = 10: 200 / 0 | 219 / 0     D = 16: 212 / 0 | 231 / 0
//   D = 20: 220 / 0 | 239 / 0    D = 24: 228 / 0 | 247 / 0    D = 32: 244 / 0 | 255 / 36
//   D = 48: 256 / 52 | 256 / 136 D = 64: 256 / 168 | 256 / 280
#include <cstdlib>
#include "ens_hmc_device.hpp"

namespace alabi {

// (HmcArgs, the draws' helpers and the steps of a walker: ens_hmc_device.hpp, shared with ens_hmc_adapt_kernel)
template <int D, bool GENERIC>
__global__ void __launch_bounds__(512)
ens_hmc_kernel(HmcArgs p) {
    extern __shared__ __attribute__((aligned(16))) double hmc_lds[];   // [n][d, ld] scale factors | [Npad] weights
    __shared__ double qs_s[ALABI_MAX_DIM], g_s[ALABI_MAX_DIM];
    __shared__ double scratch[16];
    hmc_walker_steps<D, GENERIC, false>(p, HmcAdaptArgs{}, hmc_lds, qs_s, g_s, scratch);
}

// lnp and its gradient at M arbitrary points, one workgroup per point: the kernel's evaluation behind the box gate
// (alabi_ens_log_prob_grad: -inf and a zero gradient outside the open box).
template <int D, bool GENERIC>
__global__ void __launch_bounds__(512)
ens_lp_grad_kernel(LpGradArgs lg, const double* __restrict__ pts, double* __restrict__ logp, double* __restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) double hmc_lds[];   // [Npad] weights
    __shared__ double qs_s[ALABI_MAX_DIM], g_s[ALABI_MAX_DIM];
    __shared__ double scratch[16];
    const int tid = threadIdx.x, d = lg.d, m = blockIdx.x;
    const bool in = tid < d;
    double xv = 0.0, inv_len = 0.0, lo = 0.0, hi = 0.0;
    if (in) {
        xv = pts[(size_t)m * d + tid];
        inv_len = lg.consts[tid];
        lo = lg.consts[ALABI_MAX_DIM + tid];
        hi = lg.consts[2 * ALABI_MAX_DIM + tid];
    }
    double lp, g;
    lp_grad_eval<D, GENERIC>(lg, hmc_lds, qs_s, g_s, scratch, xv, inv_len, lp, g);
    if (tid >= 64) return;
    const bool out = in && !((xv > lo) && (xv < hi));
    if (__ballot(out) != 0ull) { lp = -INFINITY; g = 0.0; }
    if (in) grad[(size_t)m * d + tid] = g;
    if (tid == 0) logp[m] = lp;
}

// The production draws of one step (alabi_ens_export_hmc_draws): per ensemble the move and e, per walker the momentum normals and
// the accept uniform.  One thread per walker.
__global__ void ens_hmc_export_kernel(unsigned long long seed, long long step, int W, int E, int d, MoveTable mt, int* __restrict__ move,
                                      double* __restrict__ e_out, double* __restrict__ z, double* __restrict__ u_acc) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= W * E) return;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const uint32_t s_lo = (uint32_t)step, s_hi = (uint32_t)((unsigned long long)step >> 32);
    const uint32_t g0 = (uint32_t)((gid / W) * W);
    if ((uint32_t)gid == g0) {
        const int mi = hmc_step_move(mt, s_lo, s_hi, g0, k0, k1);
        double mp0, mp1;
        hmc_move_params(mt, mi, mp0, mp1);
        move[gid / W] = mi;
        e_out[gid / W] = hmc_step_size(mp0, hmc_ln_jitter_of(mp1), s_lo, s_hi, g0, k0, k1);
    }
    for (int k = 0; k < d; ++k) z[(size_t)gid * d + k] = philox_normal(s_lo, s_hi, (uint32_t)gid, ALABI_HMC_STREAM_Z + 16u * (uint32_t)k, k0, k1);
    if (u_acc) {
        uint32_t r[4];
        philox4x32_10(s_lo, s_hi, (uint32_t)gid, 2u, k0, k1, r);
        u_acc[gid] = u53(r[0], r[1]);
    }
}

template <int D, bool GENERIC>
static int launch_hmc_inst(const HmcArgs& a, int grid, int T, size_t lds, hipStream_t s) {
    if (lds > 32 * 1024) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(ens_hmc_kernel<D, GENERIC>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, ALABI_HMC_MAX_LDS);
        if (err != hipSuccess) return hip_fail(err, "hipFuncSetAttribute(ens_hmc_kernel)", __FILE__, __LINE__);
    }
    hipLaunchKernelGGL((ens_hmc_kernel<D, GENERIC>), dim3(grid), dim3(T), lds, s, a);
    return ALABI_OK;
}

// inj_z set: the test entry's single step (K = 1) of move inj_k from injected draws
int launch_ens_hmc(alabi_ens* e, double* coords, double* logp, long long step0, long long done0, int K, int thin_by, double* chain,
                   double* chain_logp, long long* n_accept, int inj_k, double inj_e, const double* inj_z, const double* inj_u, hipStream_t s) {
    if (K <= 0) return ALABI_OK;
    const int db = dim_bucket(e->d);
    const size_t lds = hmc_lds_bytes(e);
    if (!e->all_hmc || !e->gauss_C || db < 0 || lds > ALABI_HMC_MAX_LDS) return ALABI_BAD_ARGUMENT;
    HmcArgs a = hmc_args(e, coords, logp, step0, done0, K, thin_by, chain, chain_logp, n_accept);
    a.inj_z = inj_z; a.inj_u = inj_u; a.inj_e = inj_e; a.inj_k = inj_k;
    if (!a.lg.Xt || !a.lg.alpha) return ALABI_NOT_COMPUTED;
    const int grid = e->W * e->E, T = hmc_threads(e);
    e->hmc_plan[0] = T; e->hmc_plan[1] = K; e->hmc_plan[2] = (int)lds; e->hmc_plan[3] = e->gp->Npad > T ? 1 : 0;
    int st = ALABI_OK;
    ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, st = (launch_hmc_inst<D, GENERIC>(a, grid, T, lds, s))));
    if (st != ALABI_OK) return st;
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

template <int D, bool GENERIC>
static int launch_lp_grad_inst(const LpGradArgs& a, const double* pts, int M, double* logp, double* grad, int T, size_t lds, hipStream_t s) {
    if (lds > 32 * 1024) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(ens_lp_grad_kernel<D, GENERIC>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, ALABI_HMC_MAX_LDS);
        if (err != hipSuccess) return hip_fail(err, "hipFuncSetAttribute(ens_lp_grad_kernel)", __FILE__, __LINE__);
    }
    hipLaunchKernelGGL((ens_lp_grad_kernel<D, GENERIC>), dim3(M), dim3(T), lds, s, a, pts, logp, grad);
    return ALABI_OK;
}

int launch_ens_lp_grad(alabi_ens* e, const double* pts, int M, double* logp, double* grad, hipStream_t s) {
    if (M <= 0) return ALABI_OK;
    const int db = dim_bucket(e->d);
    const size_t lds = (size_t)e->gp->Npad * sizeof(double);
    if (db < 0 || lds > ALABI_HMC_MAX_LDS) return ALABI_BAD_ARGUMENT;
    const LpGradArgs a = lp_grad_args(e);
    if (!a.Xt || !a.alpha) return ALABI_NOT_COMPUTED;
    int st = ALABI_OK;
    ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, st = (launch_lp_grad_inst<D, GENERIC>(a, pts, M, logp, grad, hmc_threads(e), lds, s))));
    if (st != ALABI_OK) return st;
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_hmc_export(alabi_ens* e, long long step, int* move, double* e_out, double* z, double* u_acc, hipStream_t s) {
    hipLaunchKernelGGL(ens_hmc_export_kernel, dim3((e->W * e->E + 255) / 256), dim3(256), 0, s, e->seed, step, e->W, e->E, e->d, e->moves,
                       move, e_out, z, u_acc);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // namespace alabi
