// No-U-Turn sampler ensemble for gfx950: W independent chains of multinomial NUTS (Betancourt 2017, as in Stan) on the surrogate's
// closed-form gradient (kind 7 of the move table, alabi_amd.moves.NUTSMove; tests/nuts_numpy.py is the CPU statement).
//
// The kernel's body is nuts_walker_transitions<D, GENERIC, false> of ens_nuts_device.hpp, which ens_nuts_adapt_kernel
// (ens_nuts_adapt.hip, the warm-up) instantiates with ADAPT = true; what follows describes both.
// ens_nuts_kernel has ens_hmc_kernel's launch shape: ONE workgroup per walker (E W of them, any count; no spin loops, no atomics,
// no traffic between workgroups, so trees of different sizes cost load imbalance and nothing else) and every transition of a chunk
// in one launch.  Wave 0 keeps the tree, lane k coordinate k, one double per lane each: the two ends (q, z, g), the point being
// integrated, the proposal and the subtree's candidate (q, g; their lp in every lane), rho and the subtree's rho'.  One transition
// of walker x with lp = the caller's logp, g = grad lnp(x), in whitened momentum z (C C^T = cov, C in LDS), e = p0 f as kind 6:
//     z0 ~ N(0, I);  H0 = -lp + |z0|^2 / 2;  both ends = (x, z0, g);  rho = z0;  proposal = x;  ln W = 0
//     doubling j = 0 ... Dmax - 1: bit j of the direction word set -> forward from the right end (s = e), else backward from the
//     left end (s = -e); 2^j leaves, each
//         z += (s / 2) C^T g;  q += s C z;  (lp_q, g) = lnp and its gradient at q;  z += (s / 2) C^T g      (two half kicks: every
//         leaf is a phase point, unlike the fused kick of ens_hmc_kernel)
//         delta = H0 - (-lp_q + |z|^2 / 2);  divergent iff not (delta > -1000) (NaN included): the subtree is dropped, the
//         transition ends;  ln w = delta inside the open box, -inf outside;  a = min(1, exp(delta)) inside, 0 outside or divergent
//         ln w > -inf:  ln W' = logaddexp(ln W', ln w);  the leaf is the subtree's candidate iff ln u_leaf < ln w - ln W'
//         rho' += z;  U-turn inside the subtree (below): turns -> the subtree is dropped, the transition ends
//     a complete subtree: the proposal becomes its candidate iff ln W' > -inf and ln u_tree,j < ln W' - ln W;
//         ln W = logaddexp(ln W, ln W');  rho += rho';  the extended end moves;  stop iff rho . z_left <= 0 or rho . z_right <= 0
//     the walker becomes the proposal with the lp and g of its leaf; n_accept grows by 1 when a leaf was taken.
// The orbit follows lnp WITHOUT its box gate; the box enters through the weights alone.
// U-turn inside the subtree: when the last leaf of an aligned block of 2^k leaves (k >= 1, leaves numbered n = 0, 1, ... as they
// are made) exists, the block turns iff rho_block . z_first <= 0 or rho_block . z_last <= 0.  At most Dmax checkpoints in LDS do
// it: an even n stores (z, running rho' including this leaf) in slot popcount(n); an odd n with t trailing one bits checks the
// slots popcount(n >> 1) down to popcount(n >> 1) - t + 1, slot i with rho = running - ckpt_sum[i] + ckpt_z[i].  Stan's further
// checks across subtree joints are not built.
// Draws: Philox counter (step, global walker id, stream word S + 16 b) -- S = 11 and 12 as kind 6 (momentum normals, jitter), the
// step's move stream 3; S = 13, b = 0: bit j of r0 is the direction of doubling j; S = 14, b = the leaf's ordinal within the
// transition (0 ... 2^Dmax - 2): u_leaf = u53(r0, r1); S = 15, b = j: u_tree,j.  Stream 2 is not read.
//
// BARRIERS.  lp_grad_eval has three and every thread of the workgroup must call it equally often, but only wave 0 knows whether the
// tree goes on.  So a leaf is FOUR barriers: the evaluation's three, then lane 0 writes the stop word to LDS, ONE barrier, and every
// thread reads the same word and leaves or repeats the leaf loop on it.  The next write of the word lies behind the next
// evaluation's barriers (every transition makes at least one leaf), so it cannot overtake these reads.  No thread leaves the leaf
// loop or the transition loop, and none skips a barrier, on anything but that word and the kernel's arguments; what wave 0 alone
// does sits inside `if (tid < 64)` blocks that hold no barrier.  The checkpoints are written and read by the same lane of wave 0.
//
// The gradient at the walker is evaluated at the start of every launch and afterwards it is the proposal's leaf's, carried in
// registers: the same code at the same point, so the chunk length changes no bit.  The per-walker sums (leaves, depths, divergent
// transitions, sum of a) are read at the start of a launch, grow transition by transition and are written at its end.
//
// LDS: the scale factors [n][d, d | 1], the weights [Npad] and the checkpoints [2][10][64] doubles (10 KB), together at most
// 128 KB (ens_nuts_lds_bytes; alabi_ens_run refuses a table that needs more), plus 1.2 KB static.
// hipcc -Rpass-analysis=kernel-resource-usage for ens_nuts_kernel, VGPRs / scratch bytes per lane (squared exponential | the other
// families), two waves per SIMD throughout (__launch_bounds__(512) leaves 256 VGPRs per lane):
//   D = 1: 234 / 36 | 239 / 0   D = 5: 236 / 36 | 249 / 0   D = 10: 240 / 36 | 255 / 20
//   D = 16: 252 / 36 | 254 / 44   D = 20: 256 / 52 | 254 / 76   D = 24: 256 / 52 | 256 / 100
//   D = 32: 256 / 108 | 256 / 168   D = 48: 256 / 236 | 256 / 304   D = 64: 256 / 360 | 256 / 428
// The tree is 16 doubles per lane on top of ens_hmc_kernel's 180 to 230 VGPRs, live across the evaluation: from D = 20 on (from
// D = 10 for the other families) a part of it waits in scratch while the training set is read, stored once before and loaded once
// after an evaluation.  Static LDS 1168 bytes at every bucket.
#include <cstdlib>
#include "ens_nuts_device.hpp"

namespace alabi {

template <int D, bool GENERIC>
__global__ void __launch_bounds__(512)
ens_nuts_kernel(NutsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double nuts_lds[];   // [n][d, ld] scale factors | [Npad] weights | checkpoints
    __shared__ double qs_s[ALABI_MAX_DIM], g_s[ALABI_MAX_DIM];
    __shared__ double scratch[16];
    __shared__ int stop_s;
    nuts_walker_transitions<D, GENERIC, false>(a, HmcAdaptArgs{}, nuts_lds, qs_s, g_s, scratch, &stop_s, nullptr);
}

// The production draws of one step (alabi_ens_export_nuts_draws): per ensemble the move and e, per walker the momentum normals, the
// direction word, the first `depth` tree uniforms and the first 2^depth - 1 leaf uniforms.  One thread per walker.
__global__ void ens_nuts_export_kernel(unsigned long long seed, long long step, int W, int E, int d, int depth, MoveTable mt,
                                       int* __restrict__ move, double* __restrict__ e_out, double* __restrict__ z,
                                       unsigned* __restrict__ dir, double* __restrict__ u_leaf, double* __restrict__ u_tree) {
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
    uint32_t r[4];
    philox4x32_10(s_lo, s_hi, (uint32_t)gid, ALABI_NUTS_STREAM_DIR, k0, k1, r);
    dir[gid] = r[0];
    const int nl = (1 << depth) - 1;
    for (int b = 0; b < nl; ++b) u_leaf[(size_t)gid * nl + b] = nuts_uniform(s_lo, s_hi, (uint32_t)gid, ALABI_NUTS_STREAM_LEAF + 16u * (uint32_t)b, k0, k1);
    for (int j = 0; j < depth; ++j) u_tree[(size_t)gid * depth + j] = nuts_uniform(s_lo, s_hi, (uint32_t)gid, ALABI_NUTS_STREAM_TREE + 16u * (uint32_t)j, k0, k1);
}

template <int D, bool GENERIC>
static int launch_nuts_inst(const NutsArgs& a, int grid, int T, size_t lds, hipStream_t s) {
    if (lds > 32 * 1024) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(ens_nuts_kernel<D, GENERIC>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, ALABI_HMC_MAX_LDS);
        if (err != hipSuccess) return hip_fail(err, "hipFuncSetAttribute(ens_nuts_kernel)", __FILE__, __LINE__);
    }
    hipLaunchKernelGGL((ens_nuts_kernel<D, GENERIC>), dim3(grid), dim3(T), lds, s, a);
    return ALABI_OK;
}

// inj set: the test entry's single transition (K = 1) of move inj_k from injected draws
int launch_ens_nuts(alabi_ens* e, double* coords, double* logp, long long step0, long long done0, int K, int thin_by, double* chain,
                    double* chain_logp, long long* n_accept, const NutsInject* inj, hipStream_t s) {
    if (K <= 0) return ALABI_OK;
    const int db = dim_bucket(e->d);
    const size_t lds = nuts_lds_bytes(e);
    if (!e->all_nuts || !e->gauss_C || !e->nuts_counts || !e->nuts_accept || db < 0 || lds > ALABI_HMC_MAX_LDS) return ALABI_BAD_ARGUMENT;
    NutsArgs a{};
    a.h = hmc_args(e, coords, logp, step0, done0, K, thin_by, chain, chain_logp, n_accept);
    a.counts = e->nuts_counts; a.accept_sum = e->nuts_accept;
    if (inj) {
        a.h.inj_z = inj->z0; a.h.inj_e = inj->e; a.h.inj_k = inj->k;
        a.inj_dir = inj->dir; a.inj_uleaf = inj->u_leaf; a.inj_utree = inj->u_tree; a.trace = inj->trace;
    }
    if (!a.h.lg.Xt || !a.h.lg.alpha) return ALABI_NOT_COMPUTED;
    const int grid = e->W * e->E, T = hmc_threads(e);
    e->nuts_plan[0] = T; e->nuts_plan[1] = K; e->nuts_plan[2] = (int)lds; e->nuts_plan[3] = e->gp->Npad > T ? 1 : 0;
    int st = ALABI_OK;
    ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, st = (launch_nuts_inst<D, GENERIC>(a, grid, T, lds, s))));
    if (st != ALABI_OK) return st;
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_nuts_export(alabi_ens* e, long long step, int depth, int* move, double* e_out, double* z, unsigned* dir, double* u_leaf,
                           double* u_tree, hipStream_t s) {
    hipLaunchKernelGGL(ens_nuts_export_kernel, dim3((e->W * e->E + 255) / 256), dim3(256), 0, s, e->seed, step, e->W, e->E, e->d, depth,
                       e->moves, move, e_out, z, dir, u_leaf, u_tree);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // namespace alabi
