// No-U-Turn sampler ensemble for gfx950: W independent chains of multinomial NUTS (Betancourt 2017, as in Stan) on the surrogate's
// closed-form gradient (kind 7 of the move table, alabi_amd.moves.NUTSMove; tests/nuts_numpy.py is the CPU statement).
//
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
//   D = 1: 236 / 36 | 241 / 0     D = 5: 238 / 36 | 251 / 0     D = 10: 242 / 36 | 255 / 28    D = 16: 254 / 36 | 255 / 44
//   D = 20: 256 / 60 | 255 / 76   D = 24: 256 / 68 | 256 / 116  D = 32: 256 / 112 | 256 / 168
//   D = 48: 256 / 244 | 256 / 304 D = 64: 256 / 360 | 256 / 436
// The tree is 16 doubles per lane on top of ens_hmc_kernel's 180 to 230 VGPRs, live across the evaluation: from D = 20 on (from
// D = 8 for the other families) a part of it waits in scratch while the training set is read, stored once before and loaded once
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
    const HmcArgs& p = a.h;
    const int tid = threadIdx.x, T = blockDim.x, d = p.lg.d, ld = d | 1;
    const int w = blockIdx.x;                                       // global walker id
    const uint32_t g0 = (uint32_t)((w / p.W) * p.W);                // global id of the ensemble's walker 0
    double* w_s = nuts_lds + (size_t)p.mt.n * d * ld;
    double* ck_z = w_s + p.lg.Npad;                                 // [ALABI_NUTS_MAX_DEPTH][64] z of the block's first leaf
    double* ck_r = ck_z + ALABI_NUTS_MAX_DEPTH * 64;                // [ALABI_NUTS_MAX_DEPTH][64] running rho' including that leaf
    for (int idx = tid; idx < p.mt.n * d * d; idx += T) {
        const int m = idx / (d * d), rc = idx - m * d * d;
        nuts_lds[(size_t)m * d * ld + (rc / d) * ld + (rc % d)] = p.scale_C[idx];
    }
    const bool in = tid < d;                                        // wave 0 keeps the walker: lane k its coordinate k
    double xv = 0.0, inv_len = 0.0, lo = 0.0, hi = 0.0;
    if (in) {
        xv = p.coords[(size_t)w * d + tid];
        inv_len = p.lg.consts[tid];
        lo = p.lg.consts[ALABI_MAX_DIM + tid];
        hi = p.lg.consts[2 * ALABI_MAX_DIM + tid];
    }
    double lp_old = p.logp[w];
    long long nacc = 0, n_leaves = 0, n_depth = 0, n_div = 0;
    double a_sum = 0.0;
    if (tid < 64) {
        if (a.counts) { n_leaves = a.counts[(size_t)w * 3]; n_depth = a.counts[(size_t)w * 3 + 1]; n_div = a.counts[(size_t)w * 3 + 2]; }
        if (a.accept_sum) a_sum = a.accept_sum[w];
    }
    const uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32);
    const size_t WT = (size_t)gridDim.x;
    double gx, lp_unused;
    lp_grad_eval<D, GENERIC>(p.lg, w_s, qs_s, g_s, scratch, xv, inv_len, lp_unused, gx);   // its first barrier covers the factors
    for (int t = 0; t < p.K; ++t) {
        const long long step = p.step0 + t;
        const uint32_t s_lo = (uint32_t)step, s_hi = (uint32_t)((unsigned long long)step >> 32);
        const int mi = p.inj_z ? p.inj_k : hmc_step_move(p.mt, s_lo, s_hi, g0, k0, k1);   // workgroup-uniform
        double mp0, mp1;
        hmc_move_params(p.mt, mi, mp0, mp1);
        const int Dmax = hmc_leapfrog_of(mp1);                       // p1 = max_depth + ln jitter / 512
        const int nleaf_max = (1 << Dmax) - 1;
        const double* Cs = nuts_lds + (size_t)mi * d * ld;
        const int diagonal = (p.scale_diag >> mi) & 1;
        // wave 0's tree
        double e = 0.0, s = 0.0, H0 = 0.0, lnW = 0.0, lnWs = 0.0, lpp = lp_old, lpc = 0.0, lpq = 0.0;
        double qL = xv, zL = 0.0, gL = gx, qR = xv, zR = 0.0, gR = gx, rho = 0.0, rhoS = 0.0;
        double q = xv, z = 0.0, g = gx, qp = xv, gp = gx, qc = xv, gc = gx;
        uint32_t dirw = 0;
        int j = 0, n = 0, leaves = 0, depth = 0, reason = ALABI_NUTS_STOP_DEPTH, taken = 0;
        bool fwd = false;
        if (tid < 64) {
            if (p.inj_z) {
                e = p.inj_e;
                zL = in ? p.inj_z[(size_t)w * d + tid] : 0.0;
                dirw = a.inj_dir[w];
            } else {
                e = hmc_step_size(mp0, hmc_ln_jitter_of(mp1), s_lo, s_hi, g0, k0, k1);
                zL = in ? philox_normal(s_lo, s_hi, (uint32_t)w, ALABI_HMC_STREAM_Z + 16u * (uint32_t)tid, k0, k1) : 0.0;
                uint32_t r[4];
                philox4x32_10(s_lo, s_hi, (uint32_t)w, ALABI_NUTS_STREAM_DIR, k0, k1, r);
                dirw = r[0];
            }
            zR = zL; rho = zL;
            H0 = -lp_old + 0.5 * wave_total(zL * zL);
        }
        bool go;
        do {   // one leaf per trip; the trip count is the stop word's, the same for every thread
            if (tid < 64) {
                if (n == 0) {                                       // doubling j starts: from which end, which way
                    fwd = ((dirw >> j) & 1u) != 0u;
                    s = fwd ? e : -e;
                    q = fwd ? qR : qL; z = fwd ? zR : zL; g = fwd ? gR : gL;
                    rhoS = 0.0; lnWs = -INFINITY;
                }
                z = fma(0.5 * s, scale_transposed_times(Cs, diagonal, d, ld, tid, g), z);
                q = fma(s, scale_times(Cs, diagonal, d, ld, tid, z), q);
            }
            lp_grad_eval<D, GENERIC>(p.lg, w_s, qs_s, g_s, scratch, q, inv_len, lpq, g);
            if (tid < 64) {
                z = fma(0.5 * s, scale_transposed_times(Cs, diagonal, d, ld, tid, g), z);
                const double delta = H0 - (0.5 * wave_total(z * z) - lpq);
                const bool out = in && !((q > lo) && (q < hi));         // NaN is outside
                const bool inb = __ballot(out) == 0ull;
                int stop = 0;
                const int ordinal = leaves;
                ++leaves;
                if (!(delta > -1000.0)) {                               // divergent (NaN included): drop the subtree
                    reason = ALABI_NUTS_STOP_DIVERGENT; stop = 1; ++n_div;
                } else {
                    if (inb) {
                        a_sum += fmin(1.0, exp(delta));
                        lnWs = nuts_logaddexp(lnWs, delta);
                        const double ul = p.inj_z ? a.inj_uleaf[(size_t)w * nleaf_max + ordinal]
                                                  : nuts_uniform(s_lo, s_hi, (uint32_t)w, ALABI_NUTS_STREAM_LEAF + 16u * (uint32_t)ordinal, k0, k1);
                        if (log(ul) < delta - lnWs) { qc = q; gc = g; lpc = lpq; }
                    }
                    rhoS += z;
                    if ((n & 1) == 0) {                                 // slot popcount(n) <= Dmax - 2 < ALABI_NUTS_MAX_DEPTH
                        const int slot = __popc((unsigned)n);
                        ck_z[slot * 64 + tid] = z; ck_r[slot * 64 + tid] = rhoS;
                    } else {
                        const int base = __popc((unsigned)(n >> 1));
                        bool turn = false;
                        for (int i = 0; ((n >> i) & 1) != 0; ++i) {     // wave-uniform: t trailing one bits, slots base ... base - t + 1 >= 0
                            const double zf = ck_z[(base - i) * 64 + tid];
                            const double rb = rhoS - ck_r[(base - i) * 64 + tid] + zf;
                            const double d1 = wave_total(rb * zf), d2 = wave_total(rb * z);
                            if (d1 <= 0.0 || d2 <= 0.0) turn = true;
                        }
                        if (turn) { reason = ALABI_NUTS_STOP_SUBTREE; stop = 1; }
                    }
                    ++n;
                    if (!stop && n == (1 << j)) {                       // the subtree is complete: join it
                        if (lnWs > -INFINITY) {
                            const double ut = p.inj_z ? a.inj_utree[(size_t)w * Dmax + j]
                                                      : nuts_uniform(s_lo, s_hi, (uint32_t)w, ALABI_NUTS_STREAM_TREE + 16u * (uint32_t)j, k0, k1);
                            if (log(ut) < lnWs - lnW) { qp = qc; gp = gc; lpp = lpc; taken = 1; }
                        }
                        lnW = nuts_logaddexp(lnW, lnWs);
                        rho += rhoS;
                        if (fwd) { qR = q; zR = z; gR = g; } else { qL = q; zL = z; gL = g; }
                        depth = j + 1;
                        const double d1 = wave_total(rho * zL), d2 = wave_total(rho * zR);
                        if (d1 <= 0.0 || d2 <= 0.0) { reason = ALABI_NUTS_STOP_TREE; stop = 1; }
                        else if (depth == Dmax) { reason = ALABI_NUTS_STOP_DEPTH; stop = 1; }
                        ++j; n = 0;
                    }
                }
                if (tid == 0) stop_s = stop;
            }
            __syncthreads();
            go = stop_s == 0;
        } while (go);
        if (tid < 64) {
            xv = qp; lp_old = lpp; gx = gp;
            nacc += taken;
            n_leaves += leaves; n_depth += depth;
            if (a.trace && tid < 4) a.trace[(size_t)w * 4 + tid] = tid == 0 ? depth : tid == 1 ? leaves : tid == 2 ? reason : taken;
            if (p.chain || p.chain_logp) {
                const long long done = p.done0 + t + 1;
                if (done % p.thin_by == 0) {
                    const size_t slot = (size_t)(done / p.thin_by - 1);
                    if (p.chain && in) __builtin_nontemporal_store(xv, &p.chain[(slot * WT + w) * d + tid]);
                    if (p.chain_logp && tid == 0) __builtin_nontemporal_store(lp_old, &p.chain_logp[slot * WT + w]);
                }
            }
        }
    }
    if (tid >= 64) return;
    if (in) p.coords[(size_t)w * d + tid] = xv;
    if (tid == 0) {
        p.logp[w] = lp_old;
        if (p.n_accept) p.n_accept[w] += nacc;
        if (a.counts) { a.counts[(size_t)w * 3] = n_leaves; a.counts[(size_t)w * 3 + 1] = n_depth; a.counts[(size_t)w * 3 + 2] = n_div; }
        if (a.accept_sum) a.accept_sum[w] = a_sum;
    }
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
