// Gaussian Metropolis ensemble for gfx950: emcee's GaussianMove (moves/gaussian.py) as W independent Markov chains.
//
// A Metropolis proposal reads nothing but the walker itself, so an ensemble whose every move is a GaussianMove has no red-blue
// dependency chain: ens_mh_kernel runs ONE workgroup per walker (E W of them; any count, they never wait for each other and there
// are no spin loops) and every step of a chunk in one launch.  Per step: the step's move (stream 3 at the ensemble's walker 0),
// the scale factor and the coordinate (gauss_step_draws), d normals, the proposal q = x + f C z (gauss_coord), the box gate, the
// ensemble's log-probability -- GP mean, affine map, y map, normal priors, -inf outside the open box -- and the accept test
// lp' - lp > ln u' (NaN rejects).  tests/gaussian_move_numpy.py is the CPU statement.
//
// The kernel has ens_half_kernel's shape, so that the launch-per-half-step path (path 0) and this one (path 4) give the same bits:
// the same workgroup size (alabi_ens::threads), the lane's training-set share in VGPRs (points 2 tid, 2 tid + 1 of every coordinate
// row; se_pair_terms' h for the squared exponential, inputs + alpha for the other families), the same streamed tiles where
// Npad / 2 exceeds the block (half_lane_sum), the same wave_sum_dpp -> LDS -> wave_sum_dpp reduction, the same proposal code.
// What it saves is everything around the sum: the share is loaded once per chunk, not once per proposal, the walker and its
// log-probability stay in registers, and a step costs two barriers instead of two launches.
//
// LDS: the scale factors of the table's moves, [n][d, d] doubles (32 KB per move at d = 64; a table that needs more than
// ALABI_MH_MAX_LDS runs on path 0), plus 0.9 KB.  VGPRs: __launch_bounds__(512) leaves 256 per lane, the resident share takes
// 4 D + 4 of them.  hipcc -Rpass-analysis=kernel-resource-usage: 238 / 248 VGPRs (squared exponential / the other families) and no
// scratch at the d = 10 bucket, 256 from the d = 12 bucket on, where part of the share lives in scratch (132 bytes per lane at
// d = 16, 1.5 - 2 KB at d = 64), as it does in ens_half_kernel; two waves per SIMD throughout.
#include <cstdlib>
#include "ens_device.hpp"

namespace alabi {

// ALABI_MH_MAX_LDS: ens_shared.hpp

struct MhArgs {
    double* coords;              // [E*W, d] in/out
    double* logp;                // [E*W] in/out
    const double* consts;        // device [5][ALABI_MAX_DIM]: inv_len, lo, hi, prior mean, prior 1 / std
    const double* Xsrc;          // [D, Npad] scaled inputs (squared exponential: relative to their mean)
    const double* Asrc;          // [Npad] alpha (squared exponential: h of se_pair_terms)
    const double* centre;        // [d] mean of the scaled inputs (squared exponential)
    double* chain;               // [nstore, E*W, d] or null
    double* chain_logp;          // [nstore, E*W] or null
    long long* n_accept;         // [E*W] or null
    const double* gauss_C;       // [n][d, d] scale factors of the table's moves
    long long step0;             // global step index of local step 0
    long long done0;             // steps of the call done before this launch (chain slots)
    unsigned long long seed;
    int K, W, d, Npad, thin_by, has_prior, ymap, gauss_diag;
    double prior_const, amp, mean;
    KernelFn kf;
    MoveTable mt;
};

template <int D, bool GENERIC>
__global__ void __launch_bounds__(512)
ens_mh_kernel(MhArgs p) {
    extern __shared__ __attribute__((aligned(16))) double mh_C[];   // [n][d, d]
    __shared__ double qs_s[ALABI_MAX_DIM];
    __shared__ double scratch[16];
    const int tid = threadIdx.x, T = blockDim.x, d = p.d;
    const int w = blockIdx.x;                                       // global walker id
    const uint32_t g0 = (uint32_t)((w / p.W) * p.W);                // global id of the ensemble's walker 0
    // the lane's share of the training set: issued first, resident for every step of the launch
    const int half = p.Npad >> 1;
    const bool vA = tid < half;
    f64x2 xa[D];
#pragma unroll
    for (int k = 0; k < D; ++k)
        xa[k] = vA ? reinterpret_cast<const f64x2*>(p.Xsrc + (size_t)k * p.Npad)[tid] : f64x2{0.0, 0.0};
    const f64x2 aa = vA ? reinterpret_cast<const f64x2*>(p.Asrc)[tid] : (GENERIC ? f64x2{0.0, 0.0} : f64x2{ALABI_SE_PAD, ALABI_SE_PAD});
    const int nC = p.mt.n * d * d;
    for (int idx = tid; idx < nC; idx += T) mh_C[idx] = p.gauss_C[idx];
    // wave 0 keeps the walker: lane k its coordinate k, every lane its log-probability
    const bool in = tid < d;
    double xv = 0.0, inv_len = 0.0, lo = 0.0, hi = 0.0, ctr = 0.0;
    if (in) {
        xv = p.coords[(size_t)w * d + tid];
        inv_len = p.consts[tid];
        lo = p.consts[ALABI_MAX_DIM + tid];
        hi = p.consts[2 * ALABI_MAX_DIM + tid];
        if (!GENERIC) ctr = p.centre[tid];
    }
    double lp_old = p.logp[w];
    long long nacc = 0;
    const uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32);
    const size_t WT = (size_t)gridDim.x;
    __syncthreads();
    for (int t = 0; t < p.K; ++t) {
        int ok = 1;
        double qc = 0.0, lnu = 0.0;
        if (tid < 64) {
            const long long step = p.step0 + t;
            const uint32_t s_lo = (uint32_t)step, s_hi = (uint32_t)((unsigned long long)step >> 32);
            uint32_t r[4];
            // the step's move, as ens_draw_kernel chooses it (the table is read with constant indices only)
            int mi = 0;
            if (p.mt.n > 1) {
                philox4x32_10(s_lo, s_hi, g0, 3u, k0, k1, r);
                const double um = u53(r[0], r[1]);
#pragma unroll
                for (int k = 0; k < ALABI_MAX_MOVES; ++k) mi += (k < p.mt.n && p.mt.cum[k] <= um) ? 1 : 0;
                if (mi > p.mt.n - 1) mi = p.mt.n - 1;
            }
            double mp0 = p.mt.p0[0], mp1 = p.mt.p1[0];
#pragma unroll
            for (int k = 1; k < ALABI_MAX_MOVES; ++k)
                if (k == mi) { mp0 = p.mt.p0[k]; mp1 = p.mt.p1[k]; }
            double f;
            int c;
            gauss_step_draws(s_lo, s_hi, g0, (uint32_t)w, k0, k1, step, mp0, (int)mp1, d, f, c);
            const double z = in ? philox_normal(s_lo, s_hi, (uint32_t)w, 10u + 16u * (uint32_t)tid, k0, k1) : 0.0;
            qc = gauss_coord(mh_C + (size_t)mi * d * d, (p.gauss_diag >> mi) & 1, d, tid, xv, z, f, c);
            philox4x32_10(s_lo, s_hi, (uint32_t)w, 2u, k0, k1, r);
            lnu = log(u53(r[0], r[1]));
            double qv = 0.0;
            if (in) {
                ok = (qc > lo) && (qc < hi);
                qv = qc * inv_len;
                if (!GENERIC) qv -= ctr;
            }
            if (tid < D) qs_s[tid] = qv;
        }
        const int inb = __syncthreads_and(ok);
        if (inb) {  // workgroup-uniform
            double q[D];
#pragma unroll
            for (int k = 0; k < D; ++k) q[k] = qs_s[k];
            const double acc = half_lane_sum<D, GENERIC>(xa, aa, q, p.Xsrc, p.Asrc, p.Npad, tid, T, p.kf);
            const double wsum = wave_sum_dpp(acc);
            if ((tid & 63) == 63) scratch[tid >> 6] = wsum;
        }
        __syncthreads();       // the wave partials are in LDS; behind it every wave has read qs_s, so wave 0 may write the next proposal
        if (tid >= 64) continue;
        double lp_new = -INFINITY;
        if (inb) {
            const int nw = T >> 6;
            double part = (tid < nw) ? scratch[tid] : 0.0;
            part = wave_sum_dpp(part);   // fixed order: bit-reproducible
            const double s = lane_bcast(part, 63);
            lp_new = fma(p.amp, s, p.mean);
            if (p.ymap) lp_new = apply_ymap(lp_new, p.ymap);
            if (p.has_prior)
                lp_new += normal_prior_sum(p.consts + 3 * ALABI_MAX_DIM, p.consts + 4 * ALABI_MAX_DIM, tid, d, qc) + p.prior_const;
        }
        if (0.0 + lp_new - lp_old > lnu) {   // the log factor of a symmetric proposal; false for NaN
            xv = qc;
            lp_old = lp_new;
            ++nacc;
        }
        if (p.chain || p.chain_logp) {
            const long long done = p.done0 + t + 1;
            if (done % p.thin_by == 0) {
                const size_t slot = (size_t)(done / p.thin_by - 1);
                if (p.chain && in) __builtin_nontemporal_store(xv, &p.chain[(slot * WT + w) * d + tid]);
                if (p.chain_logp && tid == 0) __builtin_nontemporal_store(lp_old, &p.chain_logp[slot * WT + w]);
            }
        }
    }
    if (tid >= 64) return;
    if (in) p.coords[(size_t)w * d + tid] = xv;
    if (tid == 0) {
        p.logp[w] = lp_old;
        if (p.n_accept) p.n_accept[w] += nacc;
    }
}

// (steps per launch: ens_mh_chunk in ens_plan.hip)

template <int D, bool GENERIC>
static int launch_mh_inst(const MhArgs& a, int grid, int T, size_t lds, hipStream_t s) {
    if (lds > 32 * 1024) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(ens_mh_kernel<D, GENERIC>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, ALABI_MH_MAX_LDS);
        if (err != hipSuccess) return hip_fail(err, "hipFuncSetAttribute(ens_mh_kernel)", __FILE__, __LINE__);
    }
    hipLaunchKernelGGL((ens_mh_kernel<D, GENERIC>), dim3(grid), dim3(T), lds, s, a);
    return ALABI_OK;
}

int launch_ens_mh(alabi_ens* e, double* coords, double* logp, long long step0, long long done0, int K, int thin_by, double* chain,
                  double* chain_logp, long long* n_accept, hipStream_t s) {
    if (K <= 0) return ALABI_OK;
    alabi_gp* gp = e->gp;
    const int db = dim_bucket(e->d);
    const bool se = gp->kf.type == 0;
    MhArgs a{};
    a.coords = coords; a.logp = logp; a.consts = e->consts;
    a.Xsrc = se ? gp->Xc : gp->Xt; a.Asrc = se ? gp->ens_h : gp->alpha; a.centre = gp->xa_centre;
    a.chain = chain; a.chain_logp = chain_logp; a.n_accept = n_accept;
    a.gauss_C = e->gauss_C;
    a.step0 = step0 + done0; a.done0 = done0; a.seed = e->seed;
    a.K = K; a.W = e->W; a.d = e->d; a.Npad = gp->Npad; a.thin_by = thin_by;
    a.has_prior = e->has_prior; a.ymap = e->ymap; a.gauss_diag = e->gauss_diag;
    a.prior_const = e->prior_const;
    a.amp = e->lp_scale * std::exp(gp->log_amp); a.mean = std::fma(e->lp_scale, gp->mean, e->lp_shift); a.kf = gp->kf;
    a.mt = e->moves;
    if (!a.Xsrc || !a.Asrc || (se && !a.centre)) return ALABI_NOT_COMPUTED;
    const int grid = e->W * e->E, T = e->threads;
    const size_t lds = (size_t)ens_mh_lds_bytes(e->moves.n, e->d);
    e->mh_plan[0] = T; e->mh_plan[1] = K; e->mh_plan[2] = (int)lds; e->mh_plan[3] = (gp->Npad >> 1) > T ? 1 : 0;
    int st = ALABI_OK;
    ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(gp->kf.type, st = (launch_mh_inst<D, GENERIC>(a, grid, T, lds, s))));
    if (st != ALABI_OK) return st;
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // namespace alabi
