// The body that ens_hmc_kernel (ens_hmc.hip) and ens_hmc_adapt_kernel (ens_hmc_adapt.hip) share: every step of a chunk for ONE
// walker by one workgroup, and what both launchers fill in.  ens_hmc.hip's header has the arithmetic and the draws; ADAPT adds the
// dual-averaging state of the step size (Hoffman & Gelman 2014, algorithm 5) that wave 0 keeps beside the walker.
#pragma once
#include "ens_grad_device.hpp"

namespace alabi {

// ALABI_HMC_MAX_LDS: ens_shared.hpp
#define ALABI_HMC_STREAM_Z 11u
#define ALABI_HMC_STREAM_JITTER 12u

struct HmcArgs {
    double* coords;              // [E*W, d] in/out
    double* logp;                // [E*W] in/out
    LpGradArgs lg;
    double* chain;               // [nstore, E*W, d] or null
    double* chain_logp;          // [nstore, E*W] or null
    long long* n_accept;         // [E*W] or null
    const double* scale_C;       // [n][d, d] scale factors of the table's moves
    long long step0;             // global step index of local step 0
    long long done0;             // steps of the call done before this launch (chain slots)
    unsigned long long seed;
    int K, W, thin_by, scale_diag;
    MoveTable mt;
    // test entry (alabi_ens_step_with_randoms_hmc): inj_z set -> one step of move inj_k with e = inj_e, z0 = inj_z [W, d], u' = inj_u [W]
    const double* inj_z;
    const double* inj_u;
    double inj_e;
    int inj_k;
};

// ens_hmc_adapt_kernel: the dual-averaging state per walker and its parameters
#define ALABI_HMC_DA_WORDS 5
struct HmcAdaptArgs {
    double* state;               // [E*W, 5] in/out: m (steps since the last restart), H-bar, ln e, ln e-bar, mu
    double* accept_stat;         // [E*W] or null: the sum of the steps' acceptance statistics is added
    double delta, gamma, t0, kappa;
};

// the step's move, as ens_draw_kernel chooses it (the table is read with constant indices only); every thread of the workgroup
__device__ __forceinline__ int hmc_step_move(const MoveTable& mt, uint32_t s_lo, uint32_t s_hi, uint32_t g0, uint32_t k0, uint32_t k1) {
    int mi = 0;
    if (mt.n > 1) {
        uint32_t r[4];
        philox4x32_10(s_lo, s_hi, g0, 3u, k0, k1, r);
        const double um = u53(r[0], r[1]);
#pragma unroll
        for (int k = 0; k < ALABI_MAX_MOVES; ++k) mi += (k < mt.n && mt.cum[k] <= um) ? 1 : 0;
        if (mi > mt.n - 1) mi = mt.n - 1;
    }
    return mi;
}
__device__ __forceinline__ void hmc_move_params(const MoveTable& mt, int mi, double& mp0, double& mp1) {
    mp0 = mt.p0[0]; mp1 = mt.p1[0];
#pragma unroll
    for (int k = 1; k < ALABI_MAX_MOVES; ++k)
        if (k == mi) { mp0 = mt.p0[k]; mp1 = mt.p1[k]; }
}
// e = step_size f of the step (one draw per step and ensemble, at its walker 0)
__device__ __forceinline__ double hmc_step_size(double eps, double ln_jitter, uint32_t s_lo, uint32_t s_hi, uint32_t g0, uint32_t k0, uint32_t k1) {
    if (ln_jitter == 0.0) return eps;
    uint32_t r[4];
    philox4x32_10(s_lo, s_hi, g0, ALABI_HMC_STREAM_JITTER, k0, k1, r);
    return eps * exp((2.0 * u53(r[0], r[1]) - 1.0) * ln_jitter);
}

// K steps of walker blockIdx.x.  hmc_lds: [n][d, ld] scale factors | [Npad] weights (dynamic); qs_s, g_s [ALABI_MAX_DIM], scratch [16].
// ADAPT: the step runs with e = exp(ln e_w) f instead of p0 f, and behind the accept test
//     a = min(1, exp(dh)), 0 outside the open box or for a NaN;   m <- m + 1
//     H-bar <- (1 - 1 / (m + t0)) H-bar + (delta - a) / (m + t0);   ln e <- mu - (sqrt(m) / gamma) H-bar
//     ln e-bar <- m^-kappa ln e + (1 - m^-kappa) ln e-bar
// in every lane of wave 0 alike.  The state and the sum of a are read at the start of the launch and written at its end, and the
// sum grows step by step from what was read: the chunk length changes no bit of either.
template <int D, bool GENERIC, bool ADAPT>
__device__ __forceinline__ void hmc_walker_steps(const HmcArgs& p, const HmcAdaptArgs& ad, double* hmc_lds, double* qs_s, double* g_s,
                                                 double* scratch) {
    const int tid = threadIdx.x, T = blockDim.x, d = p.lg.d, ld = d | 1;
    const int w = blockIdx.x;                                       // global walker id
    const uint32_t g0 = (uint32_t)((w / p.W) * p.W);                // global id of the ensemble's walker 0
    double* w_s = hmc_lds + (size_t)p.mt.n * d * ld;
    for (int idx = tid; idx < p.mt.n * d * d; idx += T) {
        const int m = idx / (d * d), rc = idx - m * d * d;
        hmc_lds[(size_t)m * d * ld + (rc / d) * ld + (rc % d)] = p.scale_C[idx];
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
    long long nacc = 0;
    double da_m = 0.0, da_h = 0.0, da_le = 0.0, da_lb = 0.0, da_mu = 0.0, da_sum = 0.0;
    if (ADAPT && tid < 64) {
        const double* st = ad.state + (size_t)w * ALABI_HMC_DA_WORDS;
        da_m = st[0]; da_h = st[1]; da_le = st[2]; da_lb = st[3]; da_mu = st[4];
        if (ad.accept_stat) da_sum = ad.accept_stat[w];
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
        const int L = hmc_leapfrog_of(mp1);
        const double* Cs = hmc_lds + (size_t)mi * d * ld;
        const int diagonal = (p.scale_diag >> mi) & 1;
        double e = 0.0, z0 = 0.0, z = 0.0, lnu = 0.0, q = xv, gq = gx, lpq = lp_old;
        if (tid < 64) {
            if (p.inj_z) {
                e = p.inj_e;
                z0 = in ? p.inj_z[(size_t)w * d + tid] : 0.0;
                lnu = log(p.inj_u[w]);
            } else {
                e = hmc_step_size(ADAPT ? exp(da_le) : mp0, hmc_ln_jitter_of(mp1), s_lo, s_hi, g0, k0, k1);
                z0 = in ? philox_normal(s_lo, s_hi, (uint32_t)w, ALABI_HMC_STREAM_Z + 16u * (uint32_t)tid, k0, k1) : 0.0;
                uint32_t r[4];
                philox4x32_10(s_lo, s_hi, (uint32_t)w, 2u, k0, k1, r);
                lnu = log(u53(r[0], r[1]));
            }
            z = fma(0.5 * e, scale_transposed_times(Cs, diagonal, d, ld, tid, gx), z0);
        }
        for (int l = 0; l < L; ++l) {   // workgroup-uniform trip count
            if (tid < 64) q = fma(e, scale_times(Cs, diagonal, d, ld, tid, z), q);
            lp_grad_eval<D, GENERIC>(p.lg, w_s, qs_s, g_s, scratch, q, inv_len, lpq, gq);
            if (tid < 64) z = fma(l == L - 1 ? 0.5 * e : e, scale_transposed_times(Cs, diagonal, d, ld, tid, gq), z);
        }
        if (tid >= 64) continue;
        const bool out = in && !((q > lo) && (q < hi));             // NaN is outside
        const bool inb = __ballot(out) == 0ull;
        const double ke0 = 0.5 * wave_total(z0 * z0), ke1 = 0.5 * wave_total(z * z);
        const double dh = lpq - ke1 - lp_old + ke0;
        if (inb && dh > lnu) {                                      // false for NaN
            xv = q; lp_old = lpq; gx = gq;
            ++nacc;
        }
        if (ADAPT) {
            const double a = (inb && dh == dh) ? fmin(1.0, exp(dh)) : 0.0;
            da_sum += a;
            da_m += 1.0;
            da_h = (1.0 - 1.0 / (da_m + ad.t0)) * da_h + (ad.delta - a) / (da_m + ad.t0);
            da_le = da_mu - (sqrt(da_m) / ad.gamma) * da_h;
            const double mk = pow(da_m, -ad.kappa);
            da_lb = mk * da_le + (1.0 - mk) * da_lb;
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
        if (ADAPT) {
            double* st = ad.state + (size_t)w * ALABI_HMC_DA_WORDS;
            st[0] = da_m; st[1] = da_h; st[2] = da_le; st[3] = da_lb; st[4] = da_mu;
            if (ad.accept_stat) ad.accept_stat[w] = da_sum;
        }
    }
}

// ---- host side: what both launchers fill in
inline size_t hmc_lds_bytes(const alabi_ens* e) { return ens_hmc_lds_bytes(e->moves.n, e->d, e->gp->Npad); }
inline int hmc_threads(const alabi_ens* e) { return e->threads > 512 ? 512 : e->threads; }
// (steps per launch: ens_hmc_chunk in ens_plan.hip)

inline LpGradArgs lp_grad_args(const alabi_ens* e) {
    const alabi_gp* gp = e->gp;
    LpGradArgs a{};
    a.Xt = gp->Xt; a.alpha = gp->alpha; a.consts = e->consts;
    a.d = e->d; a.Npad = gp->Npad; a.has_prior = e->has_prior; a.ymap = e->ymap;
    a.prior_const = e->prior_const;
    a.amp = e->lp_scale * std::exp(gp->log_amp); a.mean = std::fma(e->lp_scale, gp->mean, e->lp_shift); a.kf = gp->kf;
    return a;
}

inline HmcArgs hmc_args(const alabi_ens* e, double* coords, double* logp, long long step0, long long done0, int K, int thin_by, double* chain,
                        double* chain_logp, long long* n_accept) {
    HmcArgs a{};
    a.coords = coords; a.logp = logp; a.lg = lp_grad_args(e);
    a.chain = chain; a.chain_logp = chain_logp; a.n_accept = n_accept;
    a.scale_C = e->gauss_C;
    a.step0 = step0 + done0; a.done0 = done0; a.seed = e->seed;
    a.K = K; a.W = e->W; a.thin_by = thin_by; a.scale_diag = e->gauss_diag;
    a.mt = e->moves;
    return a;
}

}  // namespace alabi
