// What ens_nuts_kernel (ens_nuts.hip), ens_nuts_adapt_kernel and ens_step_search_kernel (ens_nuts_adapt.hip) and their launchers
// share: the arguments, the draws' streams, the LDS layout, the small helpers of the tree and nuts_walker_transitions, the body of
// both NUTS kernels.  ens_hmc_device.hpp (HmcArgs, HmcAdaptArgs, the step's move and step size) and ens_grad_device.hpp
// (lp_grad_eval, the products with a scale factor) are included read-only: ens_hmc_kernel and ens_hmc_adapt_kernel keep their code
// and their bits.
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

// ens_nuts_adapt_kernel keeps the dual-averaging state in static LDS, one copy per lane of wave 0 (every lane the same values,
// each reading and writing its own column): the words of the state, then the sum of a_t, then this transition's sum of a
#define ALABI_NUTS_DA_SUM ALABI_HMC_DA_WORDS
#define ALABI_NUTS_DA_LEAVES (ALABI_HMC_DA_WORDS + 1)
#define ALABI_NUTS_DA_ROWS (ALABI_HMC_DA_WORDS + 2)

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

// K transitions of walker blockIdx.x (ens_nuts.hip's header has the arithmetic, the draws and the barrier rule).  nuts_lds: [n][d, ld]
// scale factors | [Npad] weights | checkpoints (dynamic); qs_s, g_s [ALABI_MAX_DIM], scratch [16], stop_s: static LDS of the kernel.
// ADAPT (da_s [ALABI_NUTS_DA_ROWS][64], static LDS): a transition runs with e = exp(ln e_w) f instead of p0 f, every leaf adds its a
// to the transition's own sum as well, and behind the transition, with a_t = that sum / the transition's leaves,
//     m <- m + 1;   H-bar <- (1 - 1 / (m + t0)) H-bar + (delta - a_t) / (m + t0);   ln e <- mu - (sqrt(m) / gamma) H-bar
//     ln e-bar <- m^-kappa ln e + (1 - m^-kappa) ln e-bar
// in every lane of wave 0 alike (hmc_walker_steps' update).  The state lives in LDS and not in registers: it is touched once per
// transition, and the tree already fills the register file across the evaluation.  It is read from global memory at the start of
// the launch and written at its end, and the sum of a_t grows from what was read: the chunk length changes no bit of either.
template <int D, bool GENERIC, bool ADAPT>
__device__ __forceinline__ void nuts_walker_transitions(const NutsArgs& a, const HmcAdaptArgs& ad, double* nuts_lds, double* qs_s, double* g_s,
                                                        double* scratch, int* stop_s, double* da_s) {
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
        if (ADAPT) {                                                // this lane's column; only this lane touches it again
            const double* st = ad.state + (size_t)w * ALABI_HMC_DA_WORDS;
#pragma unroll
            for (int i = 0; i < ALABI_HMC_DA_WORDS; ++i) da_s[i * 64 + tid] = st[i];
            da_s[ALABI_NUTS_DA_SUM * 64 + tid] = ad.accept_stat ? ad.accept_stat[w] : 0.0;
        }
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
                e = hmc_step_size(ADAPT ? exp(da_s[2 * 64 + tid]) : mp0, hmc_ln_jitter_of(mp1), s_lo, s_hi, g0, k0, k1);
                zL = in ? philox_normal(s_lo, s_hi, (uint32_t)w, ALABI_HMC_STREAM_Z + 16u * (uint32_t)tid, k0, k1) : 0.0;
                uint32_t r[4];
                philox4x32_10(s_lo, s_hi, (uint32_t)w, ALABI_NUTS_STREAM_DIR, k0, k1, r);
                dirw = r[0];
            }
            zR = zL; rho = zL;
            H0 = -lp_old + 0.5 * wave_total(zL * zL);
            if (ADAPT) da_s[ALABI_NUTS_DA_LEAVES * 64 + tid] = 0.0;
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
                        const double al = fmin(1.0, exp(delta));
                        a_sum += al;
                        if (ADAPT) da_s[ALABI_NUTS_DA_LEAVES * 64 + tid] += al;
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
                if (tid == 0) *stop_s = stop;
            }
            __syncthreads();
            go = *stop_s == 0;
        } while (go);
        if (tid < 64) {
            xv = qp; lp_old = lpp; gx = gp;
            nacc += taken;
            n_leaves += leaves; n_depth += depth;
            if (ADAPT) {                                                // no barrier in here; leaves >= 1
                double* c = da_s + tid;
                const double at = c[ALABI_NUTS_DA_LEAVES * 64] / (double)leaves;
                c[ALABI_NUTS_DA_SUM * 64] += at;
                const double m = c[0] + 1.0;
                const double h = (1.0 - 1.0 / (m + ad.t0)) * c[1 * 64] + (ad.delta - at) / (m + ad.t0);
                const double le = c[4 * 64] - (sqrt(m) / ad.gamma) * h;
                const double mk = pow(m, -ad.kappa);
                c[0] = m; c[1 * 64] = h; c[2 * 64] = le;
                c[3 * 64] = mk * le + (1.0 - mk) * c[3 * 64];
            }
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
        if (ADAPT) {
            double* st = ad.state + (size_t)w * ALABI_HMC_DA_WORDS;
#pragma unroll
            for (int i = 0; i < ALABI_HMC_DA_WORDS; ++i) st[i] = da_s[i * 64];
            if (ad.accept_stat) ad.accept_stat[w] = da_s[ALABI_NUTS_DA_SUM * 64];
        }
    }
}

// ---- host side
inline size_t nuts_lds_bytes(const alabi_ens* e) { return ens_nuts_lds_bytes(e->moves.n, e->d, e->gp->Npad); }

}  // namespace alabi
