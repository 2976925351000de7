// Maximum of the ensemble's fused log-probability for gfx950: a multi-start projected BFGS ascent on the surrogate's closed-form
// gradient (alabi_ens_maximize; tests/map_numpy.py is the CPU statement and the specification), and the closed-form Hessian of the
// same log-probability (alabi_ens_log_prob_hessian; tests/hess_reference.py is its truth).
//
// A search reads nothing but its own point, like an HMC trajectory, so ens_map_kernel has ens_hmc_kernel's shape: ONE workgroup per
// start (any count; no spin loops, no atomics, no traffic between workgroups) and every iteration of the search in one launch.
// Wave 0 keeps the point, its gradient and the search direction, lane k coordinate k; value and gradient come from lp_grad_eval
// (ens_grad_device.hpp), the log-probability WITHOUT the box gate, as HMC uses it.  The method is the projected quasi-Newton ascent
// that utility_polish.hip documents for the acquisition polish, with a dense BFGS approximation B of the inverse of -Hessian in
// place of the two-loop recursion; on the shrunk box [lo', hi'] = [lo + 1e-9 w, hi - 1e-9 w], w = hi - lo:
//     start      outside the OPEN box, or value or gradient not finite: status 3, outputs NaN.  Otherwise x = clip(x0).
//     held       x_k on a face of the shrunk box and the gradient pointing outward; pg = g with the held coordinates zeroed.
//     stop       max|pg| <= gtol: status 0; then maxiter steps taken: status 1.
//     reset      B = diag(0.1 w_k / max|pg|) at the start, when the held set changes, when p is no ascent direction and for the
//                second attempt of a failed search.
//     direction  p = B pg on the free coordinates.
//     search     t = 1, 1/2, ... (30 trials at the most): xn = clip(x + t p), step = xn - x, dd = g . step; accepted when
//                fn >= f + 1e-4 dd (Armijo on the projected step); where |fn - f| <= 1e-8 max(1, |f|) the values cannot tell and
//                the gradient decides: gn . step >= -(1 - 2e-4) dd, which on a parabola is the same condition.  A failed search is
//                repeated once along the projected gradient with B reset; then status 2, the point kept.
//     update     s = step, y = g - gn on the free coordinates, applied only when s.y > 1e-10 |s| |y|: a fresh B becomes
//                (s.y / y.y) I, then B <- B - rho (s (By)^T + (By) s^T) + rho (1 + rho y.By) s s^T.  s, y and rho are temporaries in
//                registers: nothing of B is written when the update is refused.
//     result     never worse than the (clipped) start.
// Every sum runs in a fixed order (lp_grad_eval's; wave_sum_dpp over the coordinates; a lane's row of B by fma, j ascending), so a
// start gives the same bits wherever it stands in the batch.  The control flow of the search lives in wave 0; one LDS word and one
// barrier per evaluation tell the other waves whether another evaluation follows.
//
// LDS: B [d][d | 1] doubles (odd row stride, as HMC's scale factors; a lane touches its own row only) and the weights [Npad]
// doubles, together at most 128 KB (alabi_ens_maximize refuses more with ALABI_BAD_ARGUMENT: there is no other kernel for it),
// plus 1.2 KB.  ens_lp_hess_kernel: two weight arrays [Npad], at most 128 KB, plus the pair sums (17.5 KB).
// hipcc -Rpass-analysis=kernel-resource-usage for ens_map_kernel, VGPRs / scratch bytes per lane (squared exponential | the other
// families), __launch_bounds__(512) leaves 256 VGPRs per lane:
//   D = 1: 155 / 0 | 170 / 0     D = 2: 158 / 0 | 173 / 0     D = 3: 162 / 0 | 175 / 0     D = 4: 170 / 0 | 181 / 0
//   D = 5: 170 / 0 | 179 / 0     D = 6: 148 / 0 | 181 / 0     D = 8: 150 / 0 | 185 / 0     D = 10: 154 / 0 | 189 / 0
//   D = 12: 158 / 0 | 193 / 0    D = 16: 166 / 0 | 201 / 0    D = 20: 174 / 0 | 209 / 0    D = 24: 182 / 0 | 217 / 0
//   D = 32: 198 / 0 | 233 / 0    D = 48: 230 / 0 | 254 / 36   D = 64: 256 / 20 | 256 / 144
// The floor is lp_grad_eval's unrolled point loop; the query point costs 2 D of them, and from the D = 48 bucket on a part of it
// lives in scratch, as in ens_hmc_kernel.  ens_lp_hess_kernel: 43 ... 170 | 92 ... 244 VGPRs, no scratch in any bucket.
#include <cmath>
#include "ens_hess_device.hpp"

namespace alabi {

#define ALABI_MAP_ARMIJO 1e-4
#define ALABI_MAP_FLAT 1e-8
#define ALABI_MAP_CURV 1e-10
#define ALABI_MAP_SHRINK 1e-9
#define ALABI_MAP_FIRST 0.1
#define ALABI_MAP_LS_MAX 30

struct MapArgs {
    LpGradArgs lg;
    const double* starts;        // [S, d]
    double* x_out;               // [S, d]
    double* lp_out;              // [S]
    int* iters_out;              // [S, 2]: iterations, evaluations
    int* status_out;             // [S]
    double* gnorm_out;           // [S]
    double* trace;               // [S, ntrace, 4]: lp, t, held mask (the bits of a 64-bit integer), updated; or null
    int maxiter, ntrace;
    double gtol;
};

template <int D, bool GENERIC>
__global__ void __launch_bounds__(512)
ens_map_kernel(MapArgs p) {
    extern __shared__ __attribute__((aligned(16))) double map_lds[];   // [d][ld] B | [Npad] weights
    __shared__ double qs_s[ALABI_MAX_DIM], g_s[ALABI_MAX_DIM];
    __shared__ double scratch[16];
    __shared__ int more_s;
    const int tid = threadIdx.x, d = p.lg.d, ld = d | 1, m = blockIdx.x;
    double* Bs = map_lds;
    double* w_s = map_lds + (size_t)d * ld;
    const bool in = tid < d;                                        // wave 0 keeps the point: lane k its coordinate k
    double x = 0.0, inv_len = 0.0, los = 0.0, his = 0.0, wd = 0.0;
    int status = -1;                                                // -1: the search goes on
    if (tid < 64) {
        bool outside = false;
        if (in) {
            x = p.starts[(size_t)m * d + tid];
            inv_len = p.lg.consts[tid];
            const double lo = p.lg.consts[ALABI_MAX_DIM + tid], hi = p.lg.consts[2 * ALABI_MAX_DIM + tid];
            wd = hi - lo;
            los = lo + ALABI_MAP_SHRINK * wd; his = hi - ALABI_MAP_SHRINK * wd;
            outside = !((x > lo) && (x < hi));                      // NaN is outside
            x = fmin(fmax(x, los), his);
        }
        if (__ballot(outside) != 0ull) status = 3;
    }
    // wave 0's state (the other waves carry the initial values and never read them)
    double f = 0.0, g = 0.0, pg = 0.0, pk = 0.0, step = 0.0, q = x, t = 1.0, dd = 0.0, gnorm = 0.0, f_start = 0.0, x_start = x;
    int phase = 0, it = 0, nev = 0, ls = 0, attempt = 0;            // phase 0: the start's evaluation is awaited; 2: a trial's
    bool fresh = true, held = false, have_prev = false;
    unsigned long long mask = 0ull, prev = 0ull;
    for (;;) {
        if (tid == 0) more_s = status < 0 ? 1 : 0;
        __syncthreads();
        if (!more_s) break;                                         // (the evaluation's three barriers stand before the next write)
        double lpq, gq;
        lp_grad_eval<D, GENERIC>(p.lg, w_s, qs_s, g_s, scratch, q, inv_len, lpq, gq);
        if (tid >= 64) continue;
        ++nev;
        const bool finite = isfinite(lpq) && __ballot(in && !isfinite(gq)) == 0ull;
        if (phase == 0) {
            if (!finite) { status = 3; continue; }
            f = lpq; g = gq; f_start = f;
            phase = 1;
        } else {
            bool ok = false;
            if (finite) {
                const double scale = fmax(1.0, fabs(f));
                const double dn = wave_total(gq * step);
                if (fabs(lpq - f) <= ALABI_MAP_FLAT * scale) ok = dn >= -(1.0 - 2.0 * ALABI_MAP_ARMIJO) * dd;
                else ok = lpq >= f + ALABI_MAP_ARMIJO * dd;
            }
            if (ok) {
                const double yk = (in && !held) ? g - gq : 0.0;
                const double sy = wave_total(step * yk), ss = wave_total(step * step), yy = wave_total(yk * yk);
                const bool upd = sy > ALABI_MAP_CURV * sqrt(ss * yy);
                if (upd) {
                    if (fresh) { bfgs_row_diagonal(Bs, d, ld, tid, sy / yy); fresh = false; }
                    const double rho = 1.0 / sy;
                    const double By = bfgs_row_times(Bs, d, ld, tid, yk);
                    const double c = rho * (1.0 + rho * wave_total(yk * By));
                    for (int j = 0; j < d; ++j) {
                        const double sj = lane_bcast(step, j), Byj = lane_bcast(By, j);
                        if (in) Bs[tid * ld + j] = Bs[tid * ld + j] - rho * (step * Byj + By * sj) + c * (step * sj);
                    }
                }
                x = q; f = lpq; g = gq;
                if (p.trace && it < p.ntrace && tid == 0) {
                    double* tr = p.trace + ((size_t)m * p.ntrace + it) * 4;
                    tr[0] = f; tr[1] = t; tr[2] = __longlong_as_double((long long)mask); tr[3] = upd ? 1.0 : 0.0;
                }
                ++it;
                phase = 1;
            } else {
                t *= 0.5; ++ls;
                phase = 2;
            }
        }
        // advance to the next point to evaluate, or to the end of the search
        for (;;) {
            if (phase == 1) {                                       // a new iteration at (x, f, g)
                held = in && ((x <= los && g < 0.0) || (x >= his && g > 0.0));
                mask = __ballot(held);
                pg = (in && !held) ? g : 0.0;
                gnorm = wave_max(fabs(pg));
                if (gnorm <= p.gtol) { status = 0; break; }
                if (it >= p.maxiter) { status = 1; break; }
                if (have_prev && mask != prev) fresh = true;
                prev = mask; have_prev = true;
                attempt = 0;
                phase = 3;
            }
            if (phase == 3) {                                       // the direction
                if (fresh) bfgs_row_diagonal(Bs, d, ld, tid, ALABI_MAP_FIRST * wd / gnorm);
                pk = held ? 0.0 : bfgs_row_times(Bs, d, ld, tid, pg);
                if (!(wave_total(pg * pk) > 0.0)) {
                    bfgs_row_diagonal(Bs, d, ld, tid, ALABI_MAP_FIRST * wd / gnorm);
                    fresh = true;
                    pk = held ? 0.0 : bfgs_row_times(Bs, d, ld, tid, pg);
                }
                t = 1.0; ls = 0;
                phase = 2;
            }
            bool fail = ls >= ALABI_MAP_LS_MAX;                     // phase 2: the next trial
            double xn = x;
            if (!fail) {
                if (in && !held) xn = fmin(fmax(x + t * pk, los), his);
                step = xn - x;
                fail = __ballot(step != 0.0) == 0ull;               // no coordinate moves
            }
            if (fail) {
                if (attempt == 0 && !fresh) { attempt = 1; fresh = true; phase = 3; continue; }
                status = 2;
                break;
            }
            dd = wave_total(g * step);
            q = xn;
            break;
        }
    }
    if (tid >= 64) return;
    if (status == 3) { x = NAN; f = NAN; gnorm = NAN; it = 0; }
    else if (f < f_start) { x = x_start; f = f_start; }
    if (in) p.x_out[(size_t)m * d + tid] = x;
    if (tid == 0) {
        p.lp_out[m] = f;
        p.iters_out[2 * m] = it; p.iters_out[2 * m + 1] = nev;
        p.status_out[m] = status;
        p.gnorm_out[m] = gnorm;
    }
}

// The Hessian of the fused log-probability at M arbitrary points, one workgroup per point (lp_hess_eval: ens_hess_device.hpp).
// With Mu the mean after the folded affine map: identity H = grad^2 Mu; y map L = -+10^Mu: H = ln10 L grad^2 Mu + ln10^2 L grad Mu
// grad Mu^T; a normal prior on coordinate k subtracts 1 / s_k^2 on the diagonal.  The full symmetric [d, d] is written, entry (a, b)
// and (b, a) by the same arithmetic on the same operands; outside the open box all of it is NaN.
template <int D, bool GENERIC>
__global__ void __launch_bounds__(512)
ens_lp_hess_kernel(LpGradArgs lg, const double* __restrict__ pts, double* __restrict__ hess) {
    extern __shared__ __attribute__((aligned(16))) double hess_lds[];   // [Npad] u1 | [Npad] u2
    __shared__ double qs_s[ALABI_MAX_DIM], G_s[ALABI_MAX_DIM];
    __shared__ double S_s[ALABI_MAX_DIM * (ALABI_MAX_DIM + 1) / 2];
    __shared__ double scratch[16];
    __shared__ int out_s;
    const int tid = threadIdx.x, T = blockDim.x, d = lg.d, m = blockIdx.x;
    const bool in = tid < d;
    double xv = 0.0, inv_len = 0.0;
    if (tid < 64) {
        bool outside = false;
        if (in) {
            xv = pts[(size_t)m * d + tid];
            inv_len = lg.consts[tid];
            outside = !((xv > lg.consts[ALABI_MAX_DIM + tid]) && (xv < lg.consts[2 * ALABI_MAX_DIM + tid]));
        }
        const unsigned long long o = __ballot(outside);
        if (tid == 0) out_s = o != 0ull ? 1 : 0;
    }
    lp_hess_eval<D, GENERIC>(lg, hess_lds, hess_lds + lg.Npad, qs_s, S_s, G_s, scratch, xv, inv_len);
    const bool outside = out_s != 0;
    double L = 0.0;
    if (lg.ymap) {                                                  // every thread: the wave partials in a fixed order
        double s = 0.0;
        for (int w = 0; w < (T >> 6); ++w) s += scratch[w];
        L = apply_ymap(fma(lg.amp, s, lg.mean), lg.ymap);
    }
    const double ln10 = 2.302585092994046;
    const double* pistd = lg.consts + 4 * ALABI_MAX_DIM;
    for (int idx = tid; idx < d * d; idx += T) {
        const int r = idx / d, c = idx - r * d, a = r < c ? r : c, b = r < c ? c : r;
        const double ia = lg.consts[a], ib = lg.consts[b];
        double h = lg.amp * (ia * ib) * S_s[hess_pair_index(a, b, d)];
        if (lg.ymap) {
            const double ga = lg.amp * ia * G_s[a], gb = lg.amp * ib * G_s[b];
            h = ln10 * L * h + (ln10 * ln10) * L * (ga * gb);
        }
        if (lg.has_prior && a == b) { const double is = pistd[a]; h -= is * is; }
        hess[(size_t)m * d * d + idx] = outside ? NAN : h;
    }
}

static int map_threads(const alabi_ens* e) { return e->threads > 512 ? 512 : e->threads; }
static size_t map_lds_bytes(const alabi_ens* e) { return ((size_t)e->d * (e->d | 1) + (size_t)e->gp->Npad) * sizeof(double); }

// what lp_grad_eval reads of the handle (as ens_hmc.hip folds it: amp = lp_scale e^log_amp, mean = fma(lp_scale, mean, lp_shift))
static LpGradArgs map_lp_args(const alabi_ens* e) {
    const alabi_gp* gp = e->gp;
    LpGradArgs a{};
    a.Xt = gp->Xt; a.alpha = gp->alpha; a.consts = e->consts;
    a.d = e->d; a.Npad = gp->Npad; a.has_prior = e->has_prior; a.ymap = e->ymap;
    a.prior_const = e->prior_const;
    a.amp = e->lp_scale * std::exp(gp->log_amp); a.mean = std::fma(e->lp_scale, gp->mean, e->lp_shift); a.kf = gp->kf;
    return a;
}

void ens_map_plan(const alabi_ens* e, int* out) {
    const size_t lds = map_lds_bytes(e);
    out[0] = map_threads(e); out[1] = lds > 0x7fffffffull ? 0x7fffffff : (int)lds; out[2] = e->gp->Npad > map_threads(e) ? 1 : 0;
    out[3] = dim_bucket(e->d);
}

template <int D, bool GENERIC>
static int launch_map_inst(const MapArgs& a, int S, int T, size_t lds, hipStream_t s) {
    if (lds > 32 * 1024) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(ens_map_kernel<D, GENERIC>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, ALABI_HMC_MAX_LDS);
        if (err != hipSuccess) return hip_fail(err, "hipFuncSetAttribute(ens_map_kernel)", __FILE__, __LINE__);
    }
    hipLaunchKernelGGL((ens_map_kernel<D, GENERIC>), dim3(S), dim3(T), lds, s, a);
    return ALABI_OK;
}

int launch_ens_map(alabi_ens* e, const double* starts, int S, int maxiter, double gtol, double* x_out, double* lp_out, int* iters_out,
                   int* status_out, double* gnorm_out, double* trace, int ntrace, hipStream_t s) {
    if (S <= 0) return ALABI_OK;
    const int db = dim_bucket(e->d);
    const size_t lds = map_lds_bytes(e);
    if (db < 0 || lds > ALABI_HMC_MAX_LDS) return ALABI_BAD_ARGUMENT;
    MapArgs a{};
    a.lg = map_lp_args(e);
    a.starts = starts; a.x_out = x_out; a.lp_out = lp_out; a.iters_out = iters_out; a.status_out = status_out; a.gnorm_out = gnorm_out;
    a.trace = ntrace > 0 ? trace : nullptr; a.maxiter = maxiter; a.ntrace = ntrace; a.gtol = gtol;
    if (!a.lg.Xt || !a.lg.alpha) return ALABI_NOT_COMPUTED;
    int st = ALABI_OK;
    ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, st = (launch_map_inst<D, GENERIC>(a, S, map_threads(e), lds, s))));
    if (st != ALABI_OK) return st;
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

template <int D, bool GENERIC>
static int launch_lp_hess_inst(const LpGradArgs& a, const double* pts, int M, double* hess, int T, size_t lds, hipStream_t s) {
    if (lds > 32 * 1024) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(ens_lp_hess_kernel<D, GENERIC>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, ALABI_HMC_MAX_LDS);
        if (err != hipSuccess) return hip_fail(err, "hipFuncSetAttribute(ens_lp_hess_kernel)", __FILE__, __LINE__);
    }
    hipLaunchKernelGGL((ens_lp_hess_kernel<D, GENERIC>), dim3(M), dim3(T), lds, s, a, pts, hess);
    return ALABI_OK;
}

int launch_ens_lp_hess(alabi_ens* e, const double* pts, int M, double* hess, hipStream_t s) {
    if (M <= 0) return ALABI_OK;
    const int db = dim_bucket(e->d);
    const size_t lds = 2 * (size_t)e->gp->Npad * sizeof(double);
    if (db < 0 || lds > ALABI_HMC_MAX_LDS) return ALABI_BAD_ARGUMENT;
    const LpGradArgs a = map_lp_args(e);
    if (!a.Xt || !a.alpha) return ALABI_NOT_COMPUTED;
    int st = ALABI_OK;
    ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, st = (launch_lp_hess_inst<D, GENERIC>(a, pts, M, hess, map_threads(e), lds, s))));
    if (st != ALABI_OK) return st;
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // namespace alabi
