// Nested sampling on the GP surrogate for gfx950: the constrained random walks (dynesty's "rwalk") that replace the
// likelihood calls of dynesty's NestedSampler / DynamicNestedSampler as driven by the reference's run_dynesty
// (alabi/core.py:2417-2787; likelihood = surrogate_log_likelihood, core.py:1446-1508).  The nested-sampling loop itself
// (which points die, the live-point covariance, L*, the weights, the evidence) runs on the host: alabi_amd/nested.py.
//
// The sampler works in the unit cube u in [0,1]^d.  The prior is uniform on the box [lo, lo + width] in the GP's scaled
// coordinates (the caller folds an affine theta scaler into lo / width; width may be negative), so
//   x = lo + u * width,   logL(u) = map(amp * sum_n alpha_n k(x, x_n) + mean)
// with amp / mean carrying an affine y scaler and map the inverse of the nlog / log scalers (apply_ymap) -- exactly the
// log-probability of the ensemble kernels without the prior term.
//
// Kernels
//   ns_walk_kernel<D, GENERIC, TMAX, TILED>  one workgroup per walk; all `walks` Metropolis steps inside one launch (walks never talk to
//                               each other).  The workgroup's share of the training set -- centred inputs + h for the squared
//                               exponential (se_pair_terms), inputs + alpha for the other families, one point pair per lane, the
//                               layout of ens_half_kernel -- is loaded once into VGPRs and used for every step.  When Npad / 2
//                               exceeds the block size the pairs beyond it are re-read from L2 at every step (the tiled path).
//                               TILED selects that path at compile time (the resident path carries no loop registers);
//                               TMAX is the launch bound: 1024 lanes for buckets <= 16, 256 above.
//                               Per step: d normals (Philox4x32-10 + Box-Muller, below), u' = u + scale * C z with the
//                               Cholesky factor C of the live points' covariance held in LDS, the cube gate 0 < u' < 1, the
//                               GP mean at x(u'), accept iff logL(u') > L*.  A walk that accepts nothing returns its start
//                               bit for bit.
//   ns_prior_kernel             uniform points in the cube.
//   ns_propose_kernel           the proposal of one step of every walk (host-callable likelihoods): the same draws and the same
//                               arithmetic as the fused walk (shared functions below), so both paths move identically.
//   ns_accept_kernel            the accept test of one step, given the host's logL of the proposals.
//
// Draws.  Everything is keyed by (seed, call, global walk id, step): counter (c0, c1, c2, c3) = ((uint32) call, walk id, step,
// j), key = (low, high 32 bits of seed).  Normals: pair j (coordinates 2j, 2j+1) from one Philox block r[0..3]:
//   u1 = u53(r0, r1), u2 = u53(r2, r3), rad = sqrt(-2 log(1 - u1)), z_2j = rad cos(2 pi u2), z_2j+1 = rad sin(2 pi u2).
// Prior draws use step = 0xFFFFFFFF: coordinate 2j = u53(r0, r1), 2j+1 = u53(r2, r3).  Splitting the walks of one call into
// several launches (walk_id0 offsets) therefore gives bit-identical results.
#include <cmath>
#include <new>
#include "ens_device.hpp"

struct alabi_ns {
    alabi_gp* gp = nullptr;
    int d = 0;
    unsigned long long seed = 0;
    alabi::DimVec lo{}, width{};
    double lp_scale = 1.0, lp_shift = 0.0;
    int ymap = 0;
    int last_path = 0;   // 1 register-resident training set, 2 tiled (pairs beyond the block size re-read from L2 every step)
};

namespace alabi {

#define ALABI_NS_PRIOR_STEP 0xFFFFFFFFu

struct NsArgs {
    const double* Xsrc;          // squared exponential: gp->Xc (centred inputs), else gp->Xt
    const double* Asrc;          // squared exponential: gp->ens_h, else gp->alpha
    const double* centre;        // gp->xa_centre
    int Npad;
    KernelFn kf;
    double amp, mean;
    int ymap;
    DimVec lo, width, inv_len;
    const double* u0;            // [K, d]
    const double* logl0;         // [K] or NULL: evaluate the start points first
    const double* chol;          // [d, d] row-major, lower triangle read
    double* u_out;               // [K, d] (may alias u0)
    double* logl_out;            // [K]
    int* n_acc;                  // [2K] or NULL: accepted steps, likelihood evaluations
    unsigned long long seed;
    long long call;
    int walk_id0, K, d, walks;
    double logl_star, scale;
};

// Normals 2j and 2j+1 of step `step` of walk `wid`.
__device__ inline void ns_normal_pair(unsigned long long seed, long long call, uint32_t wid, uint32_t step, uint32_t j,
                                      double& z0, double& z1) {
    uint32_t r[4];
    philox4x32_10((uint32_t)call, wid, step, j, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const double u1 = u53(r[0], r[1]), u2 = u53(r[2], r[3]);
    const double rad = sqrt(-2.0 * log(1.0 - u1));
    const double ang = 6.283185307179586 * u2;
    z0 = rad * cos(ang);
    z1 = rad * sin(ang);
}

// Lanes 0 .. ceil(d/2)-1 of the calling wave write the step's normals to z_s[0 .. d).
__device__ inline void ns_draw_normals(unsigned long long seed, long long call, uint32_t wid, uint32_t step, int d, int lane,
                                       double* z_s) {
    if (2 * lane < d) {
        double z0, z1;
        ns_normal_pair(seed, call, wid, step, (uint32_t)lane, z0, z1);
        z_s[2 * lane] = z0;
        if (2 * lane + 1 < d) z_s[2 * lane + 1] = z1;
    }
}

// Coordinate k of the proposal u + scale * C z (C lower triangular, row stride ldc).
__device__ inline double ns_prop_coord(const double* C, int ldc, const double* z, int k, double u, double scale) {
    double acc = 0.0;
    for (int i = 0; i <= k; ++i) acc = fma(C[(size_t)k * ldc + i], z[i], acc);
    return u + scale * acc;
}

// GP coordinate (scaled by the inverse length scales; centred for the squared exponential) of cube coordinate k.
template <bool GENERIC>
__device__ inline double ns_gp_coord(const NsArgs& p, int k, double u) {
    double x = fma(u, p.width.v[k], p.lo.v[k]) * p.inv_len.v[k];
    if (!GENERIC) x -= p.centre[k];
    return x;
}

// logL at the point in qs_s: the kernel sum of ens_half_kernel (first pair from the registers xa / aa, further pairs from L2),
// wave totals by DPP, one barrier, wave 0 adds the partials.  Called by every thread; the result is valid in wave 0.
template <int D, bool GENERIC, bool TILED>
__device__ inline double ns_logl(const NsArgs& p, const f64x2 (&xa)[D], f64x2 aa, const double* qs_s, double* scratch) {
    const int tid = threadIdx.x, T = blockDim.x, half = p.Npad >> 1;
    double q[D];
#pragma unroll
    for (int k = 0; k < D; ++k) q[k] = qs_s[k];
    double acc;
    if (!GENERIC) {
        const double nhq = se_neg_half_norm<D>(q);
        double fa, fb;
        se_pair_terms<D>(xa, aa, q, nhq, fa, fb);
        acc = 0.0; acc += fa; acc += fb;
        for (int j = tid + T; TILED && j < half; j += T) {
            f64x2 x[D];
#pragma unroll
            for (int k = 0; k < D; ++k) x[k] = reinterpret_cast<const f64x2*>(p.Xsrc + (size_t)k * p.Npad)[j];
            se_pair_terms<D>(x, reinterpret_cast<const f64x2*>(p.Asrc)[j], q, nhq, fa, fb);
            acc += fa; acc += fb;
        }
    } else {
        double r2a = 0.0, r2b = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double da = xa[k].x - q[k], db = xa[k].y - q[k];
            r2a = fma(da, da, r2a);
            r2b = fma(db, db, r2b);
        }
        acc = aa.x * radial<GENERIC>(r2a, p.kf);
        acc = fma(aa.y, radial<GENERIC>(r2b, p.kf), acc);
        for (int j = tid + T; TILED && j < half; j += T) {
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const f64x2 x = reinterpret_cast<const f64x2*>(p.Xsrc + (size_t)k * p.Npad)[j];
                const double d0 = x.x - q[k], d1 = x.y - q[k];
                s0 = fma(d0, d0, s0);
                s1 = fma(d1, d1, s1);
            }
            const f64x2 al = reinterpret_cast<const f64x2*>(p.Asrc)[j];
            acc = fma(al.x, radial<GENERIC>(s0, p.kf), acc);
            acc = fma(al.y, radial<GENERIC>(s1, p.kf), acc);
        }
    }
    const double wsum = wave_sum_dpp(acc);
    if ((tid & 63) == 63) scratch[tid >> 6] = wsum;
    __syncthreads();
    double lp = 0.0;
    if (tid < 64) {
        double part = (tid < (T >> 6)) ? scratch[tid] : 0.0;
        part = wave_sum_dpp(part);   // fixed order: bit-reproducible
        const double s = lane_bcast(part, 63);
        lp = fma(p.amp, s, p.mean);
        if (p.ymap) lp = apply_ymap(lp, p.ymap);
    }
    return lp;
}

// TMAX: 1024 lanes for dimension buckets <= 16, 256 above (the register budget of xa[D] and the query), see ns_threads.
template <int D, bool GENERIC, int TMAX, bool TILED>
__global__ void __launch_bounds__(TMAX)
ns_walk_kernel(NsArgs p) {
    __shared__ double C_s[D * D];
    __shared__ double u_s[D], up_s[D], qs_s[D], z_s[D];
    __shared__ double scratch[16];
    __shared__ double L_s;
    __shared__ int acc_s, nev_s;
    const int tid = threadIdx.x, T = blockDim.x, b = blockIdx.x, d = p.d;
    const uint32_t wid = (uint32_t)(p.walk_id0 + b);
    // the training-set share of this lane: issued first, resident for the whole walk
    const int half = p.Npad >> 1;
    const bool vA = tid < half;
    f64x2 xa[D];
#pragma unroll
    for (int k = 0; k < D; ++k)
        xa[k] = vA ? reinterpret_cast<const f64x2*>(p.Xsrc + (size_t)k * p.Npad)[tid] : f64x2{0.0, 0.0};
    const f64x2 aa = vA ? reinterpret_cast<const f64x2*>(p.Asrc)[tid] : (GENERIC ? f64x2{0.0, 0.0} : f64x2{ALABI_SE_PAD, ALABI_SE_PAD});
    for (int i = tid; i < D * D; i += T) {
        const int r = i / D, c = i % D;
        C_s[i] = (r < d && c <= r && p.walks > 0) ? p.chol[(size_t)r * d + c] : 0.0;
    }
    if (tid < D) {
        const double u = tid < d ? p.u0[(size_t)b * d + tid] : 0.0;
        u_s[tid] = u;
        z_s[tid] = 0.0;
        qs_s[tid] = tid < d ? ns_gp_coord<GENERIC>(p, tid, u) : 0.0;
    }
    if (tid == 0) { L_s = p.logl0 ? p.logl0[b] : -INFINITY; acc_s = 0; nev_s = 0; }
    __syncthreads();
    // step -1 evaluates start points given without a logL (one inlined copy of the kernel sum: a second one for the start
    // pushed the D = 10 instantiation from 128 VGPRs into scratch)
    for (int s = p.logl0 ? 0 : -1; s < p.walks; ++s) {
        int ok = 1;
        if (s >= 0) {
            if (tid < 64) ns_draw_normals(p.seed, p.call, wid, (uint32_t)s, d, tid, z_s);
            __syncthreads();
            if (tid < d) {
                const double up = ns_prop_coord(C_s, D, z_s, tid, u_s[tid], p.scale);
                ok = (up > 0.0) && (up < 1.0);
                up_s[tid] = up;
                qs_s[tid] = ns_gp_coord<GENERIC>(p, tid, up);
            }
        }
        const int inb = __syncthreads_and(ok);
        if (inb) {                                       // workgroup-uniform
            const double lp = ns_logl<D, GENERIC, TILED>(p, xa, aa, qs_s, scratch);
            if (s < 0) {
                if (tid == 0) L_s = lp;
            } else {
                if (tid < 64 && lp > p.logl_star) {     // false for NaN
                    if (tid < d) u_s[tid] = up_s[tid];
                    if (tid == 0) { L_s = lp; acc_s += 1; }
                }
                if (tid == 0) nev_s += 1;
            }
        }
        __syncthreads();
    }
    if (tid < d) p.u_out[(size_t)b * d + tid] = u_s[tid];
    if (tid == 0) {
        p.logl_out[b] = L_s;
        if (p.n_acc) { p.n_acc[b] = acc_s; p.n_acc[p.K + b] = nev_s; }
    }
}

__global__ void __launch_bounds__(256)
ns_prior_kernel(unsigned long long seed, long long call, int walk_id0, int n, int d, double* __restrict__ u_out) {
    const int npair = (d + 1) / 2;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n * npair) return;
    const int i = (int)(t / npair), j = (int)(t % npair);
    uint32_t r[4];
    philox4x32_10((uint32_t)call, (uint32_t)(walk_id0 + i), ALABI_NS_PRIOR_STEP, (uint32_t)j, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    u_out[(size_t)i * d + 2 * j] = u53(r[0], r[1]);
    if (2 * j + 1 < d) u_out[(size_t)i * d + 2 * j + 1] = u53(r[2], r[3]);
}

// One 64-lane workgroup per walk: the normals and the proposal exactly as ns_walk_kernel forms them.
__global__ void __launch_bounds__(64)
ns_propose_kernel(unsigned long long seed, long long call, int walk_id0, int d, int step, const double* __restrict__ chol,
                  double scale, const double* __restrict__ u_cur, double* __restrict__ u_prop) {
    __shared__ double C_s[ALABI_MAX_DIM * ALABI_MAX_DIM];
    __shared__ double z_s[ALABI_MAX_DIM];
    const int tid = threadIdx.x, b = blockIdx.x;
    for (int i = tid; i < d * d; i += 64) {
        const int r = i / d, c = i % d;
        C_s[r * ALABI_MAX_DIM + c] = c <= r ? chol[i] : 0.0;
    }
    ns_draw_normals(seed, call, (uint32_t)(walk_id0 + b), (uint32_t)step, d, tid, z_s);
    __syncthreads();
    if (tid < d) u_prop[(size_t)b * d + tid] = ns_prop_coord(C_s, ALABI_MAX_DIM, z_s, tid, u_cur[(size_t)b * d + tid], scale);
}

__global__ void __launch_bounds__(256)
ns_accept_kernel(int K, int d, const double* __restrict__ u_prop, const double* __restrict__ logl_prop, double logl_star,
                 double* __restrict__ u_cur, double* __restrict__ logl_cur, int* __restrict__ n_acc) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= K) return;
    bool inside = true;
    for (int k = 0; k < d; ++k) {
        const double v = u_prop[(size_t)b * d + k];
        inside = inside && (v > 0.0) && (v < 1.0);
    }
    const double lp = logl_prop[b];
    if (inside && lp > logl_star) {
        for (int k = 0; k < d; ++k) u_cur[(size_t)b * d + k] = u_prop[(size_t)b * d + k];
        logl_cur[b] = lp;
        if (n_acc) n_acc[b] += 1;
    }
    if (n_acc && inside) n_acc[K + b] += 1;
}

}  // namespace alabi

using namespace alabi;

static inline hipStream_t ns_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Block size of the walk kernel: one training-point pair per lane when Npad / 2 <= 1024 (the register-resident path), 1024 lanes
// otherwise (pairs beyond them re-read from L2 each step).  Dimension buckets above 16 use at most 256 lanes, and their
// instantiations are compiled for 256 (ns_tmax) so that xa[D] gets the registers of a 256-lane block.
static constexpr int ns_tmax(int db) { return db <= 16 ? 1024 : 256; }
static int ns_threads(const alabi_gp* gp, int db) {
    const int half = gp->Npad / 2, cap = ns_tmax(db);
    int T = round_up(half, 64);
    if (T < 64) T = 64;
    return T < cap ? T : cap;
}

extern "C" {

int alabi_ns_create(alabi_gp* gp, int d, const double* bounds, unsigned long long seed, alabi_ns** out) {
    if (!gp || !out || !bounds || d < 1 || d > ALABI_MAX_DIM || d != gp->d) return ALABI_BAD_ARGUMENT;
    for (int k = 0; k < d; ++k) {
        const double lo = bounds[2 * k], hi = bounds[2 * k + 1];
        if (!std::isfinite(lo) || !std::isfinite(hi) || lo == hi) return ALABI_BAD_ARGUMENT;
    }
    alabi_ns* n = new (std::nothrow) alabi_ns();
    if (!n) return ALABI_BAD_ARGUMENT;
    n->gp = gp; n->d = d; n->seed = seed;
    for (int k = 0; k < ALABI_MAX_DIM; ++k) {
        n->lo.v[k] = k < d ? bounds[2 * k] : 0.0;
        n->width.v[k] = k < d ? bounds[2 * k + 1] - bounds[2 * k] : 0.0;
    }
    *out = n;
    return ALABI_OK;
}

int alabi_ns_destroy(alabi_ns* ns) {
    delete ns;
    return ALABI_OK;
}

int alabi_ns_set_logp(alabi_ns* ns, double scale, double shift, int map_kind) {
    if (!ns || !(scale > 0.0) || !std::isfinite(scale) || !std::isfinite(shift) || map_kind < 0 || map_kind > 2)
        return ALABI_BAD_ARGUMENT;
    ns->lp_scale = scale; ns->lp_shift = shift; ns->ymap = map_kind;
    return ALABI_OK;
}

int alabi_ns_last_path(alabi_ns* ns, int* path) {
    if (!ns || !path) return ALABI_BAD_ARGUMENT;
    *path = ns->last_path;
    return ALABI_OK;
}

int alabi_ns_walk(alabi_ns* ns, long long call, int walk_id0, const double* u0, const double* logl0, int K, double logl_star,
                  const double* chol, double scale, int walks, double* u_out, double* logl_out, int* n_accept, void* stream) {
    if (!ns || K < 0 || walks < 0 || walk_id0 < 0 || call < 0 || std::isnan(logl_star)) return ALABI_BAD_ARGUMENT;
    if ((long long)walk_id0 + K > 0xFFFFFFFFLL) return ALABI_BAD_ARGUMENT;
    if (K == 0) return ALABI_OK;
    if (!u0 || !u_out || !logl_out || (walks > 0 && (!chol || !(scale > 0.0) || !std::isfinite(scale)))) return ALABI_BAD_ARGUMENT;
    alabi_gp* gp = ns->gp;
    if (!gp->computed || !gp->has_alpha) return ALABI_NOT_COMPUTED;
    const hipStream_t s = ns_stream(stream);
    const bool se = gp->kf.type == 0;
    if (se) { const int st = ens_se_prepare(gp, s); if (st != ALABI_OK) return st; }
    NsArgs a{};
    a.Xsrc = se ? gp->Xc : gp->Xt; a.Asrc = se ? gp->ens_h : gp->alpha; a.centre = gp->xa_centre;
    a.Npad = gp->Npad; a.kf = gp->kf;
    a.amp = ns->lp_scale * std::exp(gp->log_amp); a.mean = std::fma(ns->lp_scale, gp->mean, ns->lp_shift); a.ymap = ns->ymap;
    a.lo = ns->lo; a.width = ns->width; a.inv_len = gp->inv_len;
    a.u0 = u0; a.logl0 = logl0; a.chol = chol; a.u_out = u_out; a.logl_out = logl_out; a.n_acc = n_accept;
    a.seed = ns->seed; a.call = call; a.walk_id0 = walk_id0; a.K = K; a.d = ns->d; a.walks = walks;
    a.logl_star = logl_star; a.scale = scale;
    const int db = dim_bucket(ns->d), T = ns_threads(gp, db);
    ns->last_path = (gp->Npad / 2 <= T) ? 1 : 2;
    if (ns->last_path == 1) {
        ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(gp->kf.type,
            hipLaunchKernelGGL((ns_walk_kernel<D, GENERIC, ns_tmax(D), false>), dim3(K), dim3(T), 0, s, a)));
    } else {
        ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(gp->kf.type,
            hipLaunchKernelGGL((ns_walk_kernel<D, GENERIC, ns_tmax(D), true>), dim3(K), dim3(T), 0, s, a)));
    }
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int alabi_ns_prior_draw(alabi_ns* ns, long long call, int walk_id0, int n, double* u_out, double* logl_out, void* stream) {
    if (!ns || !u_out || n < 0 || walk_id0 < 0 || call < 0 || (long long)walk_id0 + n > 0xFFFFFFFFLL) return ALABI_BAD_ARGUMENT;
    if (n == 0) return ALABI_OK;
    const hipStream_t s = ns_stream(stream);
    const long long threads = (long long)n * ((ns->d + 1) / 2);
    hipLaunchKernelGGL(ns_prior_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, ns->seed, call, walk_id0, n, ns->d, u_out);
    ALABI_LAUNCH_CHECK();
    if (!logl_out) return ALABI_OK;
    return alabi_ns_walk(ns, call, walk_id0, u_out, nullptr, n, -INFINITY, nullptr, 1.0, 0, u_out, logl_out, nullptr, stream);
}

int alabi_ns_propose(alabi_ns* ns, long long call, int walk_id0, const double* u_cur, int K, int step, const double* chol,
                     double scale, double* u_prop, void* stream) {
    if (!ns || K < 0 || step < 0 || walk_id0 < 0 || call < 0 || (long long)walk_id0 + K > 0xFFFFFFFFLL) return ALABI_BAD_ARGUMENT;
    if (K == 0) return ALABI_OK;
    if (!u_cur || !u_prop || !chol || !(scale > 0.0) || !std::isfinite(scale)) return ALABI_BAD_ARGUMENT;
    hipLaunchKernelGGL(ns_propose_kernel, dim3(K), dim3(64), 0, ns_stream(stream), ns->seed, call, walk_id0, ns->d, step, chol, scale,
                       u_cur, u_prop);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int alabi_ns_accept(alabi_ns* ns, int K, const double* u_prop, const double* logl_prop, double logl_star, double* u_cur,
                    double* logl_cur, int* n_accept, void* stream) {
    if (!ns || K < 0 || std::isnan(logl_star)) return ALABI_BAD_ARGUMENT;
    if (K == 0) return ALABI_OK;
    if (!u_prop || !logl_prop || !u_cur || !logl_cur) return ALABI_BAD_ARGUMENT;
    hipLaunchKernelGGL(ns_accept_kernel, dim3((K + 255) / 256), dim3(256), 0, ns_stream(stream), K, ns->d, u_prop, logl_prop, logl_star,
                       u_cur, logl_cur, n_accept);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // extern "C"
