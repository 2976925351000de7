// Code shared by the nested-sampling translation units (nested.hip: the random walk and the slice move; nested_unif.hip: uniform
// draws inside bounding ellipsoids; nested_mlf.hip: the MLFriends region over them).  Device: the sampler handle, the kernel
// arguments, the Philox normals, the Cholesky factor of the one-wave kernels (ns_load_chol), the inverse normal CDF, the prior
// transform, the GP mean at one point (ns_logl) and the ellipsoid candidate (ns_unif_candidate).  Host: the block-size rule, the
// dispatch of the four templated kernels (ns_dispatch), the GP part of NsArgs (ns_point_args) and the launch path of both draw
// entries (ns_draw_launch).  The templated kernels keep their bodies, share load and D x D Cholesky load included, in their own
// files: NOTES.md "Nested sampling".  The draw layout (which Philox counter feeds which draw) is stated in nested.hip.
#pragma once
#include <cmath>
#include "ens_device.hpp"

struct alabi_ns {
    alabi_gp* gp = nullptr;
    int d = 0;
    unsigned long long seed = 0;
    alabi::DimVec lo{}, width{};             // normal coordinate (bit of nmask set): mean, std
    alabi::DimVec box_lo{}, box_width{};     // the box given to alabi_ns_create
    unsigned long long nmask = 0;
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
    unsigned long long nmask;    // coordinates with a normal prior: lo = mean, width = std
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

// The 64 lanes of a one-wave workgroup: the lower triangle of the Cholesky factor chol [d, d] into C_s with row stride ldc, zero above
// the diagonal (a barrier must follow).  Only the [d, d] block is written, which is all that ns_prop_coord and ns_slice_advance read.
__device__ __forceinline__ void ns_load_chol(double* C_s, int ldc, const double* chol, int d) {
    for (int i = threadIdx.x; i < d * d; i += 64) {
        const int r = i / d, c = i % d;
        C_s[r * ldc + c] = c <= r ? chol[i] : 0.0;
    }
}

// AS 241 PPND16: numerator, denominator (constant term 1 first) for |p - 1/2| <= 0.425 in r = 0.180625 - (p - 1/2)^2; for
// r = sqrt(-log(min(p, 1 - p))) <= 5 in r - 1.6; for r > 5 in r - 5.  Coefficients in ascending order.
#define ALABI_NS_NDTRI_COEFS 48
static __constant__ double ns_ndtri_coef[ALABI_NS_NDTRI_COEFS] = {
    3.3871328727963666080, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
    4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3,
    1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3,
    2.1213794301586595867e+4, 3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3,
    1.42343711074968357734, 4.63033784615654529590, 5.76949722146069140550, 3.64784832476320460504,
    1.27045825245236838258, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4,
    1.0, 2.05319162663775882187, 1.67638483018380384940, 6.89767334985100004550e-1,
    1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9,
    6.65790464350110377720, 5.46378491116411436990, 1.78482653991729133580, 2.96560571828504891230e-1,
    2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7,
    1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2,
    7.86869131145613259100e-4, 1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15};

// Every thread of the workgroup: the table into LDS (a barrier must follow before ns_ndtri reads it).
__device__ inline void ns_ndtri_load(double* tab_s) {
    for (int i = threadIdx.x; i < ALABI_NS_NDTRI_COEFS; i += blockDim.x) tab_s[i] = ns_ndtri_coef[i];
}

// Inverse of the standard normal CDF at 0 < p < 1; tab_s: the table in LDS.
__device__ __forceinline__ double ns_ndtri(const double* tab_s, double p) {
    const double q = p - 0.5;
    const bool centre = fabs(q) <= 0.425;
    double r = fma(-q, q, 0.180625);
    int base = 0;
    if (!centre) {
        r = sqrt(-log(q < 0.0 ? p : 1.0 - p));
        base = r <= 5.0 ? 16 : 32;
        r -= r <= 5.0 ? 1.6 : 5.0;
    }
    const double* c = tab_s + base;
    double num = c[7], den = c[15];
#pragma unroll
    for (int k = 6; k >= 0; --k) {
        num = fma(num, r, c[k]);
        den = fma(den, r, c[8 + k]);
    }
    const double v = num / den;
    return centre ? q * v : (q < 0.0 ? -v : v);
}

// Scaled coordinate (the prior transform, before the length scales) of cube coordinate k.
template <bool NORMAL>
__device__ __forceinline__ double ns_scaled_coord(const NsArgs& p, const double* tab_s, int k, double u) {
    double t = u;
    if (NORMAL && ((p.nmask >> k) & 1ull)) t = ns_ndtri(tab_s, u > 0.0 ? u : 0x1p-54);
    return fma(t, p.width.v[k], p.lo.v[k]);
}

// GP coordinate (scaled by the inverse length scales; centred for the squared exponential) of cube coordinate k.
template <bool GENERIC, bool NORMAL>
__device__ __forceinline__ double ns_gp_coord(const NsArgs& p, const double* tab_s, int k, double u) {
    double x = ns_scaled_coord<NORMAL>(p, tab_s, k, u) * p.inv_len.v[k];
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
// ---- the uniform-in-ellipsoids candidate (nested_unif.hip states the draw layout; nested_mlf.hip adds the neighbour test to it)
struct NsUnifArgs {
    const double* centres;       // [E, d]
    const double* axes;          // [E, d, d] lower triangular A
    const double* inv_axes;      // [E, d, d] lower triangular A^-1
    const double* cum;           // [E]
    double* cand_u;              // [M, d]
    double* cand_logl;           // [M]
    int* cand_status;            // [M]
    unsigned long long seed;
    long long call;
    int E, M, cand_id0, d;
};

#define ALABI_NS_UNIF_STEP 0x80000000u

// Candidate `cid` up to the thinning test.  Called by EVERY thread of the workgroup (blockDim.x a multiple of 64, at most 1024) with
// identical arguments; returns the workgroup-uniform status 0 / 1 / 2 and leaves the point in u_s[0 .. d).  z_s, u_s: d doubles of
// LDS each, cnt_s: 16 ints.  Three barriers on every path that reaches them; the caller may touch u_s / z_s / cnt_s again only in
// ways the next call's own barriers order (it reads u_s after the return, which follows the last barrier).
__device__ inline int ns_unif_candidate(const NsUnifArgs& q, uint32_t cid, double* z_s, double* u_s, int* cnt_s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6, d = q.d;
    if (tid < 64) ns_draw_normals(q.seed, q.call, cid, 0u, d, tid, z_s);
    uint32_t r[4];
    philox4x32_10((uint32_t)q.call, cid, ALABI_NS_UNIF_STEP, 0u, (uint32_t)q.seed, (uint32_t)(q.seed >> 32), r);
    const double v_ell = u53(r[0], r[1]), v_rad = u53(r[2], r[3]);
    philox4x32_10((uint32_t)q.call, cid, ALABI_NS_UNIF_STEP, 1u, (uint32_t)q.seed, (uint32_t)(q.seed >> 32), r);
    const double v_thin = u53(r[0], r[1]);
    int e = 0;
    while (e < q.E - 1 && !(v_ell < q.cum[e])) ++e;
    __syncthreads();
    double n2 = 0.0;
    for (int i = 0; i < d; ++i) n2 = fma(z_s[i], z_s[i], n2);
    const double s = pow(v_rad, 1.0 / (double)d) / sqrt(n2);
    int ok = 1;
    if (tid < d) {
        const double u = ns_prop_coord(q.axes + (size_t)e * d * d, d, z_s, tid, q.centres[(size_t)e * d + tid], s);
        ok = (u > 0.0) && (u < 1.0);
        u_s[tid] = u;
    }
    if (!__syncthreads_and(ok)) return 0;
    // wave w tests ellipsoids w, w + nw, ...: lane k forms row k of A^-1 (u - c), the squared norm is summed in row order
    int cnt = 0;
    for (int e2 = wave; e2 < q.E; e2 += nw) {
        if (e2 == e) continue;
        double y = 0.0;
        if (lane < d) {
            const double* R = q.inv_axes + ((size_t)e2 * d + lane) * d;
            const double* c = q.centres + (size_t)e2 * d;
            for (int i = 0; i <= lane; ++i) y = fma(R[i], u_s[i] - c[i], y);
        }
        double m = 0.0;
        for (int k = 0; k < d; ++k) {
            const double yk = __shfl(y, k, 64);
            m = fma(yk, yk, m);
        }
        cnt += (m <= 1.0) ? 1 : 0;
    }
    if (lane == 0) cnt_s[wave] = cnt;
    __syncthreads();
    int nq = 1;
    for (int w = 0; w < nw; ++w) nq += cnt_s[w];
    return (v_thin * (double)nq >= 1.0) ? 1 : 2;
}
}  // namespace alabi

static inline hipStream_t ns_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

#define NS_DISPATCH_FLAGS(TILED_, NORMAL_, ...)                                          \
    if (NORMAL_) { constexpr bool NORMAL = true;                                         \
        if (TILED_) { constexpr bool TILED = true; __VA_ARGS__; } else { constexpr bool TILED = false; __VA_ARGS__; } } \
    else { constexpr bool NORMAL = false;                                                \
        if (TILED_) { constexpr bool TILED = true; __VA_ARGS__; } else { constexpr bool TILED = false; __VA_ARGS__; } }

// Block size of the walk kernel: one training-point pair per lane when Npad / 2 <= 1024 (the register-resident path), 1024 lanes
// otherwise (pairs beyond them re-read from L2 each step).  Dimension buckets above 16 use at most 256 lanes, and their
// instantiations are compiled for 256 (ns_tmax) so that xa[D] gets the registers of a 256-lane block.
static constexpr int ns_tmax(int db) { return db <= 16 ? 1024 : 256; }
static inline int ns_threads(const alabi_gp* gp, int db) {
    const int half = gp->Npad / 2, cap = ns_tmax(db);
    int T = alabi::round_up(half, 64);
    if (T < 64) T = 64;
    return T < cap ? T : cap;
}

// The template arguments of one instantiation of the four templated kernels as a value that a generic lambda can take;
// NS_KERNEL(kernel, inst) names that instantiation of `kernel`.
template <int D_, bool GENERIC_, bool TILED_, bool NORMAL_>
struct NsInst { static constexpr int D = D_; static constexpr bool GENERIC = GENERIC_, TILED = TILED_, NORMAL = NORMAL_; };
#define NS_KERNEL(KERNEL, INST) \
    KERNEL<decltype(INST)::D, decltype(INST)::GENERIC, ns_tmax(decltype(INST)::D), decltype(INST)::TILED, decltype(INST)::NORMAL>

// Launches pick(inst)(args...) on `grid` workgroups: the instantiation and block size that fit this handle (dimension bucket, kernel
// family, register-resident or tiled training set, normal-prior mask); records the path in last_path.
template <class Pick, class... Args>
static int ns_dispatch(alabi_ns* ns, Pick pick, int grid, hipStream_t s, const Args&... args) {
    const alabi_gp* gp = ns->gp;
    const int db = alabi::dim_bucket(ns->d), T = ns_threads(gp, db);
    ns->last_path = (gp->Npad / 2 <= T) ? 1 : 2;
    const bool tiled = ns->last_path == 2;
    ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(gp->kf.type, NS_DISPATCH_FLAGS(tiled, ns->nmask != 0,
        hipLaunchKernelGGL(pick(NsInst<D, GENERIC, TILED, NORMAL>()), dim3(grid), dim3(T), 0, s, args...))));
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

// The NsArgs of a kernel that evaluates logL at single points (no walk): the GP's training set in the layout of its kernel family,
// the affine map of the log-probability and the prior transform.  ALABI_NOT_COMPUTED without a factorised GP with alpha.
static inline int ns_point_args(alabi_ns* ns, long long call, hipStream_t s, alabi::NsArgs& a) {
    alabi_gp* gp = ns->gp;
    if (!gp->computed || !gp->has_alpha) return ALABI_NOT_COMPUTED;
    const bool se = gp->kf.type == 0;
    if (se) { const int st = alabi::ens_se_prepare(gp, s); if (st != ALABI_OK) return st; }
    a.Xsrc = se ? gp->Xc : gp->Xt; a.Asrc = se ? gp->ens_h : gp->alpha; a.centre = gp->xa_centre;
    a.Npad = gp->Npad; a.kf = gp->kf;
    a.amp = ns->lp_scale * std::exp(gp->log_amp); a.mean = std::fma(ns->lp_scale, gp->mean, ns->lp_shift); a.ymap = ns->ymap;
    a.lo = ns->lo; a.width = ns->width; a.inv_len = gp->inv_len; a.nmask = ns->nmask;
    a.seed = ns->seed; a.call = call; a.d = ns->d;
    return ALABI_OK;
}

// alabi_ns_unif_draw and, after its own checks of the region, alabi_ns_mlf_draw.  geom: the 64-lane kernel of a host likelihood
// (evaluate = 0); pick(inst): the fused kernel; region: the move's further kernel arguments (none, or the NsMlfArgs).
template <class Geom, class Pick, class... Region>
static int ns_draw_launch(alabi_ns* ns, long long call, int cand_id0, int M, int evaluate, int E, const double* centres,
                          const double* axes, const double* inv_axes, const double* cum, double* cand_u, double* cand_logl,
                          int* cand_status, void* stream, Geom geom, Pick pick, const Region&... region) {
    using namespace alabi;
    if (!ns || M < 0 || cand_id0 < 0 || call < 0 || E < 1 || E > ALABI_NS_MAX_ELLIPSOIDS) return ALABI_BAD_ARGUMENT;
    if ((long long)cand_id0 + M > 0xFFFFFFFFLL) return ALABI_BAD_ARGUMENT;
    if (!centres || !axes || !inv_axes || !cum) return ALABI_BAD_ARGUMENT;
    if (M == 0) return ALABI_OK;
    if (!cand_u || !cand_logl || !cand_status) return ALABI_BAD_ARGUMENT;
    const hipStream_t s = ns_stream(stream);
    NsUnifArgs q{};
    q.centres = centres; q.axes = axes; q.inv_axes = inv_axes; q.cum = cum;
    q.cand_u = cand_u; q.cand_logl = cand_logl; q.cand_status = cand_status;
    q.seed = ns->seed; q.call = call; q.E = E; q.M = M; q.cand_id0 = cand_id0; q.d = ns->d;
    if (!evaluate) {
        hipLaunchKernelGGL(geom, dim3(M < 65536 ? M : 65536), dim3(64), 0, s, q, region...);
        ALABI_LAUNCH_CHECK();
        return ALABI_OK;
    }
    NsArgs a{};
    { const int st = ns_point_args(ns, call, s, a); if (st != ALABI_OK) return st; }
    // a workgroup keeps its training-set share for all its candidates: no more workgroups than the device holds at once needs
    return ns_dispatch(ns, pick, M < 1024 ? M : 1024, s, a, q, region...);
}
