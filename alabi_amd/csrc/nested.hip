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
// Normal priors (alabi_ns_set_normal_prior; the reference's prior_transform_normal, alabi/utility.py:381-482): on the coordinates
// of a 64-bit mask the cube maps through the inverse normal CDF instead, x = mean + std * ndtri(u), NOT truncated to the box, as
// in the reference.  The host stores mean in lo and std in width (std may be negative, as width may), so ns_scaled_coord is
//   x = fma(t, width, lo),   t = u (uniform coordinate) or ndtri(u), with ndtri(2^-54) at u = 0 (normal coordinate).
// The clamp: u53 returns exactly 0 with probability 2^-53, ndtri(0) = -inf, and the centred squared-exponential form turns
// x = -inf into NaN; 2^-54 maps to -8.37 std.  Every other value of u53 is >= 2^-53, so for drawn points this is
// ndtri(max(u, 2^-54)); a positive u below 2^-54 (only a proposal of a walk can land there) keeps its own finite ndtri (-37 std
// at 1e-300), which AS 241 gives to full accuracy.  u < 1 always holds (u53 < 1, and the walks keep 0 < u < 1).  The prior enters
// nested sampling through this map alone: no Jacobian term.  Kernels with a non-empty mask are instantiations of their own
// (template flag NORMAL); with an empty mask the instantiations and every result are those of the uniform-only code.
// ndtri is Wichura's AS 241 (PPND16, Appl. Statist. 37 (1988) 477-484) in fp64 (ns_ndtri): three rational approximations of
// degree 7 / 7, one Horner pair whose 16 coefficients each lane reads from a 48-entry table in LDS (ns_ndtri_coef, copied
// there at the start of the kernel).  Literal coefficients -- HIP's normcdfinv has about 180 of them -- are hoisted out of the
// step loop as loop invariants and then spilled: +1.4 KB of scratch per lane in every instantiation; LDS reads are not hoisted.
//
// Kernels
//   ns_walk_kernel<D, GENERIC, TMAX, TILED, NORMAL>  one workgroup per walk; all `walks` Metropolis steps inside one launch (walks never talk to
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
//   ns_slice_kernel<D, GENERIC, TMAX, TILED, NORMAL>  random-direction slice sampling (dynesty's "rslice"), one workgroup per walk, all slices
//                               of the walk in one launch, the training-set share in VGPRs as above.  The slice is a state machine
//                               (ns_slice_advance: direction, stepping out, shrinking; its scalars live in LDS) advanced by wave 0
//                               from one in-cube query to the next; the loop around it holds the single ns_logl call site.
//   ns_slice_step_kernel        the same state machine driven one query at a time around a host likelihood: per-walk state in
//                               device memory, consumes the host's logL of the pending query, advances to the next one.
//   ns_prior_kernel             uniform points in the cube.
//   ns_transform_kernel         cube points -> scaled coordinates by ns_scaled_coord, the map the walks use (alabi_ns_transform).
//   ns_propose_kernel           the proposal of one step of every walk (host-callable likelihoods): the same draws and the same
//                               arithmetic as the fused walk (shared functions below), so both paths move identically.
//   ns_accept_kernel            the accept test of one step, given the host's logL of the proposals.
// alabi_ns_walk and alabi_ns_slice check their own arguments and share ns_walk_launch (below); ns_dispatch, ns_point_args and the
// ns_load_chol of the one-wave kernels are in ns_device.hpp.
//
// Draws.  Everything is keyed by (seed, call, global walk id, step): counter (c0, c1, c2, c3) = ((uint32) call, walk id, step,
// j), key = (low, high 32 bits of seed).  Normals: pair j (coordinates 2j, 2j+1) from one Philox block r[0..3]:
//   u1 = u53(r0, r1), u2 = u53(r2, r3), rad = sqrt(-2 log(1 - u1)), z_2j = rad cos(2 pi u2), z_2j+1 = rad sin(2 pi u2).
// Prior draws use step = 0xFFFFFFFF: coordinate 2j = u53(r0, r1), 2j+1 = u53(r2, r3).  Splitting the walks of one call into
// several launches (walk_id0 offsets) therefore gives bit-identical results.
// Slice move (ns_slice_kernel / ns_slice_step_kernel): slice s of a walk takes its direction normals from step = s as above, and its
// uniforms from counter (call, walk id, 0x80000000 | s, m), value u53(r0, r1): m = 0 the interval offset r, m >= 1 the m-th shrink
// draw.  s < 2^31 - 1 keeps these apart from the prior draws.
// Ellipsoid move (nested_unif.hip): the second counter word is the candidate id instead of a walk id; candidate c takes its normals
// from step = 0 as above and its uniforms from counter (call, c, 0x80000000, m): m = 0 gives v_ell = u53(r0, r1) and v_rad =
// u53(r2, r3), m = 1 gives v_thin = u53(r0, r1).  A call is one move, so these never meet the walk or slice draws of the same key.
#include <new>
#include "ns_device.hpp"

namespace alabi {

// ---------------------------------------------------------------------------------------------------------------- slice move
#define ALABI_NS_SLICE_CAP 64            // contractions after which a slice ends where it started (termination guard)
enum { NS_INIT = 0, NS_LEFT = 1, NS_RIGHT = 2, NS_SHRINK = 3, NS_DONE = 4 };

// Scalars of one walk.  In the split path they are followed in device memory by u[d], a[d], q[d] (ns_slice_stride).
struct NsSliceState {
    double tl, tr, t, L;                 // interval ends and the coordinate of the pending query along the axis; logL of the walk
    int phase, s, m, ncs;                // ncs: contractions of slice s so far
    int nev, nexp, ncon, ncap;           // evaluations, expansions, contractions, capped slices of the walk
    int pending, pad;                    // a query (point q, coordinate t) waits for its logL
};

__host__ __device__ inline size_t ns_slice_stride(int d) { return sizeof(NsSliceState) + (size_t)3 * d * sizeof(double); }

__device__ inline double ns_slice_uniform(unsigned long long seed, long long call, uint32_t wid, int s, int m) {
    uint32_t r[4];
    philox4x32_10((uint32_t)call, wid, 0x80000000u | (uint32_t)s, (uint32_t)m, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    return u53(r[0], r[1]);
}

// Advances one walk from its state to its next query strictly inside the cube (returns 1; the point is in q_s, its logL is to be
// handed in as `lp` by the next call) or to its end (returns 0).  Called by all 64 lanes of ONE wave with identical scalar
// arguments: the scalars of the state are read into registers, carried wave-uniformly and written back by lane 0; lane k < d owns
// coordinate k of the position u_s, the axis a_s and the query q_s, so no lane reads what another one wrote in this call.  No
// barrier inside.  C: lower-triangular factor, row stride ldc, zero above the diagonal.
__device__ __forceinline__ int ns_slice_advance(NsSliceState* st, double* u_s, double* a_s, double* q_s, const double* C, int ldc,
                                       unsigned long long seed, long long call, uint32_t wid, int d, int slices, double scale,
                                       double lstar, int lane, double lp) {
    double tl = st->tl, tr = st->tr, t = st->t, L = st->L;
    int phase = st->phase, s = st->s, m = st->m, ncs = st->ncs;
    int nev = st->nev, nexp = st->nexp, ncon = st->ncon, ncap = st->ncap;
    bool have = st->pending != 0;
    const bool mine = lane < d;
    double u = mine ? u_s[lane] : 0.5, a = mine ? a_s[lane] : 0.0, q = mine ? q_s[lane] : 0.5;
    int query = 0;
    while (phase != NS_DONE) {
        bool contract = false;
        if (have) {                                          // the logL of the point at t
            have = false;
            nev += 1;
            const bool above = lp > lstar;                   // false for NaN
            if (phase == NS_LEFT) {
                if (above) { tl -= 1.0; nexp += 1; } else phase = NS_RIGHT;
            } else if (phase == NS_RIGHT) {
                if (above) { tr += 1.0; nexp += 1; } else phase = NS_SHRINK;
            } else if (above) {
                u = q; L = lp; s += 1; phase = NS_INIT;
            } else {
                contract = true;
            }
        }
        if (contract) {
            if (t < 0.0) tl = t; else tr = t;
            ncon += 1; ncs += 1;
        }
        if (phase == NS_INIT) {
            if (s >= slices) { phase = NS_DONE; break; }
            // axis a = scale C z / |z|: pair j of the normals is drawn by lane j and read by every lane through the cross-lane network
            double z0 = 0.0, z1 = 0.0;
            if (2 * lane < d) ns_normal_pair(seed, call, wid, (uint32_t)s, (uint32_t)lane, z0, z1);
            double acc = 0.0, n2 = 0.0;
            for (int i = 0; i < d; ++i) {
                const double zi = __shfl((i & 1) ? z1 : z0, i >> 1, 64);
                n2 = fma(zi, zi, n2);
                if (mine && i <= lane) acc = fma(C[(size_t)lane * ldc + i], zi, acc);
            }
            a = (scale * acc) / sqrt(n2);
            const double r = ns_slice_uniform(seed, call, wid, s, 0);
            tl = -r; tr = 1.0 - r; m = 1; ncs = 0; phase = NS_LEFT;
        }
        if (phase == NS_SHRINK) {
            if (ncs >= ALABI_NS_SLICE_CAP) { ncap += 1; s += 1; phase = NS_INIT; continue; }
            const double w = tr - tl;
            t = tl + ns_slice_uniform(seed, call, wid, s, m) * w;
            m += 1;
        } else {
            t = phase == NS_LEFT ? tl : tr;
        }
        q = u + t * a;
        if (__all(!mine || (q > 0.0 && q < 1.0))) { query = 1; break; }
        // outside the cube: the stepping on this side ends / one contraction, without an evaluation
        if (phase == NS_LEFT) phase = NS_RIGHT;
        else if (phase == NS_RIGHT) phase = NS_SHRINK;
        else { if (t < 0.0) tl = t; else tr = t; ncon += 1; ncs += 1; }
    }
    if (mine) { u_s[lane] = u; a_s[lane] = a; q_s[lane] = q; }
    if (lane == 0) {
        st->tl = tl; st->tr = tr; st->t = t; st->L = L;
        st->phase = phase; st->s = s; st->m = m; st->ncs = ncs;
        st->nev = nev; st->nexp = nexp; st->ncon = ncon; st->ncap = ncap;
        st->pending = query;
    }
    return query;
}

__device__ inline void ns_slice_reset(NsSliceState* st, double logl) {
    st->tl = 0.0; st->tr = 0.0; st->t = 0.0; st->L = logl;
    st->phase = NS_INIT; st->s = 0; st->m = 0; st->ncs = 0;
    st->nev = 0; st->nexp = 0; st->ncon = 0; st->ncap = 0;
    st->pending = 0; st->pad = 0;
}

// NsArgs as the walk kernel; p.walks = slices, p.n_acc = counts [4K]: evaluations, expansions, contractions, capped slices.
template <int D, bool GENERIC, int TMAX, bool TILED, bool NORMAL>
__global__ void __launch_bounds__(TMAX)
ns_slice_kernel(NsArgs p) {
    __shared__ double C_s[D * D];
    __shared__ double u_s[D], a_s[D], q_s[D], qs_s[D];
    __shared__ double scratch[16];
    __shared__ NsSliceState st_s;
    __shared__ int go_s;
    __shared__ double nd_s[ALABI_NS_NDTRI_COEFS];            // NORMAL only (unused, so not allocated, otherwise)
    const int tid = threadIdx.x, T = blockDim.x, b = blockIdx.x, d = p.d;
    const uint32_t wid = (uint32_t)(p.walk_id0 + b);
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
        u_s[tid] = tid < d ? p.u0[(size_t)b * d + tid] : 0.0;
        a_s[tid] = 0.0; q_s[tid] = 0.0; qs_s[tid] = 0.0;
    }
    if (tid == 0) ns_slice_reset(&st_s, p.logl0[b]);
    if (NORMAL) ns_ndtri_load(nd_s);
    __syncthreads();
    double lp = 0.0;
    for (;;) {
        if (tid < 64) {
            const int query = ns_slice_advance(&st_s, u_s, a_s, q_s, C_s, D, p.seed, p.call, wid, d, p.walks, p.scale, p.logl_star,
                                               tid, lp);
            if (tid < d) qs_s[tid] = ns_gp_coord<GENERIC, NORMAL>(p, nd_s, tid, q_s[tid]);
            if (tid == 0) go_s = query;
        }
        __syncthreads();
        if (!go_s) break;                                    // workgroup-uniform
        // wave 0 writes go_s / qs_s / scratch again only after the barrier inside ns_logl, which every wave passes after reading them
        lp = ns_logl<D, GENERIC, TILED>(p, xa, aa, qs_s, scratch);
    }
    if (tid < d) p.u_out[(size_t)b * d + tid] = u_s[tid];
    if (tid == 0) {
        p.logl_out[b] = st_s.L;
        if (p.n_acc) {
            p.n_acc[b] = st_s.nev; p.n_acc[p.K + b] = st_s.nexp; p.n_acc[2 * p.K + b] = st_s.ncon; p.n_acc[3 * p.K + b] = st_s.ncap;
        }
    }
}

__global__ void __launch_bounds__(256)
ns_slice_begin_kernel(int K, int d, const double* __restrict__ u0, const double* __restrict__ logl0, char* __restrict__ state) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= K) return;
    char* base = state + (size_t)b * ns_slice_stride(d);
    ns_slice_reset(reinterpret_cast<NsSliceState*>(base), logl0[b]);
    double* v = reinterpret_cast<double*>(base + sizeof(NsSliceState));
    for (int k = 0; k < d; ++k) { v[k] = u0[(size_t)b * d + k]; v[d + k] = 0.0; v[2 * d + k] = 0.0; }
}

// One 64-lane workgroup (one wave) per walk: state in, ns_slice_advance, state out, the next query and whether there is one.
__global__ void __launch_bounds__(64)
ns_slice_step_kernel(unsigned long long seed, long long call, int walk_id0, int d, int slices, const double* __restrict__ chol,
                     double scale, double logl_star, char* __restrict__ state, const double* __restrict__ logl_query,
                     double* __restrict__ u_query, int* __restrict__ active) {
    __shared__ double C_s[ALABI_MAX_DIM * ALABI_MAX_DIM];
    __shared__ double u_s[ALABI_MAX_DIM], a_s[ALABI_MAX_DIM], q_s[ALABI_MAX_DIM];
    __shared__ NsSliceState st_s;
    const int tid = threadIdx.x, b = blockIdx.x;
    char* base = state + (size_t)b * ns_slice_stride(d);
    NsSliceState* g = reinterpret_cast<NsSliceState*>(base);
    double* v = reinterpret_cast<double*>(base + sizeof(NsSliceState));
    ns_load_chol(C_s, ALABI_MAX_DIM, chol, d);
    if (tid < d) { u_s[tid] = v[tid]; a_s[tid] = v[d + tid]; q_s[tid] = v[2 * d + tid]; }
    if (tid == 0) st_s = *g;
    __syncthreads();
    const double lp = st_s.pending ? logl_query[b] : 0.0;
    const int query = ns_slice_advance(&st_s, u_s, a_s, q_s, C_s, ALABI_MAX_DIM, seed, call, (uint32_t)(walk_id0 + b), d, slices, scale,
                                       logl_star, tid, lp);
    __syncthreads();
    if (tid < d) { v[tid] = u_s[tid]; v[d + tid] = a_s[tid]; v[2 * d + tid] = q_s[tid]; u_query[(size_t)b * d + tid] = q_s[tid]; }
    if (tid == 0) { *g = st_s; active[b] = query; }
}

__global__ void __launch_bounds__(256)
ns_slice_end_kernel(int K, int d, const char* __restrict__ state, double* __restrict__ u_out, double* __restrict__ logl_out,
                    int* __restrict__ counts) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= K) return;
    const char* base = state + (size_t)b * ns_slice_stride(d);
    const NsSliceState* st = reinterpret_cast<const NsSliceState*>(base);
    const double* v = reinterpret_cast<const double*>(base + sizeof(NsSliceState));
    for (int k = 0; k < d; ++k) u_out[(size_t)b * d + k] = v[k];
    logl_out[b] = st->L;
    if (counts) { counts[b] = st->nev; counts[K + b] = st->nexp; counts[2 * K + b] = st->ncon; counts[3 * K + b] = st->ncap; }
}

// TMAX: 1024 lanes for dimension buckets <= 16, 256 above (the register budget of xa[D] and the query), see ns_threads.
template <int D, bool GENERIC, int TMAX, bool TILED, bool NORMAL>
__global__ void __launch_bounds__(TMAX)
ns_walk_kernel(NsArgs p) {
    __shared__ double C_s[D * D];
    __shared__ double u_s[D], up_s[D], qs_s[D], z_s[D];
    __shared__ double scratch[16];
    __shared__ double L_s;
    __shared__ int acc_s, nev_s;
    __shared__ double nd_s[ALABI_NS_NDTRI_COEFS];            // NORMAL only (unused, so not allocated, otherwise)
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
    if (NORMAL) { ns_ndtri_load(nd_s); __syncthreads(); }
    if (tid < D) {
        const double u = tid < d ? p.u0[(size_t)b * d + tid] : 0.0;
        u_s[tid] = u;
        z_s[tid] = 0.0;
        qs_s[tid] = tid < d ? ns_gp_coord<GENERIC, NORMAL>(p, nd_s, tid, u) : 0.0;
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
                qs_s[tid] = ns_gp_coord<GENERIC, NORMAL>(p, nd_s, tid, up);
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

// p.u0 [K, d] cube points -> p.u_out [K, d] scaled coordinates; four points per workgroup, one per wave, lane k = coordinate k.
__global__ void __launch_bounds__(256)
ns_transform_kernel(NsArgs p) {
    __shared__ double nd_s[ALABI_NS_NDTRI_COEFS];
    ns_ndtri_load(nd_s);
    __syncthreads();
    const int k = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= p.K || k >= p.d) return;
    p.u_out[(size_t)b * p.d + k] = ns_scaled_coord<true>(p, nd_s, k, p.u0[(size_t)b * p.d + k]);
}

// One 64-lane workgroup per walk: the normals and the proposal exactly as ns_walk_kernel forms them.
__global__ void __launch_bounds__(64)
ns_propose_kernel(unsigned long long seed, long long call, int walk_id0, int d, int step, const double* __restrict__ chol,
                  double scale, const double* __restrict__ u_cur, double* __restrict__ u_prop) {
    __shared__ double C_s[ALABI_MAX_DIM * ALABI_MAX_DIM];
    __shared__ double z_s[ALABI_MAX_DIM];
    const int tid = threadIdx.x, b = blockIdx.x;
    ns_load_chol(C_s, ALABI_MAX_DIM, chol, d);
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

// The launch of alabi_ns_walk and alabi_ns_slice after their argument checks: K workgroups of the kernel pick(inst).  walks: steps
// or slices (NsArgs::walks and n_acc serve both kernels).
template <class Pick>
static int ns_walk_launch(alabi_ns* ns, long long call, int walk_id0, const double* u0, const double* logl0, int K, double logl_star,
                          const double* chol, double scale, int walks, double* u_out, double* logl_out, int* n_acc, void* stream,
                          Pick pick) {
    const hipStream_t s = ns_stream(stream);
    NsArgs a{};
    { const int st = ns_point_args(ns, call, s, a); if (st != ALABI_OK) return st; }
    a.u0 = u0; a.logl0 = logl0; a.chol = chol; a.u_out = u_out; a.logl_out = logl_out; a.n_acc = n_acc;
    a.walk_id0 = walk_id0; a.K = K; a.walks = walks; a.logl_star = logl_star; a.scale = scale;
    return ns_dispatch(ns, pick, K, s, a);
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
    n->box_lo = n->lo; n->box_width = n->width;
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

int alabi_ns_set_normal_prior(alabi_ns* ns, const double* mean, const double* std) {
    if (!ns || !mean || !std) return ALABI_BAD_ARGUMENT;
    for (int k = 0; k < ns->d; ++k)
        if (std::isfinite(mean[k]) && (!std::isfinite(std[k]) || std[k] == 0.0)) return ALABI_BAD_ARGUMENT;
    ns->nmask = 0;
    for (int k = 0; k < ns->d; ++k) {
        const bool normal = std::isfinite(mean[k]);
        ns->lo.v[k] = normal ? mean[k] : ns->box_lo.v[k];
        ns->width.v[k] = normal ? std[k] : ns->box_width.v[k];
        if (normal) ns->nmask |= 1ull << k;
    }
    return ALABI_OK;
}

int alabi_ns_transform(alabi_ns* ns, const double* u, int K, double* x_out, void* stream) {
    if (!ns || K < 0) return ALABI_BAD_ARGUMENT;
    if (K == 0) return ALABI_OK;
    if (!u || !x_out) return ALABI_BAD_ARGUMENT;
    NsArgs a{};
    a.lo = ns->lo; a.width = ns->width; a.nmask = ns->nmask;
    a.u0 = u; a.u_out = x_out; a.K = K; a.d = ns->d;
    hipLaunchKernelGGL(ns_transform_kernel, dim3((unsigned)(((long long)K + 3) / 4)), dim3(256), 0, ns_stream(stream), a);
    ALABI_LAUNCH_CHECK();
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
    return ns_walk_launch(ns, call, walk_id0, u0, logl0, K, logl_star, chol, scale, walks, u_out, logl_out, n_accept, stream,
                          [](auto inst) { return NS_KERNEL(ns_walk_kernel, inst); });
}

int alabi_ns_slice(alabi_ns* ns, long long call, int walk_id0, const double* u0, const double* logl0, int K, double logl_star,
                   const double* chol, double scale, int slices, double* u_out, double* logl_out, int* counts, void* stream) {
    if (!ns || K < 0 || slices < 0 || slices >= 0x7FFFFFFF || walk_id0 < 0 || call < 0 || std::isnan(logl_star)) return ALABI_BAD_ARGUMENT;
    if ((long long)walk_id0 + K > 0xFFFFFFFFLL) return ALABI_BAD_ARGUMENT;
    if (K == 0) return ALABI_OK;
    if (!u0 || !logl0 || !u_out || !logl_out || (slices > 0 && (!chol || !(scale > 0.0) || !std::isfinite(scale)))) return ALABI_BAD_ARGUMENT;
    return ns_walk_launch(ns, call, walk_id0, u0, logl0, K, logl_star, chol, scale, slices, u_out, logl_out, counts, stream,
                          [](auto inst) { return NS_KERNEL(ns_slice_kernel, inst); });
}

int alabi_ns_slice_state_bytes(alabi_ns* ns, int K, long long* bytes) {
    if (!ns || !bytes || K < 0) return ALABI_BAD_ARGUMENT;
    *bytes = (long long)K * (long long)ns_slice_stride(ns->d);
    return ALABI_OK;
}

int alabi_ns_slice_begin(alabi_ns* ns, const double* u0, const double* logl0, int K, void* state, void* stream) {
    if (!ns || K < 0) return ALABI_BAD_ARGUMENT;
    if (K == 0) return ALABI_OK;
    if (!u0 || !logl0 || !state) return ALABI_BAD_ARGUMENT;
    hipLaunchKernelGGL(ns_slice_begin_kernel, dim3((K + 255) / 256), dim3(256), 0, ns_stream(stream), K, ns->d, u0, logl0,
                       static_cast<char*>(state));
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int alabi_ns_slice_step(alabi_ns* ns, long long call, int walk_id0, int K, double logl_star, const double* chol, double scale,
                        int slices, void* state, const double* logl_query, double* u_query, int* active, void* stream) {
    if (!ns || K < 0 || slices < 0 || slices >= 0x7FFFFFFF || walk_id0 < 0 || call < 0 || std::isnan(logl_star)) return ALABI_BAD_ARGUMENT;
    if ((long long)walk_id0 + K > 0xFFFFFFFFLL) return ALABI_BAD_ARGUMENT;
    if (K == 0) return ALABI_OK;
    if (!state || !logl_query || !u_query || !active || !chol || !(scale > 0.0) || !std::isfinite(scale)) return ALABI_BAD_ARGUMENT;
    hipLaunchKernelGGL(ns_slice_step_kernel, dim3(K), dim3(64), 0, ns_stream(stream), ns->seed, call, walk_id0, ns->d, slices, chol,
                       scale, logl_star, static_cast<char*>(state), logl_query, u_query, active);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int alabi_ns_slice_end(alabi_ns* ns, int K, const void* state, double* u_out, double* logl_out, int* counts, void* stream) {
    if (!ns || K < 0) return ALABI_BAD_ARGUMENT;
    if (K == 0) return ALABI_OK;
    if (!state || !u_out || !logl_out) return ALABI_BAD_ARGUMENT;
    hipLaunchKernelGGL(ns_slice_end_kernel, dim3((K + 255) / 256), dim3(256), 0, ns_stream(stream), K, ns->d,
                       static_cast<const char*>(state), u_out, logl_out, counts);
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
