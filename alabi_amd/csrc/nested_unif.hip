// Nested sampling on the GP surrogate for gfx950: uniform draws inside bounding ellipsoids (MultiNest's move; dynesty's
// sample="unif" with bound="single" / "multi"), the replacement step of the reference's run_pymultinest (alabi/core.py:2790-3238).
// The host fits the ellipsoids to the surviving live points once per iteration (alabi_amd/nested.py: bounding_ellipsoids) and
// keeps the nested-sampling loop; the device draws candidate points, tests them and evaluates the GP mean at the ones that pass.
//
// Ellipsoid e of E <= ALABI_NS_MAX_ELLIPSOIDS is {c_e + A_e z : |z| <= 1} with A_e lower triangular; the table holds the centres
// [E,d], the factors A [E,d,d] and their inverses [E,d,d] (row-major, lower triangles read) and the cumulative volume fractions
// cum [E] (cum[E-1] = 1).  It is a device array passed per call, like the Cholesky factor of the walks, and is read from L2 (global
// loads) in every dimension bucket: a candidate reads one factor and E - 1 inverses, E d (d + 1) / 2 doubles at most, spread over
// the lanes of the workgroup, against Npad d / 2 operands of one kernel sum; 2 E d^2 doubles fit the 64 KB of static LDS only for
// E d^2 <= 4096 (d <= 11 at E = 32), which would split the buckets <= 16 into two code paths.  (Unmeasured.)
//
// Candidate c (global id cand_id0 + index) of call `call`; everything below depends on (seed, call, c) only, never on M, the grid
// or how the candidates of a call are split over launches:
//   normals   z_2j, z_2j+1 = ns_normal_pair(seed, call, c, step = 0, j), j < ceil(d / 2)
//   uniforms  Philox counter (call, c, 0x80000000, 0): v_ell = u53(r0, r1), v_rad = u53(r2, r3); counter (call, c, 0x80000000, 1):
//             v_thin = u53(r0, r1); the key as everywhere (nested.hip, "Draws")
//   ellipsoid e = the first index with v_ell < cum[e]
//   point     rho = pow(v_rad, 1 / d), |z|^2 by an fma chain in coordinate order, s = rho / |z|,
//             u_k = ns_prop_coord(A_e, d, z, k, c_e[k], s) = c_e[k] + s sum_{i<=k} A_e[k][i] z_i        (uniform in ellipsoid e)
//   status 0  (outside) not all 0 < u_k < 1
//   status 1  (thinned) v_thin q >= 1, q = 1 + #{e' != e : |A_e'^-1 (u - c_e')|^2 <= 1}, the triangular product row by row and
//             the squared norm in row order, both fma chains: a point inside q ellipsoids is drawn q times as often, so keeping it
//             with probability 1 / q makes the draw uniform over the union
//   status 2  (evaluated) logL(u) by ns_gp_coord + ns_logl: the prior transform, normal-prior mask and y map of the walks
//
// Kernels
//   ns_unif_draw_kernel<D, GENERIC, TMAX, TILED, NORMAL>  flags and dispatch of ns_walk_kernel.  The workgroup's share of the training
//                               set is loaded once into VGPRs; the workgroup then handles candidates blockIdx.x, blockIdx.x +
//                               gridDim.x, ... of the launch's M, one ns_logl call per status-2 candidate.  Every branch is
//                               workgroup-uniform.  Writes cand_u [M,d], cand_logl [M] (-inf below status 2), cand_status [M].
//   ns_unif_geom_kernel         the same candidates up to the thinning test for a host likelihood (evaluate = 0): 64 lanes, no
//                               training set; status 2 leaves logL for the host to fill (-inf is written).
//   ns_unif_select_kernel       one workgroup, an ordered scan: the first `need` candidates with status 2 and logL > L*, in candidate
//                               order, to u_out / logl_out; counts[5] = taken, consumed (index after the last taken candidate when
//                               `need` were found, else M), and the evaluated / outside / thinned candidates among the consumed.
//                               Plain vector stores, no atomics: the order is the semantics.
// alabi_ns_unif_draw is ns_draw_launch (ns_device.hpp), the launch path it shares with alabi_ns_mlf_draw.
#include "ns_device.hpp"

namespace alabi {

// NsUnifArgs and ns_unif_candidate (the candidate up to the thinning test) live in ns_device.hpp: nested_mlf.hip draws the same ones.
template <int D, bool GENERIC, int TMAX, bool TILED, bool NORMAL>
__global__ void __launch_bounds__(TMAX)
ns_unif_draw_kernel(NsArgs p, NsUnifArgs q) {
    __shared__ double z_s[D], u_s[D], qs_s[D];
    __shared__ double scratch[16];
    __shared__ int cnt_s[16];
    __shared__ double nd_s[ALABI_NS_NDTRI_COEFS];            // NORMAL only (unused, so not allocated, otherwise)
    const int tid = threadIdx.x, d = q.d;
    // the training-set share of this lane: issued first, resident for every candidate of the workgroup
    const int half = p.Npad >> 1;
    const bool vA = tid < half;
    f64x2 xa[D];
#pragma unroll
    for (int k = 0; k < D; ++k)
        xa[k] = vA ? reinterpret_cast<const f64x2*>(p.Xsrc + (size_t)k * p.Npad)[tid] : f64x2{0.0, 0.0};
    const f64x2 aa = vA ? reinterpret_cast<const f64x2*>(p.Asrc)[tid] : (GENERIC ? f64x2{0.0, 0.0} : f64x2{ALABI_SE_PAD, ALABI_SE_PAD});
    if (NORMAL) ns_ndtri_load(nd_s);                         // the barriers of the first candidate order it before its first read
    for (long long c = blockIdx.x; c < q.M; c += gridDim.x) {
        const int st = ns_unif_candidate(q, (uint32_t)(q.cand_id0 + c), z_s, u_s, cnt_s);
        if (tid < d) q.cand_u[(size_t)c * d + tid] = u_s[tid];
        double lp = -INFINITY;
        if (st == 2) {                                       // workgroup-uniform
            if (tid < D) qs_s[tid] = tid < d ? ns_gp_coord<GENERIC, NORMAL>(p, nd_s, tid, u_s[tid]) : 0.0;
            __syncthreads();
            lp = ns_logl<D, GENERIC, TILED>(p, xa, aa, qs_s, scratch);
        }
        if (tid == 0) { q.cand_logl[c] = lp; q.cand_status[c] = st; }
    }
}

__global__ void __launch_bounds__(64)
ns_unif_geom_kernel(NsUnifArgs q) {
    __shared__ double z_s[ALABI_MAX_DIM], u_s[ALABI_MAX_DIM];
    __shared__ int cnt_s[16];
    const int tid = threadIdx.x, d = q.d;
    for (long long c = blockIdx.x; c < q.M; c += gridDim.x) {
        const int st = ns_unif_candidate(q, (uint32_t)(q.cand_id0 + c), z_s, u_s, cnt_s);
        if (tid < d) q.cand_u[(size_t)c * d + tid] = u_s[tid];
        if (tid == 0) { q.cand_logl[c] = -INFINITY; q.cand_status[c] = st; }
    }
}

#define ALABI_NS_SELECT_T 256

__global__ void __launch_bounds__(ALABI_NS_SELECT_T)
ns_unif_select_kernel(int M, int d, const double* __restrict__ cand_u, const double* __restrict__ cand_logl,
                      const int* __restrict__ cand_status, double logl_star, int need, double* __restrict__ u_out,
                      double* __restrict__ logl_out, int* __restrict__ counts) {
    constexpr int T = ALABI_NS_SELECT_T;
    __shared__ int scan_s[T];
    __shared__ int red_s[3][T];
    __shared__ int taken_s, consumed_s;
    const int tid = threadIdx.x;
    if (tid == 0) { taken_s = 0; consumed_s = need > 0 ? M : 0; }
    __syncthreads();
    // ordered scan, T candidates at a time: the rank of a passing candidate = passing candidates in front of it
    for (int base = 0; need > 0 && base < M; base += T) {
        const int taken = taken_s;                           // written after the last barrier of the previous round
        if (taken >= need) break;                            // workgroup-uniform
        const int i = base + tid;
        const int pass = (i < M && cand_status[i] == 2 && cand_logl[i] > logl_star) ? 1 : 0;     // false for NaN
        scan_s[tid] = pass;
        __syncthreads();
        for (int off = 1; off < T; off <<= 1) {
            const int v = tid >= off ? scan_s[tid - off] : 0;
            __syncthreads();
            scan_s[tid] += v;
            __syncthreads();
        }
        const int rank = taken + scan_s[tid] - pass;
        if (pass && rank < need) {
            for (int k = 0; k < d; ++k) u_out[(size_t)rank * d + k] = cand_u[(size_t)i * d + k];
            logl_out[rank] = cand_logl[i];
            if (rank == need - 1) consumed_s = i + 1;        // one thread at most
        }
        const int total = scan_s[T - 1];
        __syncthreads();
        if (tid == 0) taken_s = (taken + total < need) ? taken + total : need;
        __syncthreads();
    }
    const int consumed = consumed_s;
    int n2 = 0, n0 = 0, n1 = 0;
    for (int i = tid; i < consumed; i += T) {
        const int st = cand_status[i];
        n2 += st == 2; n0 += st == 0; n1 += st == 1;
    }
    red_s[0][tid] = n2; red_s[1][tid] = n0; red_s[2][tid] = n1;
    __syncthreads();
    for (int off = T >> 1; off > 0; off >>= 1) {
        if (tid < off) {
            red_s[0][tid] += red_s[0][tid + off]; red_s[1][tid] += red_s[1][tid + off]; red_s[2][tid] += red_s[2][tid + off];
        }
        __syncthreads();
    }
    if (tid < 5) {
        const int v = tid == 0 ? taken_s : tid == 1 ? consumed : red_s[tid - 2][0];
        counts[tid] = v;
    }
}

}  // namespace alabi

using namespace alabi;

extern "C" {

int alabi_ns_unif_draw(alabi_ns* ns, long long call, int cand_id0, int M, int evaluate, int E, const double* centres,
                       const double* axes, const double* inv_axes, const double* cum, double* cand_u, double* cand_logl,
                       int* cand_status, void* stream) {
    return ns_draw_launch(ns, call, cand_id0, M, evaluate, E, centres, axes, inv_axes, cum, cand_u, cand_logl, cand_status, stream,
                          ns_unif_geom_kernel, [](auto inst) { return NS_KERNEL(ns_unif_draw_kernel, inst); });
}

int alabi_ns_unif_select(alabi_ns* ns, int M, const double* cand_u, const double* cand_logl, const int* cand_status,
                         double logl_star, int need, double* u_out, double* logl_out, int* counts, void* stream) {
    if (!ns || M < 0 || need < 0 || std::isnan(logl_star) || !counts) return ALABI_BAD_ARGUMENT;
    if (M > 0 && (!cand_u || !cand_logl || !cand_status)) return ALABI_BAD_ARGUMENT;
    if (need > 0 && M > 0 && (!u_out || !logl_out)) return ALABI_BAD_ARGUMENT;
    hipLaunchKernelGGL(ns_unif_select_kernel, dim3(1), dim3(ALABI_NS_SELECT_T), 0, ns_stream(stream), M, ns->d, cand_u, cand_logl,
                       cand_status, logl_star, need, u_out, logl_out, counts);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // extern "C"
