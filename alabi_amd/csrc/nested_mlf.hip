// Nested sampling on the GP surrogate for gfx950: the MLFriends region (UltraNest's bound; Buchner 2016, 2019) over the ellipsoid
// bounds of nested_unif.hip, the replacement step of the reference's run_ultranest (alabi/core.py:3241-3690).  A candidate drawn
// uniformly in the union of the ellipsoids counts only if it lies within a radius r of some live point, in the metric whitened by
// the live points' covariance: a union of small balls follows a curved contour that a union of ellipsoids cannot.  The host
// (alabi_amd/nested.py: mlfriends_metric) fits the ellipsoids, forms the metric L^-1 (lower triangular) and the whitened live points
// w_i = L^-1 p_i [n,d]; the device finds r^2 by bootstrapping and applies the neighbour test to the candidates.
//
// Radius.  Round b < B of call `call` draws n indices idx_k = min(floor(v_k n), n - 1), v_k = u53(r0, r1) of Philox counter
// (call, b, 0x80000001, k), the key as everywhere (nested.hip, "Draws"); selected = the set of drawn indices;
//   r2_b = max over unselected i of min over selected j of |w_i - w_j|^2     (0 when nothing is left out)
// the squared distance an fma chain in coordinate order.  The host takes r^2 = max_b r2_b.  max and min do not depend on the order,
// so r2_b is a function of (seed, call, b, w) alone.
//
// Candidate c: exactly the candidate of nested_unif.hip (ns_unif_candidate: the same keys, ellipsoid choice, cube test and 1 / q
// thinning), and for one that would have status 2
//   w_c = metric_inv u: lane k forms row k, an fma chain over i <= k
//   status 2 iff some j < n has |w_c - w_j|^2 <= r2 (fma chain in coordinate order), else status 1
// so status 1 means "thinned, or no live point within r".  r2 = +inf keeps every status of alabi_ns_unif_draw; r2 = 0 keeps exact
// hits only.  ns_unif_select_kernel takes the candidates as before.
//
// Kernels (ordinary grids, workgroup-uniform barriers, no hand-off between workgroups, no atomics on global memory)
//   ns_mlf_radius_kernel        one workgroup per round.  The selection is a bit mask of n <= ALABI_NS_MLF_MAX_POINTS bits in LDS, set
//                               by LDS atomic ORs; lane t takes the unselected i = t, t + T, ... and runs over the selected j (j is
//                               workgroup-uniform, so row j is one broadcast read); max over the workgroup through LDS.  w is read
//                               from L2: n d doubles, 32 KB at n = 400, d = 10.  (Unmeasured against a [d, npad] copy.)
//   ns_mlf_draw_kernel<D, GENERIC, TMAX, TILED, NORMAL>  ns_unif_draw_kernel with the neighbour test between the candidate and its
//                               logL: threads j = tid, tid + T, ... each form one squared distance, __syncthreads_or decides.  The
//                               test costs n d fused multiply-adds per surviving candidate and saves the N d of a GP mean for each
//                               one it rejects.
//   ns_mlf_geom_kernel          the same up to the neighbour test for a host likelihood (evaluate = 0): 64 lanes, no training set.
// alabi_ns_mlf_draw checks the region's arguments and then takes the launch path of alabi_ns_unif_draw (ns_draw_launch, ns_device.hpp).
#include "ns_device.hpp"

namespace alabi {

struct NsMlfArgs {
    const double* w;             // [n, d] whitened live points
    const double* metric_inv;    // [d, d] lower triangular L^-1
    double r2;
    int n;
};

#define ALABI_NS_MLF_STEP 0x80000001u
#define ALABI_NS_MLF_RADIUS_T 256

// |a - b|^2 over d coordinates, an fma chain in coordinate order.
__device__ __forceinline__ double ns_mlf_dist2(const double* a, const double* b, int d) {
    double s = 0.0;
    for (int k = 0; k < d; ++k) {
        const double t = a[k] - b[k];
        s = fma(t, t, s);
    }
    return s;
}

__global__ void __launch_bounds__(ALABI_NS_MLF_RADIUS_T)
ns_mlf_radius_kernel(unsigned long long seed, long long call, int n, int d, const double* __restrict__ w,
                     double* __restrict__ r2_out) {
    constexpr int T = ALABI_NS_MLF_RADIUS_T;
    __shared__ unsigned int sel_s[ALABI_NS_MLF_MAX_POINTS / 32];
    __shared__ double red_s[T];
    const int tid = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const int words = (n + 31) >> 5;
    for (int i = tid; i < words; i += T) sel_s[i] = 0u;
    __syncthreads();
    for (int k = tid; k < n; k += T) {
        uint32_t r[4];
        philox4x32_10((uint32_t)call, b, ALABI_NS_MLF_STEP, (uint32_t)k, (uint32_t)seed, (uint32_t)(seed >> 32), r);
        int idx = (int)(u53(r[0], r[1]) * (double)n);
        idx = idx < n - 1 ? idx : n - 1;
        atomicOr(&sel_s[idx >> 5], 1u << (idx & 31));
    }
    __syncthreads();
    double far = 0.0;
    for (int i = tid; i < n; i += T) {
        if ((sel_s[i >> 5] >> (i & 31)) & 1u) continue;
        const double* wi = w + (size_t)i * d;
        double near = INFINITY;
        for (int j = 0; j < n; ++j) {
            if (!((sel_s[j >> 5] >> (j & 31)) & 1u)) continue;
            near = fmin(near, ns_mlf_dist2(wi, w + (size_t)j * d, d));
        }
        far = fmax(far, near);                               // at least one index is selected, so near is finite
    }
    red_s[tid] = far;
    __syncthreads();
    for (int off = T >> 1; off > 0; off >>= 1) {
        if (tid < off) red_s[tid] = fmax(red_s[tid], red_s[tid + off]);
        __syncthreads();
    }
    if (tid == 0) r2_out[b] = red_s[0];
}

// The neighbour test of the candidate in u_s[0 .. d).  Called by EVERY thread of the workgroup with identical arguments after
// ns_unif_candidate returned 2; wc_s: d doubles of LDS, written here and read until the workgroup's next barrier pair, which the
// next candidate's ns_unif_candidate provides before this function runs again.  Returns workgroup-uniform 1 (a live point within
// r) or 0.
__device__ inline int ns_mlf_has_friend(const NsMlfArgs& m, int d, const double* u_s, double* wc_s) {
    const int tid = threadIdx.x;
    if (tid < d) {
        const double* R = m.metric_inv + (size_t)tid * d;
        double y = 0.0;
        for (int i = 0; i <= tid; ++i) y = fma(R[i], u_s[i], y);
        wc_s[tid] = y;
    }
    __syncthreads();
    int hit = 0;
    for (int j = tid; j < m.n; j += blockDim.x) hit |= (ns_mlf_dist2(wc_s, m.w + (size_t)j * d, d) <= m.r2) ? 1 : 0;
    return __syncthreads_or(hit) ? 1 : 0;
}

template <int D, bool GENERIC, int TMAX, bool TILED, bool NORMAL>
__global__ void __launch_bounds__(TMAX)
ns_mlf_draw_kernel(NsArgs p, NsUnifArgs q, NsMlfArgs m) {
    __shared__ double z_s[D], u_s[D], qs_s[D], wc_s[D];
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
        int st = ns_unif_candidate(q, (uint32_t)(q.cand_id0 + c), z_s, u_s, cnt_s);
        if (tid < d) q.cand_u[(size_t)c * d + tid] = u_s[tid];
        if (st == 2 && !ns_mlf_has_friend(m, d, u_s, wc_s)) st = 1;      // workgroup-uniform
        double lp = -INFINITY;
        if (st == 2) {
            if (tid < D) qs_s[tid] = tid < d ? ns_gp_coord<GENERIC, NORMAL>(p, nd_s, tid, u_s[tid]) : 0.0;
            __syncthreads();
            lp = ns_logl<D, GENERIC, TILED>(p, xa, aa, qs_s, scratch);
        }
        if (tid == 0) { q.cand_logl[c] = lp; q.cand_status[c] = st; }
    }
}

__global__ void __launch_bounds__(64)
ns_mlf_geom_kernel(NsUnifArgs q, NsMlfArgs m) {
    __shared__ double z_s[ALABI_MAX_DIM], u_s[ALABI_MAX_DIM], wc_s[ALABI_MAX_DIM];
    __shared__ int cnt_s[16];
    const int tid = threadIdx.x, d = q.d;
    for (long long c = blockIdx.x; c < q.M; c += gridDim.x) {
        int st = ns_unif_candidate(q, (uint32_t)(q.cand_id0 + c), z_s, u_s, cnt_s);
        if (tid < d) q.cand_u[(size_t)c * d + tid] = u_s[tid];
        if (st == 2 && !ns_mlf_has_friend(m, d, u_s, wc_s)) st = 1;
        if (tid == 0) { q.cand_logl[c] = -INFINITY; q.cand_status[c] = st; }
    }
}

}  // namespace alabi

using namespace alabi;

extern "C" {

int alabi_ns_mlf_radius(alabi_ns* ns, long long call, int n, const double* w, int B, double* r2_out, void* stream) {
    if (!ns || call < 0 || n < 1 || n > ALABI_NS_MLF_MAX_POINTS || B < 1 || !w || !r2_out) return ALABI_BAD_ARGUMENT;
    hipLaunchKernelGGL(ns_mlf_radius_kernel, dim3(B), dim3(ALABI_NS_MLF_RADIUS_T), 0, ns_stream(stream), ns->seed, call, n, ns->d, w,
                       r2_out);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int alabi_ns_mlf_draw(alabi_ns* ns, long long call, int cand_id0, int M, int evaluate, int E, const double* centres,
                      const double* axes, const double* inv_axes, const double* cum, int n, const double* w,
                      const double* metric_inv, double r2, double* cand_u, double* cand_logl, int* cand_status, void* stream) {
    // like every other bad argument of the draw, before its M == 0 return; a NaN r2 fails the comparison
    if (!w || !metric_inv || n < 1 || n > ALABI_NS_MLF_MAX_POINTS || !(r2 >= 0.0)) return ALABI_BAD_ARGUMENT;
    NsMlfArgs m{};
    m.w = w; m.metric_inv = metric_inv; m.r2 = r2; m.n = n;
    return ns_draw_launch(ns, call, cand_id0, M, evaluate, E, centres, axes, inv_axes, cum, cand_u, cand_logl, cand_status, stream,
                          ns_mlf_geom_kernel, [](auto inst) { return NS_KERNEL(ns_mlf_draw_kernel, inst); }, m);
}

}  // extern "C"
