// Gaussian kernel density estimate for gfx950: the log-density / density of scipy.stats.gaussian_kde as called by the
// reference's metrics (alabi/metrics.py:210-336, kl_divergence_kde):
//
//   p(q) = det(2 pi Sigma)^(-1/2) sum_i w_i exp(-|L^-1 (q - x_i)|^2 / 2),   Sigma = L L^T (scipy's cho_cov),  sum_i w_i = 1.
//
// Layout.  Samples and queries are centred on the plain mean c of the samples (r2 is translation invariant, and the augmented
// dot product below loses eps * (|z|^2 + |u|^2) / 2 absolutely, so samples thousands of bandwidths from the origin would
// otherwise cost digits -- the reason xa_centre_kernel exists for the GP), whitened, z = L^-1 (x - c), u = L^-1 (q - c), and
// augmented:
//   sample row  s' = (z, -|z|^2/2 + log w, 1, 0..)          [rows][Npad], rows = round_up(d + 2, 4)
//   query row   q' = (u, 1, -|u|^2/2, 0..) * 256/ln2          [Mpad][rows]
// so that q'.s' = (-r2/2 + log w) * 256/ln2 is the argument of exp2s_tab256 (2^(./256)) and v_mfma_f64_16x16x4f64 forms it
// for 16 queries x 16 samples per instruction (rows / 4 of them per tile).  The vector unit evaluates exp2s_tab256, one add and
// one max per evaluation -- the weights cost nothing in the inner loop.  Padding samples (N up to a multiple of 16) and zero
// weights carry z = 0 and log w = KDE_LOG0 (finite, so no 0 * inf anywhere): exp2s_tab256 clamps their argument and returns 0.
//
// Grid.  A workgroup is four wavefronts of 16 QT queries; the sample axis is cut into `parts` runs of `pts` samples (a
// multiple of 16), one per blockIdx.y, so a thousand queries against 10^5..10^6 samples still fill the chip.  Each
// (query, part) writes its partial sum and the largest exponent it met to a workspace; kde_combine_kernel adds the parts in
// ascending order.  The plan is a function of (N, M, d) only, so repeated calls are bit-identical on any device; no atomics.
//
// Tails.  Every exponent is <= log w <= 0, so the sum cannot overflow, but far from all samples it underflows (scipy's pdf is 0
// there, its logpdf finite).  logpdf: where the largest exponent of a query is below KDE_TAIL (natural log units) the combine
// flags the query and records that maximum as its shift; the partial kernel runs again over the waves holding a flagged
// query with the shift folded into the query's constant slot (q'_{d+1} = (-|u|^2/2 - shift) * 256/ln2 -- still free), and the
// second combine returns log(sum) + shift.  pdf needs no second pass: an underflowed density is 0, as scipy's.
#include <cmath>
#include <new>
#include <vector>
#include "gp_device.hpp"

#define KDE_LOG0 (-1.0e300)              /* log w of padding and zero-weight samples */
#define KDE_TAIL (-650.0)                /* largest exponent below this (natural log): rerun shifted */
#define KDE_LN2_256 0.0027076061740622863 /* ln2 / 256: scaled exponent -> natural log */
#define KDE_TARGET_WGS 2048LL            /* workgroups per call the sample split aims at (8 per CU on 256 CUs; device independent) */

typedef double v4f64 __attribute__((ext_vector_type(4)));

struct alabi_kde {
    int d = 0;
    int rows = 0;              // round_up(d + 2, 4)
    long long N = 0, Npad = 0; // samples, rounded up to 16
    bool ready = false;
    double log_norm = 0.0;     // -log det(2 pi Sigma) / 2
    double norm = 0.0;         // (2 pi)^(-d/2) / prod L_ii (scipy's evaluation order)
    double* Sa = nullptr;      // [rows][Npad] augmented sample rows
    size_t sa_bytes = 0;
    double* L = nullptr;       // [d][d] row-major lower Cholesky factor of Sigma
    double* centre = nullptr;  // [d]
    double* Qa = nullptr;      // workspace: [Mpad][rows] augmented query rows
    double* psum = nullptr;    // [parts][Mpad] partial sums
    double* pmax = nullptr;    // [parts][Mpad] largest exponent per part (scaled)
    double* shift = nullptr;   // [Mpad] tail shift (scaled), 0 where none
    int* flag = nullptr;       // [Mpad] 1 = rerun shifted
    size_t q_bytes = 0, p_bytes = 0, m_bytes = 0;
};

namespace alabi {

__global__ void __launch_bounds__(256)
kde_centre_kernel(const double* __restrict__ X, long long N, int d, double* __restrict__ centre) {
    __shared__ double scratch[16];
    const int k = blockIdx.x;
    double t = 0.0;
    for (long long n = threadIdx.x; n < N; n += 256) t += X[n * d + k];
    t = block_sum(t, scratch);
    if (threadIdx.x == 0) centre[k] = t / (double)N;
}

// z = L^-1 (x - c) by forward substitution with L [d][d] in LDS; z_k is written to out[k * os] (the caller's output row / column)
// and read back from there, so no array of d values has to live in registers.  Returns |z|^2.
__device__ inline double whiten(const double* __restrict__ x, int d, const double* __restrict__ c, const double* Ls, double* out,
                                size_t os) {
    double zz = 0.0;
    for (int k = 0; k < d; ++k) {
        double v = x[k] - c[k];
        for (int j = 0; j < k; ++j) v = fma(-Ls[k * d + j], out[(size_t)j * os], v);
        const double z = v / Ls[k * d + k];
        out[(size_t)k * os] = z;
        zz = fma(z, z, zz);
    }
    return zz;
}

__device__ inline void stage_L(const double* __restrict__ L, int d, double* Ls) {
    for (int e = threadIdx.x; e < d * d; e += blockDim.x) Ls[e] = L[e];
    __syncthreads();
}

__global__ void __launch_bounds__(256)
kde_prep_samples_kernel(const double* __restrict__ X, const double* __restrict__ logw, double logw_const, long long N,
                        long long Npad, int d, int rows, const double* __restrict__ L, const double* __restrict__ centre,
                        double* Sa) {
    extern __shared__ double Ls[];                                 // [d][d]
    stage_L(L, d, Ls);
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= Npad) return;
    double zz = 0.0, lw = KDE_LOG0;
    if (n < N) {
        zz = whiten(X + n * d, d, centre, Ls, Sa + n, (size_t)Npad);
        lw = logw ? logw[n] : logw_const;
        if (!(lw > KDE_LOG0)) lw = KDE_LOG0;   // log 0 = -inf (and a NaN weight) -> the finite sentinel
    } else {
        for (int k = 0; k < d; ++k) Sa[(size_t)k * Npad + n] = 0.0;
    }
    Sa[(size_t)d * Npad + n] = lw > KDE_LOG0 ? fma(-0.5, zz, lw) : KDE_LOG0;
    Sa[(size_t)(d + 1) * Npad + n] = 1.0;
    for (int k = d + 2; k < rows; ++k) Sa[(size_t)k * Npad + n] = 0.0;
}

__global__ void __launch_bounds__(256)
kde_prep_queries_kernel(const double* __restrict__ Q, long long M, long long Mpad, int d, int rows,
                        const double* __restrict__ L, const double* __restrict__ centre, double* Qa) {
    extern __shared__ double Ls[];                                 // [d][d]
    stage_L(L, d, Ls);
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= Mpad) return;
    double* row = Qa + (size_t)m * rows;
    if (m >= M) {                              // rows past M: all zero (their products are 0, never written out)
        for (int k = 0; k < rows; ++k) row[k] = 0.0;
        return;
    }
    const double qs = ALABI_EXP2S256_SCALE;
    const double uu = whiten(Q + m * d, d, centre, Ls, row, 1);
    for (int k = 0; k < d; ++k) row[k] *= qs;
    row[d] = qs;
    row[d + 1] = -0.5 * uu * qs;
    for (int k = d + 2; k < rows; ++k) row[k] = 0.0;
}

// Partial sums over samples [blockIdx.y * pts, +pts) for 4 x 16 QT queries per workgroup.  shift / flag NULL: first pass over
// every query; otherwise the tail pass: waves without a flagged query leave at once, the others subtract shift[m] from the
// constant slot sc = d + 1 of their A operands.
template <int KS, int QT>
__global__ void __launch_bounds__(256)
kde_partial_kernel(const double* __restrict__ Sa, long long Npad, int pts, const double* __restrict__ Qa, int rows, int sc,
                   long long M, const double* __restrict__ shift, const int* __restrict__ flag, double* __restrict__ psum,
                   double* __restrict__ pmax, long long stride) {
    __shared__ double etab[256];                                   // 2^(j/256) for exp2s_tab256
    etab[threadIdx.x] = exp2((double)threadIdx.x * 0.00390625);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const long long q0 = ((long long)blockIdx.x * 4 + wv) * (16 * QT);
    if (q0 >= M) return;
    if (flag) {
        bool need = false;
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            const long long m = q0 + 16 * qt + lr;
            need = need || (m < M && flag[m] != 0);
        }
        if (!__any(need)) return;
    }
    // A operands: query row lr of tile qt, coordinate 4 s + lk of k-step s
    double a[QT][KS];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const long long m = q0 + 16 * qt + lr;
        const bool valid = m < M;
        const double sh = (shift && valid) ? shift[m] : 0.0;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int c = 4 * s + lk;
            double v = Qa[(size_t)m * rows + c];                   // rows past M exist (zero) up to the padded count
            if (c == sc) v -= sh;
            a[qt][s] = v;
        }
    }
    double sum[QT][4], mx[QT][4];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int i = 0; i < 4; ++i) { sum[qt][i] = 0.0; mx[qt][i] = -INFINITY; }
    const double* sb = Sa + (size_t)lk * Npad + lr;                // B operand: sample column lr of the tile, coordinate 4 s + lk
    const long long n_lo = (long long)blockIdx.y * pts, n_end = n_lo + pts;
    const long long n_hi = n_end < Npad ? n_end : Npad;
    for (long long n0 = n_lo; n0 < n_hi; n0 += 16) {
        double b[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) b[s] = sb[(size_t)(4 * s) * Npad + n0];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            v4f64 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[qt][s], b[s], acc, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {                         // C/D layout: row (query) lk + 4 i, column (sample) lr
                mx[qt][i] = fmax(mx[qt][i], acc[i]);
                sum[qt][i] += exp2s_tab256(acc[i], etab);
            }
        }
    }
    // fold the 16 sample columns of every query: the 16 lanes of a DPP row share lk; the sum ends in lane 15 of the row
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double v = sum[qt][i];
            v += dpp_move<0x111, 0xf>(v);
            v += dpp_move<0x112, 0xf>(v);
            v += dpp_move<0x114, 0xf>(v);
            v += dpp_move<0x118, 0xf>(v);
            double w = mx[qt][i];                                  // max: xor shuffles inside the 16-lane row (no zero fill)
            w = fmax(w, __shfl_xor(w, 1, 64));
            w = fmax(w, __shfl_xor(w, 2, 64));
            w = fmax(w, __shfl_xor(w, 4, 64));
            w = fmax(w, __shfl_xor(w, 8, 64));
            const long long m = q0 + 16 * qt + lk + 4 * i;
            if (lr == 15 && m < M) {
                psum[(size_t)blockIdx.y * stride + m] = v;
                pmax[(size_t)blockIdx.y * stride + m] = w;
            }
        }
}

// mode 0: pdf = sum * norm.  mode 1: logpdf first pass (flags the tail).  mode 2: logpdf of the flagged queries after the
// shifted pass.  The parts are added in ascending order.
__global__ void __launch_bounds__(256)
kde_combine_kernel(const double* __restrict__ psum, const double* __restrict__ pmax, int parts, long long stride, long long M,
                   int mode, double log_norm, double norm, double* __restrict__ shift, int* __restrict__ flag,
                   double* __restrict__ out) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    if (mode == 2 && flag[m] == 0) return;
    double s = 0.0;
    for (int k = 0; k < parts; ++k) s += psum[(size_t)k * stride + m];
    if (mode == 0) {
        out[m] = s * norm;
    } else if (mode == 1) {
        double w = -INFINITY;
        for (int k = 0; k < parts; ++k) w = fmax(w, pmax[(size_t)k * stride + m]);
        const bool tail = w * KDE_LN2_256 < KDE_TAIL;
        flag[m] = tail ? 1 : 0;
        shift[m] = tail ? w : 0.0;
        if (!tail) out[m] = log(s) + log_norm;
    } else {
        out[m] = log(s) + fma(shift[m], KDE_LN2_256, log_norm);
    }
}

}  // namespace alabi

using namespace alabi;

#define ALABI_DISPATCH_KS17(KS_, ...)                                                           \
    switch (KS_) {                                                                              \
        case 1: { constexpr int KS = 1; __VA_ARGS__; } break;                                   \
        case 2: { constexpr int KS = 2; __VA_ARGS__; } break;                                   \
        case 3: { constexpr int KS = 3; __VA_ARGS__; } break;                                   \
        case 4: { constexpr int KS = 4; __VA_ARGS__; } break;                                   \
        case 5: { constexpr int KS = 5; __VA_ARGS__; } break;                                   \
        case 6: { constexpr int KS = 6; __VA_ARGS__; } break;                                   \
        case 7: { constexpr int KS = 7; __VA_ARGS__; } break;                                   \
        case 8: { constexpr int KS = 8; __VA_ARGS__; } break;                                   \
        case 9: { constexpr int KS = 9; __VA_ARGS__; } break;                                   \
        case 10: { constexpr int KS = 10; __VA_ARGS__; } break;                                 \
        case 11: { constexpr int KS = 11; __VA_ARGS__; } break;                                 \
        case 12: { constexpr int KS = 12; __VA_ARGS__; } break;                                 \
        case 13: { constexpr int KS = 13; __VA_ARGS__; } break;                                 \
        case 14: { constexpr int KS = 14; __VA_ARGS__; } break;                                 \
        case 15: { constexpr int KS = 15; __VA_ARGS__; } break;                                 \
        case 16: { constexpr int KS = 16; __VA_ARGS__; } break;                                 \
        case 17: { constexpr int KS = 17; __VA_ARGS__; } break;                                 \
        default: return ALABI_BAD_ARGUMENT;                                                     \
    }

namespace {

// Query tiles per wavefront: four (64 queries) while the A operands fit comfortably in registers, two above d = 30.
inline int kde_qt(int rows) { return rows / 4 <= 8 ? 4 : 2; }

struct KdePlan {
    long long wgs, mpad, stride;
    int parts, pts;
};

// A function of (N, M, d) only: repeated calls split the sample axis identically on every device.
KdePlan kde_plan(long long Npad, long long M, int rows) {
    KdePlan p;
    const long long qpb = 4LL * 16 * kde_qt(rows);
    p.wgs = (M + qpb - 1) / qpb;
    p.mpad = p.wgs * qpb;
    p.stride = p.mpad;
    const long long tiles = Npad / 16;
    long long parts = 1;
    if (p.wgs < KDE_TARGET_WGS) {
        parts = (KDE_TARGET_WGS + p.wgs - 1) / p.wgs;
        if (parts > tiles / 8) parts = tiles / 8;                  // at least eight 16-sample tiles per part
        if (parts < 1) parts = 1;
    }
    const long long tiles_per = (tiles + parts - 1) / parts;
    p.pts = (int)(tiles_per * 16);
    p.parts = (int)((Npad + p.pts - 1) / p.pts);
    return p;
}

template <typename T>
int grow(T** buf, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return ALABI_OK;
    if (*buf) ALABI_HIP_CHECK(hipFree(*buf));
    *buf = nullptr;
    *cap = 0;
    ALABI_HIP_CHECK(hipMalloc((void**)buf, bytes));
    *cap = bytes;
    return ALABI_OK;
}

int kde_run(alabi_kde* kde, const double* Q, long long M, double* out, bool log_out, hipStream_t s) {
    if (!kde) return ALABI_BAD_ARGUMENT;
    if (!kde->ready) return ALABI_NOT_COMPUTED;
    if (M < 0) return ALABI_BAD_ARGUMENT;
    if (M == 0) return ALABI_OK;
    if (!Q || !out) return ALABI_BAD_ARGUMENT;
    const int d = kde->d, rows = kde->rows;
    const KdePlan p = kde_plan(kde->Npad, M, rows);
    if (p.wgs > 0x7fffffffLL || p.parts > 65535) return ALABI_BAD_ARGUMENT;
    int st;
    size_t qcap = kde->q_bytes;
    if ((st = grow(&kde->Qa, &qcap, (size_t)p.mpad * rows * sizeof(double))) != ALABI_OK) return st;
    kde->q_bytes = qcap;
    const size_t pbytes = (size_t)p.parts * p.stride * sizeof(double);
    if (pbytes > kde->p_bytes) {
        size_t c1 = kde->p_bytes, c2 = kde->p_bytes;
        if ((st = grow(&kde->psum, &c1, pbytes)) != ALABI_OK) return st;
        if ((st = grow(&kde->pmax, &c2, pbytes)) != ALABI_OK) return st;
        kde->p_bytes = pbytes;
    }
    const size_t mbytes = (size_t)p.mpad * sizeof(double);
    if (mbytes > kde->m_bytes) {
        size_t c1 = kde->m_bytes, c2 = kde->m_bytes;
        if ((st = grow(&kde->shift, &c1, mbytes)) != ALABI_OK) return st;
        if ((st = grow(&kde->flag, &c2, mbytes)) != ALABI_OK) return st;   // int32 [Mpad] in an Mpad-double allocation
        kde->m_bytes = mbytes;
    }
    const size_t lds = (size_t)d * d * sizeof(double);
    hipLaunchKernelGGL(kde_prep_queries_kernel, dim3((unsigned)((p.mpad + 255) / 256)), dim3(256), lds, s, Q, M, p.mpad, d, rows,
                       kde->L, kde->centre, kde->Qa);
    const int ks = rows / 4, qt = kde_qt(rows);
    const unsigned cgrid = (unsigned)((M + 255) / 256);
    auto partial = [&](const double* shift, const int* flag) -> int {
        if (qt == 4) {
            ALABI_DISPATCH_KS17(ks, if constexpr (KS <= 8) hipLaunchKernelGGL((kde_partial_kernel<KS, 4>), dim3((unsigned)p.wgs, p.parts),
                dim3(256), 0, s, kde->Sa, kde->Npad, p.pts, kde->Qa, rows, d + 1, M, shift, flag, kde->psum, kde->pmax, p.stride));
        } else {
            ALABI_DISPATCH_KS17(ks, if constexpr (KS > 8) hipLaunchKernelGGL((kde_partial_kernel<KS, 2>), dim3((unsigned)p.wgs, p.parts),
                dim3(256), 0, s, kde->Sa, kde->Npad, p.pts, kde->Qa, rows, d + 1, M, shift, flag, kde->psum, kde->pmax, p.stride));
        }
        return ALABI_OK;
    };
    if ((st = partial(nullptr, nullptr)) != ALABI_OK) return st;
    if (!log_out) {
        hipLaunchKernelGGL(kde_combine_kernel, dim3(cgrid), dim3(256), 0, s, kde->psum, kde->pmax, p.parts, p.stride, M, 0,
                           kde->log_norm, kde->norm, kde->shift, kde->flag, out);
        ALABI_LAUNCH_CHECK();
        return ALABI_OK;
    }
    hipLaunchKernelGGL(kde_combine_kernel, dim3(cgrid), dim3(256), 0, s, kde->psum, kde->pmax, p.parts, p.stride, M, 1,
                       kde->log_norm, kde->norm, kde->shift, kde->flag, out);
    if ((st = partial(kde->shift, kde->flag)) != ALABI_OK) return st;
    hipLaunchKernelGGL(kde_combine_kernel, dim3(cgrid), dim3(256), 0, s, kde->psum, kde->pmax, p.parts, p.stride, M, 2,
                       kde->log_norm, kde->norm, kde->shift, kde->flag, out);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // namespace

int alabi_kde_create(int d, alabi_kde** out) {
    if (!out || d < 1 || d > ALABI_MAX_DIM) return ALABI_BAD_ARGUMENT;
    alabi_kde* k = new (std::nothrow) alabi_kde();
    if (!k) return ALABI_BAD_ARGUMENT;
    k->d = d;
    k->rows = round_up(d + 2, 4);
    if (hipMalloc(&k->L, (size_t)d * d * sizeof(double)) != hipSuccess ||
        hipMalloc(&k->centre, (size_t)d * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        if (k->L) (void)hipFree(k->L);
        delete k;
        g_last_error = "hipMalloc failed in alabi_kde_create";
        return ALABI_HIP_ERROR;
    }
    *out = k;
    return ALABI_OK;
}

int alabi_kde_destroy(alabi_kde* kde) {
    if (!kde) return ALABI_OK;
    for (double* p : {kde->Sa, kde->L, kde->centre, kde->Qa, kde->psum, kde->pmax, kde->shift, (double*)kde->flag})
        if (p) (void)hipFree(p);
    delete kde;
    return ALABI_OK;
}

int alabi_kde_set_data(alabi_kde* kde, const double* X, const double* logw, long long N, const double* cho_cov, void* stream) {
    if (!kde || !X || !cho_cov || N < 1) return ALABI_BAD_ARGUMENT;
    const int d = kde->d;
    if (N > (1LL << 40)) return ALABI_BAD_ARGUMENT;
    double norm = pow(2.0 * M_PI, -0.5 * d), half_log_det = 0.0;   // scipy's log_det / 2
    for (int k = 0; k < d; ++k) {
        const double lkk = cho_cov[k * d + k];
        if (!(lkk > 0.0) || !std::isfinite(lkk)) return ALABI_BAD_ARGUMENT;
        norm /= lkk;
        half_log_det += log(lkk * sqrt(2.0 * M_PI));
        for (int j = 0; j <= k; ++j)
            if (!std::isfinite(cho_cov[k * d + j])) return ALABI_BAD_ARGUMENT;
    }
    hipStream_t s = (hipStream_t)stream;
    kde->ready = false;
    const long long Npad = (N + 15) / 16 * 16;
    int st;
    if ((st = grow(&kde->Sa, &kde->sa_bytes, (size_t)kde->rows * Npad * sizeof(double))) != ALABI_OK) return st;
    // the factor's upper triangle is ignored: copy the lower one (the host array need not outlive the call)
    std::vector<double> Lh((size_t)d * d, 0.0);
    for (int k = 0; k < d; ++k)
        for (int j = 0; j <= k; ++j) Lh[(size_t)k * d + j] = cho_cov[k * d + j];
    ALABI_HIP_CHECK(hipMemcpyAsync(kde->L, Lh.data(), Lh.size() * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(kde_centre_kernel, dim3(d), dim3(256), 0, s, X, N, d, kde->centre);
    hipLaunchKernelGGL(kde_prep_samples_kernel, dim3((unsigned)((Npad + 255) / 256)), dim3(256), (size_t)d * d * sizeof(double), s,
                       X, logw, -log((double)N), N, Npad, d, kde->rows, kde->L, kde->centre, kde->Sa);
    ALABI_LAUNCH_CHECK();
    ALABI_HIP_CHECK(hipStreamSynchronize(s));   // Lh is pageable host memory
    kde->N = N;
    kde->Npad = Npad;
    kde->log_norm = -half_log_det;
    kde->norm = norm;
    kde->ready = true;
    return ALABI_OK;
}

int alabi_kde_logpdf(alabi_kde* kde, const double* Q, long long M, double* out, void* stream) {
    return kde_run(kde, Q, M, out, true, (hipStream_t)stream);
}

int alabi_kde_pdf(alabi_kde* kde, const double* Q, long long M, double* out, void* stream) {
    return kde_run(kde, Q, M, out, false, (hipStream_t)stream);
}

int alabi_kde_plan(alabi_kde* kde, long long M, int* parts, int* pts) {
    if (!kde || !kde->ready || M < 1 || !parts || !pts) return ALABI_BAD_ARGUMENT;
    const KdePlan p = kde_plan(kde->Npad, M, kde->rows);
    *parts = p.parts;
    *pts = p.pts;
    return ALABI_OK;
}
