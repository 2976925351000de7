// extern "C" entry points of libalabi_hip.so (declared in include/alabi_hip.h).
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "gp_device.hpp"

namespace alabi {
thread_local std::string g_last_error;

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

__global__ void __launch_bounds__(256)
copy_factor_kernel(const double* __restrict__ L, int ld, int N, double* __restrict__ out) {
    size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)N * N) return;
    int r = (int)(e / N), c = (int)(e % N);
    out[e] = (c <= r) ? L[(size_t)r * ld + c] : 0.0;
}

namespace {
struct CachedBuf { void* p; size_t bytes; };
std::mutex g_cache_mu;
std::vector<CachedBuf> g_cache;        // at most 4 buffers, the smallest is dropped first
}

void* dev_cache_take(size_t need, size_t* bytes) {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    int best = -1;
    for (int i = 0; i < (int)g_cache.size(); ++i)
        if (g_cache[i].bytes >= need && (best < 0 || g_cache[i].bytes < g_cache[best].bytes)) best = i;
    if (best < 0) return nullptr;
    void* p = g_cache[best].p;
    *bytes = g_cache[best].bytes;
    g_cache.erase(g_cache.begin() + best);
    return p;
}

void dev_cache_give(void* p, size_t bytes) {
    if (!p) return;
    void* drop = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        g_cache.push_back({p, bytes});
        if (g_cache.size() > 4) {
            int sm = 0;
            for (int i = 1; i < (int)g_cache.size(); ++i) if (g_cache[i].bytes < g_cache[sm].bytes) sm = i;
            drop = g_cache[sm].p;
            g_cache.erase(g_cache.begin() + sm);
        }
    }
    if (drop) (void)hipFree(drop);
}

int dev_alloc_cached(void** p, size_t need, size_t* bytes) {
    *p = dev_cache_take(need, bytes);
    if (*p) return (int)hipSuccess;
    const hipError_t e = hipMalloc(p, need);
    if (e != hipSuccess) { (void)hipGetLastError(); *p = nullptr; *bytes = 0; return (int)e; }
    *bytes = need;
    return (int)hipSuccess;
}

int grow_cached(double** p, size_t* bytes, size_t need, hipStream_t s) {
    if (need <= *bytes) return ALABI_OK;
    if (*p) {
        ALABI_HIP_CHECK(hipStreamSynchronize(s));
        dev_cache_give(*p, *bytes);
        *p = nullptr; *bytes = 0;
    }
    return dev_alloc_cached((void**)p, need, bytes) == (int)hipSuccess ? ALABI_OK : ALABI_NOT_COMPUTED;
}

int grow_plain(double** p, size_t* bytes, size_t need, hipStream_t s) {
    if (need <= *bytes) return ALABI_OK;
    if (*p) {
        ALABI_HIP_CHECK(hipStreamSynchronize(s));
        ALABI_HIP_CHECK(hipFree(*p));
        *p = nullptr; *bytes = 0;
    }
    ALABI_HIP_CHECK(hipMalloc(p, need));
    *bytes = need;
    return ALABI_OK;
}

static int fill_dimvec(DimVec& v, const double* src, int d, int stride, int off, double pad) {
    for (int k = 0; k < ALABI_MAX_DIM; ++k) v.v[k] = (k < d) ? src[k * stride + off] : pad;
    return 0;
}
}  // namespace alabi

using namespace alabi;

extern "C" {

int alabi_abi_version(void) { return 1; }

const char* alabi_status_string(int status) {
    switch (status) {
        case ALABI_OK: return "ok";
        case ALABI_NOT_POSITIVE_DEFINITE: return "matrix is not positive definite";
        case ALABI_BAD_ARGUMENT: return "bad argument";
        case ALABI_HIP_ERROR: return "HIP runtime error";
        case ALABI_NOT_COMPUTED: return "GP not computed / y not set";
        case ALABI_TIMEOUT: return "persistent ensemble kernel timed out waiting for a hand-off";
        default: return "unknown status";
    }
}

const char* alabi_last_error(void) { return g_last_error.c_str(); }

int alabi_device_info(int* n_cu, int* lds_bytes, char* arch) {
    int dev = 0;
    ALABI_HIP_CHECK(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    ALABI_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (lds_bytes) *lds_bytes = (int)prop.sharedMemPerBlock;
    if (arch) { strncpy(arch, prop.gcnArchName, 63); arch[63] = 0; }
    return ALABI_OK;
}

// ---------------------------------------------------------------------------------- GP
int alabi_gp_create(int n_cap, int d, alabi_gp** out) {
    if (!out || n_cap <= 0 || d <= 0 || d > ALABI_MAX_DIM) return ALABI_BAD_ARGUMENT;
    alabi_gp* gp = new (std::nothrow) alabi_gp();
    if (!gp) return ALABI_BAD_ARGUMENT;
    gp->n_cap = round_up(n_cap, ALABI_BLK);
    gp->d = d;
    for (int k = 0; k < ALABI_MAX_DIM; ++k) { gp->log_M[k] = 0.0; gp->inv_len.v[k] = (k < d) ? 1.0 : 0.0; }
    const size_t nc = gp->n_cap;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipMalloc(&gp->L, nc * nc * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&gp->Xt, (size_t)dim_bucket(d) * nc * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&gp->y, nc * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&gp->alpha, nc * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&gp->dinv, nc * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&gp->work, 2 * nc * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&gp->work2, nc * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&gp->flags, sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&gp->red, 4 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&gp->info, sizeof(int));
    if (e != hipSuccess) {
        alabi_gp_destroy(gp);
        return hip_fail(e, "hipMalloc(gp buffers)", __FILE__, __LINE__);
    }
    *out = gp;
    return ALABI_OK;
}

int alabi_gp_destroy(alabi_gp* gp) {
    if (!gp) return ALABI_OK;
    if (gp->L) (void)hipFree(gp->L);
    if (gp->Xt) (void)hipFree(gp->Xt);
    if (gp->Xa) (void)hipFree(gp->Xa);
    if (gp->xa_centre) (void)hipFree(gp->xa_centre);
    if (gp->host_status) (void)hipHostFree(gp->host_status);
    if (gp->point_host) (void)hipHostFree(gp->point_host);
    if (gp->point_dev) (void)hipFree(gp->point_dev);
    if (gp->y) (void)hipFree(gp->y);
    if (gp->alpha) (void)hipFree(gp->alpha);
    if (gp->dinv) (void)hipFree(gp->dinv);
    if (gp->work) (void)hipFree(gp->work);
    if (gp->work2) (void)hipFree(gp->work2);
    if (gp->flags) (void)hipFree(gp->flags);
    if (gp->red) (void)hipFree(gp->red);
    if (gp->info) (void)hipFree(gp->info);
    if (gp->chol_ctl) (void)hipFree(gp->chol_ctl);
    if (gp->ws || gp->winv) (void)hipDeviceSynchronize();   // nothing in flight may still use the buffers handed to the cache
    alabi::dev_cache_give(gp->ws, gp->ws_bytes);
    if (gp->scan) (void)hipFree(gp->scan);
    alabi::dev_cache_give(gp->winv, gp->winv_bytes);
    if (gp->small) (void)hipFree(gp->small);
    if (gp->pgrad) (void)hipFree(gp->pgrad);
    if (gp->Xc) (void)hipFree(gp->Xc);
    if (gp->ens_h) (void)hipFree(gp->ens_h);
    if (gp->mupart) (void)hipFree(gp->mupart);
    delete gp;
    return ALABI_OK;
}

int alabi_gp_set_hyper(alabi_gp* gp, double mean, double log_white_noise, double log_amp, const double* log_M) {
    if (!gp || !log_M) return ALABI_BAD_ARGUMENT;
    if (!std::isfinite(mean) || !std::isfinite(log_white_noise) || !std::isfinite(log_amp)) return ALABI_BAD_ARGUMENT;
    for (int k = 0; k < gp->d; ++k)
        if (!std::isfinite(log_M[k])) return ALABI_BAD_ARGUMENT;
    gp->mean = mean; gp->log_wn = log_white_noise; gp->log_amp = log_amp;
    for (int k = 0; k < gp->d; ++k) { gp->log_M[k] = log_M[k]; gp->inv_len.v[k] = std::exp(-0.5 * log_M[k]); }
    gp->computed = false; gp->has_alpha = false; gp->gen++;
    return ALABI_OK;
}

int alabi_gp_set_kernel(alabi_gp* gp, int kernel_type, double log_alpha) {
    if (!gp || kernel_type < 0 || kernel_type > 3 || !std::isfinite(log_alpha)) return ALABI_BAD_ARGUMENT;
    gp->kf.type = kernel_type;
    gp->kf.alpha = std::exp(log_alpha);
    gp->computed = false; gp->has_alpha = false; gp->gen++;
    return ALABI_OK;
}

int alabi_gp_compute(alabi_gp* gp, const double* X, int N, void* stream) {
    if (!gp || !X || N <= 0 || N > gp->n_cap) return ALABI_BAD_ARGUMENT;
    hipStream_t s = as_stream(stream);
    gp->N = N; gp->Npad = round_up(N, ALABI_BLK);
    gp->computed = false; gp->has_alpha = false; gp->gen++;
    int st;
    if ((st = launch_prepare_inputs(gp, X, N, s)) != ALABI_OK) return st;
    // 3..256 block columns: the task-queue factorisation (one launch); a wait that runs out there is remembered for a while
    static std::atomic<int> tasks_penalty{0};
    int queued = 0, ctl_ints = 0;
    // a forced queue (chol_tasks.hpp): then the penalty does not apply either
    if (!chol_queue_forced_on(chol_switches()) && tasks_penalty.load(std::memory_order_relaxed) > 0) tasks_penalty.fetch_sub(1, std::memory_order_relaxed);
    else if ((st = cholesky_tasks_prepare(gp, s, &ctl_ints)) != ALABI_OK) return st;
    if ((st = launch_assemble(gp, s, ctl_ints)) != ALABI_OK) return st;   // also clears the status word and the queue's control words
    if (ctl_ints > 0 && (st = launch_cholesky_tasks(gp, s, &queued)) != ALABI_OK) return st;
    if (!queued && (st = launch_cholesky(gp, s)) != ALABI_OK) return st;
    // one read-back of (pivot status, queue time-out) into pinned memory, one synchronisation
    if (!gp->host_status) ALABI_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&gp->host_status), 2 * sizeof(int), hipHostMallocDefault));
    gp->host_status[1] = 0;
    ALABI_HIP_CHECK(hipMemcpyAsync(&gp->host_status[0], gp->info, sizeof(int), hipMemcpyDeviceToHost, s));
    if (queued) ALABI_HIP_CHECK(hipMemcpyAsync(&gp->host_status[1], gp->chol_ctl + 1, sizeof(int), hipMemcpyDeviceToHost, s));
    ALABI_HIP_CHECK(hipStreamSynchronize(s));
    gp->factor_path = queued ? 2 : 1;
    if (queued && gp->host_status[1]) {                     // undefined matrix state: assemble and factorise again, step by step
        gp->factor_path = 3;
        tasks_penalty.store(64, std::memory_order_relaxed);
        if ((st = launch_assemble(gp, s)) != ALABI_OK) return st;
        if ((st = launch_cholesky(gp, s)) != ALABI_OK) return st;
        ALABI_HIP_CHECK(hipMemcpyAsync(&gp->host_status[0], gp->info, sizeof(int), hipMemcpyDeviceToHost, s));
        ALABI_HIP_CHECK(hipStreamSynchronize(s));
    }
    const int info = gp->host_status[0];
    gp->last_pivot = info;
    if (info != 0) return ALABI_NOT_POSITIVE_DEFINITE;
    gp->computed = true;
    gp->factor_gen++;
    return ALABI_OK;
}

int alabi_gp_fit_predict(alabi_gp* gp, const double* X, int N, const double* y, const double* Xs, long long M, double* mu,
                         double* nll_out, void* stream) {
    if (!gp || !y || !nll_out || M < 0 || (M > 0 && (!Xs || !mu))) return ALABI_BAD_ARGUMENT;
    int st = alabi_gp_compute(gp, X, N, stream);
    if (st != ALABI_OK) return st;
    if ((st = alabi_gp_set_y(gp, y, stream)) != ALABI_OK) return st;
    if ((st = alabi_gp_nll(gp, nll_out, stream)) != ALABI_OK) return st;
    if (M > 0) st = alabi_gp_predict(gp, Xs, M, mu, nullptr, stream);
    return st;
}

int alabi_gp_append(alabi_gp* gp, const double* x_new, void* stream) {
    if (!gp || !x_new) return ALABI_BAD_ARGUMENT;
    if (!gp->computed) return ALABI_NOT_COMPUTED;
    if (gp->N >= gp->Npad || gp->N + 1 > gp->n_cap) return ALABI_BAD_ARGUMENT;      // no padding row left: refit
    hipStream_t s = as_stream(stream);
    int st = ensure_winv(gp, s);
    if (st == ALABI_NOT_COMPUTED) return ALABI_BAD_ARGUMENT;                          // no room for the cached L^-1: refit
    if (st != ALABI_OK) return st;
    if ((st = launch_append(gp, x_new, s)) != ALABI_OK) return st;
    int info = 0;
    ALABI_HIP_CHECK(hipMemcpyAsync(&info, gp->info, sizeof(int), hipMemcpyDeviceToHost, s));
    ALABI_HIP_CHECK(hipStreamSynchronize(s));
    gp->last_pivot = info;
    if (info != 0) return ALABI_NOT_POSITIVE_DEFINITE;                                // factor and cache untouched
    gp->N += 1;
    gp->has_alpha = false;
    gp->gen++; gp->factor_gen++;
    gp->winv_gen = gp->factor_gen;                                                    // the cache was extended with the factor
    return ALABI_OK;
}

int alabi_gp_set_mean(alabi_gp* gp, double mean) {
    if (!gp || !std::isfinite(mean)) return ALABI_BAD_ARGUMENT;
    if (mean != gp->mean) { gp->mean = mean; gp->has_alpha = false; gp->gen++; }
    return ALABI_OK;
}

int alabi_gp_last_pivot(alabi_gp* gp, int* pivot) {
    if (!gp || !pivot) return ALABI_BAD_ARGUMENT;
    *pivot = gp->last_pivot;
    return ALABI_OK;
}

int alabi_gp_n(alabi_gp* gp, int* n) {
    if (!gp || !n) return ALABI_BAD_ARGUMENT;
    *n = gp->N;
    return ALABI_OK;
}

int alabi_gp_set_y(alabi_gp* gp, const double* y, void* stream) {
    if (!gp || !y) return ALABI_BAD_ARGUMENT;
    if (!gp->computed) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    ALABI_HIP_CHECK(hipMemcpyAsync(gp->y, y, (size_t)gp->N * sizeof(double), hipMemcpyDeviceToDevice, s));
    int st = launch_alpha(gp, s);
    if (st != ALABI_OK) return st;
    gp->has_alpha = true; gp->gen++;
    return ALABI_OK;
}

int alabi_gp_predict(alabi_gp* gp, const double* Xs, long long M, double* mu, double* var, void* stream) {
    if (!gp || M < 0 || (M > 0 && (!Xs || !mu))) return ALABI_BAD_ARGUMENT;
    if (!gp->computed || !gp->has_alpha) return ALABI_NOT_COMPUTED;
    if (M == 0) return ALABI_OK;
    hipStream_t s = as_stream(stream);
    const PredictSwitches sw = predict_switches();
    if (var) {
        // small batches: groups of 16 multiply with the cached L^-1, one workgroup per (block row, group), K* evaluated in
        // place -- no pre-pass, no substitution chain (the path of per-point objective calls: utility.py:1030-1163, core.py:1441)
        if (predict_var_small(M, gp->Npad, gp->d, sw)) return launch_predict_var_small(gp, Xs, (int)M, mu, var, sw, s);
        return launch_predict_var(gp, Xs, M, mu, var, sw, s);
    }
    return launch_predict_mean(gp, Xs, M, mu, sw, s);
}

int alabi_gp_predict_grad(alabi_gp* gp, const double* Xs, long long M, double* mu, double* var, double* dmu, double* dvar,
                          void* stream) {
    if (!gp || M < 0 || (M > 0 && (!Xs || !dmu || !dvar))) return ALABI_BAD_ARGUMENT;
    if (!gp->computed || !gp->has_alpha) return ALABI_NOT_COMPUTED;
    if (M == 0) return ALABI_OK;
    return launch_predict_grad(gp, Xs, M, mu, var, dmu, dvar, as_stream(stream));
}

// One point in, its value and gradient out, everything on the host side: the evaluation an optimiser makes ~30 times per
// active-learning iteration (the polish step of find_next_point).  Pinned staging buffers owned by the handle: one small copy in,
// the three kernels, one small copy out, one synchronisation -- no tensor is created on the way.
int alabi_gp_predict_grad_point(alabi_gp* gp, const double* x, double* out, void* stream) {
    if (!gp || !x || !out) return ALABI_BAD_ARGUMENT;
    if (!gp->computed || !gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    const int d = gp->d, nres = 2 + 2 * d;
    if (!gp->point_host) {
        ALABI_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&gp->point_host), (size_t)(3 + 3 * ALABI_MAX_DIM) * sizeof(double), hipHostMallocDefault));
        ALABI_HIP_CHECK(hipMalloc(&gp->point_dev, (size_t)(3 + 3 * ALABI_MAX_DIM) * sizeof(double)));
    }
    // Zero copy: the kernels read the point from and write the 2 + 2 d results to the pinned (device-visible, coherent) staging buffer
    // themselves -- two copy operations fewer on the stream per evaluation (ALABI_POINT_COPY=1: explicit copies, the earlier form).
    static const bool copies = [] { const char* e = getenv("ALABI_POINT_COPY"); return e && e[0] == '1'; }();
    for (int k = 0; k < d; ++k) gp->point_host[k] = x[k];
    int st;
    if (copies) {
        double* xd = gp->point_dev; double* res = gp->point_dev + d;      // res: mu, var, dmu[d], dvar[d]
        ALABI_HIP_CHECK(hipMemcpyAsync(xd, gp->point_host, (size_t)d * sizeof(double), hipMemcpyHostToDevice, s));
        if ((st = launch_predict_grad(gp, xd, 1, res, res + 1, res + 2, res + 2 + d, s)) != ALABI_OK) return st;
        ALABI_HIP_CHECK(hipMemcpyAsync(gp->point_host + d, res, (size_t)nres * sizeof(double), hipMemcpyDeviceToHost, s));
    } else {
        double* res = gp->point_host + d;
        if ((st = launch_predict_grad(gp, gp->point_host, 1, res, res + 1, res + 2, res + 2 + d, s)) != ALABI_OK) return st;
    }
    ALABI_HIP_CHECK(hipStreamSynchronize(s));
    for (int k = 0; k < nres; ++k) out[k] = gp->point_host[d + k];
    return ALABI_OK;
}

static int gp_reductions_to_host(alabi_gp* gp, double out[2], hipStream_t s) {
    int st = launch_reductions(gp, s);
    if (st != ALABI_OK) return st;
    ALABI_HIP_CHECK(hipMemcpyAsync(out, gp->red, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    ALABI_HIP_CHECK(hipStreamSynchronize(s));
    return ALABI_OK;
}

int alabi_gp_logdet(alabi_gp* gp, double* out, void* stream) {
    if (!gp || !out) return ALABI_BAD_ARGUMENT;
    if (!gp->computed) return ALABI_NOT_COMPUTED;
    double r[2];
    int st = gp_reductions_to_host(gp, r, as_stream(stream));
    if (st != ALABI_OK) return st;
    *out = r[0];
    return ALABI_OK;
}

int alabi_gp_nll(alabi_gp* gp, double* out, void* stream) {
    if (!gp || !out) return ALABI_BAD_ARGUMENT;
    if (!gp->computed || !gp->has_alpha) return ALABI_NOT_COMPUTED;
    double r[2];
    int st = gp_reductions_to_host(gp, r, as_stream(stream));
    if (st != ALABI_OK) return st;
    *out = 0.5 * r[1] + 0.5 * r[0] + 0.5 * gp->N * std::log(2.0 * 3.141592653589793);
    return ALABI_OK;
}

int alabi_gp_grad_log_likelihood(alabi_gp* gp, double* grad_out, void* stream) {
    if (!gp || !grad_out) return ALABI_BAD_ARGUMENT;
    if (!gp->computed || !gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    double* grad_dev = gp->work;                       // solve scratch, free once alpha exists (2 n_cap >= d + 4 doubles)
    if (2 * (size_t)gp->n_cap < (size_t)gp->d + 4) return ALABI_BAD_ARGUMENT;
    int st = launch_grad_log_likelihood(gp, grad_dev, s);
    if (st != ALABI_OK) return st;
    ALABI_HIP_CHECK(hipMemcpyAsync(grad_out, grad_dev, (size_t)(gp->d + 4) * sizeof(double), hipMemcpyDeviceToHost, s));
    ALABI_HIP_CHECK(hipStreamSynchronize(s));
    return ALABI_OK;
}

int alabi_gp_get_alpha(alabi_gp* gp, double* alpha_out, void* stream) {
    if (!gp || !alpha_out) return ALABI_BAD_ARGUMENT;
    if (!gp->computed || !gp->has_alpha) return ALABI_NOT_COMPUTED;
    ALABI_HIP_CHECK(hipMemcpyAsync(alpha_out, gp->alpha, (size_t)gp->N * sizeof(double), hipMemcpyDeviceToDevice,
                                   as_stream(stream)));
    return ALABI_OK;
}

int alabi_gp_get_factor(alabi_gp* gp, double* L_out, void* stream) {
    if (!gp || !L_out) return ALABI_BAD_ARGUMENT;
    if (!gp->computed) return ALABI_NOT_COMPUTED;
    size_t n2 = (size_t)gp->N * gp->N;
    hipLaunchKernelGGL(copy_factor_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, as_stream(stream),
                       gp->L, gp->Npad, gp->N, L_out);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int alabi_gp_last_factor_path(alabi_gp* gp, int* path) {
    if (!gp || !path) return ALABI_BAD_ARGUMENT;
    *path = gp->factor_path;
    return ALABI_OK;
}

int alabi_gp_last_solve_path(alabi_gp* gp, int* path) {
    if (!gp || !path) return ALABI_BAD_ARGUMENT;
    *path = gp->solve_path;
    return ALABI_OK;
}

int alabi_gp_get_inverse(alabi_gp* gp, double* Kinv_out, void* stream) {
    if (!gp || !Kinv_out) return ALABI_BAD_ARGUMENT;
    if (!gp->computed) return ALABI_NOT_COMPUTED;
    return launch_get_inverse(gp, Kinv_out, as_stream(stream));
}

int alabi_kernel_matrix(const double* X1, int n1, const double* X2, int n2, int d, int kernel_type, double log_alpha,
                        double log_amp, const double* log_M, double* K_out, void* stream) {
    if (!X1 || !X2 || !K_out || !log_M || n1 <= 0 || n2 <= 0 || d <= 0 || d > ALABI_MAX_DIM || kernel_type < 0 ||
        kernel_type > 3)
        return ALABI_BAD_ARGUMENT;
    const KernelFn kf{kernel_type, std::exp(log_alpha)};
    DimVec inv;
    for (int k = 0; k < ALABI_MAX_DIM; ++k) inv.v[k] = (k < d) ? std::exp(-0.5 * log_M[k]) : 0.0;
    return launch_kernel_matrix(X1, n1, X2, n2, d, std::exp(log_amp), inv, kf, K_out, as_stream(stream));
}

// ----------------------------------------------------------------------------- utility
int alabi_utility_eval(int algo, const double* Xs, long long M, int d, const double* bounds, double y_best,
                       const double* mu, const double* var, double* u, void* stream) {
    if (algo < 0 || algo > 2 || M < 0 || d <= 0 || d > ALABI_MAX_DIM || !bounds) return ALABI_BAD_ARGUMENT;
    if (M == 0) return ALABI_OK;
    if (!Xs || !mu || !var || !u) return ALABI_BAD_ARGUMENT;
    DimVec lo, hi;
    fill_dimvec(lo, bounds, d, 2, 0, 0.0);
    fill_dimvec(hi, bounds, d, 2, 1, 0.0);
    return launch_utility_eval(algo, Xs, M, d, lo, hi, y_best, mu, var, u, as_stream(stream));
}

int alabi_utility_scan(alabi_gp* gp, int algo, const double* Xs, long long M, const double* bounds, double y_best,
                       double* u, double* mu_out, double* var_out, double* best_val, long long* best_idx,
                       void* stream) {
    if (!gp || algo < 0 || algo > 2 || M <= 0 || !Xs || !bounds || !best_val || !best_idx) return ALABI_BAD_ARGUMENT;
    if (!gp->computed || !gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    const int nblocks = 1024;
    const size_t need = ((size_t)3 * M + 2 * nblocks) * sizeof(double);
    int st;
    if ((st = grow_plain(&gp->scan, &gp->scan_bytes, need, s)) != ALABI_OK) return st;
    double* pv = gp->scan;
    long long* pi = reinterpret_cast<long long*>(gp->scan + nblocks);
    double* mu = mu_out ? mu_out : gp->scan + 2 * nblocks;
    double* var = var_out ? var_out : gp->scan + 2 * nblocks + M;
    double* uu = u ? u : gp->scan + 2 * nblocks + 2 * M;
    if ((st = launch_predict_var(gp, Xs, M, mu, var, predict_switches(), s)) != ALABI_OK) return st;
    DimVec lo, hi;
    fill_dimvec(lo, bounds, gp->d, 2, 0, 0.0);
    fill_dimvec(hi, bounds, gp->d, 2, 1, 0.0);
    if ((st = launch_utility_eval(algo, Xs, M, gp->d, lo, hi, y_best, mu, var, uu, s)) != ALABI_OK) return st;
    if ((st = launch_argmin(uu, M, pv, pi, nblocks, s)) != ALABI_OK) return st;
    double hv; long long hi_idx;
    ALABI_HIP_CHECK(hipMemcpyAsync(&hv, pv, sizeof(double), hipMemcpyDeviceToHost, s));
    ALABI_HIP_CHECK(hipMemcpyAsync(&hi_idx, pi, sizeof(long long), hipMemcpyDeviceToHost, s));
    ALABI_HIP_CHECK(hipStreamSynchronize(s));
    *best_idx = hi_idx;
    *best_val = (hi_idx >= 0) ? hv : NAN;
    return ALABI_OK;
}

// ---------------------------------------------------------------------------- ensemble
static void free_draws(DrawBuffers& b) {
    if (b.order) (void)hipFree(b.order);
    if (b.cw) (void)hipFree(b.cw);
    if (b.zz) (void)hipFree(b.zz);
    if (b.lnfac) (void)hipFree(b.lnfac);
    if (b.lnu) (void)hipFree(b.lnu);
    if (b.partner) (void)hipFree(b.partner);
    if (b.u_z) (void)hipFree(b.u_z);
    if (b.u_acc) (void)hipFree(b.u_acc);
    if (b.packed) (void)hipFree(b.packed);
    if (b.pos_of) (void)hipFree(b.pos_of);
    if (b.link) (void)hipFree(b.link);
    if (b.packed_x) (void)hipFree(b.packed_x);
    if (b.place) (void)hipFree(b.place);
    b = DrawBuffers{};
}

static hipError_t alloc_draws(DrawBuffers& b, size_t n) {
    hipError_t err = hipSuccess;
    if (err == hipSuccess) err = hipMalloc(&b.order, n * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&b.cw, n * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&b.zz, n * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&b.lnfac, n * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&b.lnu, n * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&b.partner, n * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&b.u_z, n * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&b.u_acc, n * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&b.packed, 4 * n * sizeof(unsigned long long));
    if (err == hipSuccess) err = hipMalloc(&b.pos_of, n * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&b.link, 2 * n * sizeof(unsigned long long));
    return err;
}

// Second set of draw buffers, side stream and events for drawing one chunk ahead; created on the first multi-chunk stream call.
// Not available (single buffer, draws on the main stream) when the set would be large or anything fails to allocate.
static bool ens_draw_ahead_ready(alabi_ens* e) {
    if (e->draws2_state != 0) return e->draws2_state > 0;
    e->draws2_state = -1;
    const size_t n = (size_t)e->chunk_cap * e->W * e->E;
    if (n > ((size_t)1 << 20)) return false;                       // 104 bytes per record: at most 109 MB
    bool ok = alloc_draws(e->draws2, n) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&e->side_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&e->ev_free, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&e->ev_drawn, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        free_draws(e->draws2);
        if (e->side_stream) { (void)hipStreamDestroy(e->side_stream); e->side_stream = nullptr; }
        if (e->ev_free) { (void)hipEventDestroy(e->ev_free); e->ev_free = nullptr; }
        if (e->ev_drawn) { (void)hipEventDestroy(e->ev_drawn); e->ev_drawn = nullptr; }
        return false;
    }
    e->draws2_state = 1;
    return true;
}

static void free_move_buffers(MoveBuffers& m) {
    if (m.cw2) (void)hipFree(m.cw2);
    if (m.partner2) (void)hipFree(m.partner2);
    if (m.move) (void)hipFree(m.move);
    if (m.cw3) (void)hipFree(m.cw3);
    if (m.partner3) (void)hipFree(m.partner3);
    if (m.kind) (void)hipFree(m.kind);
    if (m.par) (void)hipFree(m.par);
    m = MoveBuffers{};
}

static void free_kde_buffers(KdeBuffers& k) {
    if (k.white) (void)hipFree(k.white);
    if (k.L) (void)hipFree(k.L);
    if (k.mean) (void)hipFree(k.mean);
    if (k.flag) (void)hipFree(k.flag);
    if (k.singular) (void)hipFree(k.singular);
    k = KdeBuffers{};
}

// The second-partner arrays of the records (first buffer set), allocated when a move set is first given or a DE step is injected;
// the third-partner arrays when the set holds a snooker move or a snooker step is injected.
static int ensure_move_buffers(alabi_ens* e, bool third = false, bool whole_half = false) {
    const size_t n = (size_t)e->chunk_cap * e->W * e->E;
    hipError_t err = hipSuccess;
    if (!e->mv.cw2) {
        err = hipMalloc(&e->mv.cw2, n * sizeof(int));
        if (err == hipSuccess) err = hipMalloc(&e->mv.partner2, n * sizeof(int));
        if (err == hipSuccess) err = hipMalloc(&e->mv.move, (size_t)e->chunk_cap * e->E * sizeof(int));
    }
    if (third && !e->mv.cw3 && err == hipSuccess) {
        err = hipMalloc(&e->mv.cw3, n * sizeof(int));
        if (err == hipSuccess) err = hipMalloc(&e->mv.partner3, n * sizeof(int));
    }
    if (whole_half && !e->mv.kind && err == hipSuccess) {
        err = hipMalloc(&e->mv.kind, (size_t)e->chunk_cap * e->E * sizeof(int));
        if (err == hipSuccess) err = hipMalloc(&e->mv.par, (size_t)e->chunk_cap * e->E * 2 * sizeof(double));
    }
    if (err != hipSuccess) { free_move_buffers(e->mv); return hip_fail(err, "hipMalloc(move buffers)", __FILE__, __LINE__); }
    return ALABI_OK;
}

// What the KDE pre-pass leaves for the half-step kernels: whitened rows of the larger half, factor, mean, flag and the counter.
static int ensure_kde_buffers(alabi_ens* e) {
    if (e->kde.white) return ALABI_OK;
    const size_t E = (size_t)e->E, d = (size_t)e->d, ncmax = (size_t)(e->W + 1) / 2;
    hipError_t err = hipMalloc(&e->kde.white, E * ncmax * d * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&e->kde.L, E * d * d * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&e->kde.mean, E * d * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&e->kde.flag, E * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&e->kde.singular, sizeof(unsigned long long));
    if (err == hipSuccess) err = hipMemset(e->kde.flag, 0, E * sizeof(int));
    if (err == hipSuccess) err = hipMemset(e->kde.singular, 0, sizeof(unsigned long long));
    if (err != hipSuccess) { free_kde_buffers(e->kde); return hip_fail(err, "hipMalloc(KDE buffers)", __FILE__, __LINE__); }
    return ALABI_OK;
}

// The further-partner arrays and, for a set with a walk or KDE move, the step's kind and the pre-pass buffers, offset to local step t
static void set_move_args(const alabi_ens* e, HalfArgs& h, size_t t) {
    const size_t WT = (size_t)e->W * e->E;
    h.cw2 = e->has_de ? e->mv.cw2 + t * WT : nullptr;
    h.cw3 = (e->has_snooker || e->has_wk) ? e->mv.cw3 + t * WT : nullptr;
    h.mvkind = e->has_wk ? e->mv.kind + t * e->E : nullptr;
    h.mvpar = e->has_wk ? e->mv.par + 2 * t * e->E : nullptr;
    h.kde = e->kde;
    h.seed = e->seed;
    h.mvidx = e->has_gauss ? e->mv.move + t * e->E : nullptr;
    h.gauss_C = e->has_gauss ? e->gauss_C : nullptr;
    h.gauss_diag = e->gauss_diag;
}

static DrawBuffers offset_draws(const DrawBuffers& b, size_t off) {
    DrawBuffers r = b;
    r.order += off; r.cw += off; r.zz += off; r.lnfac += off; r.lnu += off;
    r.partner += off; r.u_z += off; r.u_acc += off; r.packed += 4 * off; r.pos_of += off; r.link += 2 * off;
    if (r.packed_x) r.packed_x += 4 * off;
    if (r.place) r.place += off;
    return r;
}

// alabi_ens_create and alabi_ens_create_metropolis: the same handle, they differ in the fewest walkers they take (min_w)
static int ens_create(alabi_gp* gp, int W, int min_w, int d, int n_ensembles, const double* bounds, unsigned long long seed, alabi_ens** out) {
    if (!gp || !out || !bounds || W < min_w || W > 8192 || d != gp->d || n_ensembles < 1 || n_ensembles > 4096)
        return ALABI_BAD_ARGUMENT;
    if ((long long)W * n_ensembles > (1LL << 22)) return ALABI_BAD_ARGUMENT;
    alabi_ens* e = new (std::nothrow) alabi_ens();
    if (!e) return ALABI_BAD_ARGUMENT;
    e->gp = gp; e->W = W; e->d = d; e->E = n_ensembles; e->seed = seed;
    { static std::atomic<long long> next_serial{0}; e->serial = ++next_serial; }
    for (int k = 0; k < ALABI_MAX_DIM; ++k) {
        e->lo[k] = (k < d) ? bounds[2 * k] : 0.0;
        e->hi[k] = (k < d) ? bounds[2 * k + 1] : 0.0;
    }
    // 256 compute lanes (up to 4 point pairs each) cover Npad <= 2048: few, fat waves keep the per-wave overhead of a
    // proposal (broadcast, DPP reduction) small -- measured 2.00 us per half step against 2.11 us with 512 lanes.
    // Larger training sets run on the launch-per-half-step path with 512-lane workgroups (room for several proposals per
    // workgroup in ens_half_multi_kernel).
    e->threads = (gp->Npad / 2 <= 1024) ? 256 : 512;
    if (const char* env = getenv("ALABI_ENS_THREADS")) {
        int v = atoi(env);
        if (v == 64 || v == 128 || v == 256 || v == 512 || v == 1024) e->threads = v;
    }
    const long long WT = (long long)W * n_ensembles;
    long long cap = (4LL << 20) / WT;
    if (cap > 1024) cap = 1024;
    if (cap < 16) cap = 16;
    if (const char* env = getenv("ALABI_ENS_CHUNK")) {      // a shorter chunk (tests of the chunk boundary at few steps)
        const long long v = atoll(env);
        if (v >= 2 && v < cap) cap = v;
    }
    e->chunk_cap = (int)cap;
    const size_t n = (size_t)e->chunk_cap * WT;
    DrawBuffers& b = e->draws;
    hipError_t err = alloc_draws(b, n);
    if (err == hipSuccess) err = hipMalloc(&e->run_state, 4 * sizeof(long long));
    if (err == hipSuccess) err = hipMalloc(&e->consts, 5 * ALABI_MAX_DIM * sizeof(double));
    // persistent dataflow path: one workgroup per list position, all co-resident (at most one per CU)
    {
        int dev = 0, n_cu = 0;
        const char* env = getenv("ALABI_ENS_STREAM");
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
            n_ensembles <= n_cu && !(env && env[0] == '0')) {
            // at most one workgroup per CU: G positions-in-flight per ensemble, each workgroup strides over the list
            int G = n_cu / n_ensembles;
            if (G > (W + 1) / 2) G = (W + 1) / 2;
            e->stream_grid = G;
            const size_t hist_words = ((size_t)e->chunk_cap + 1) * WT * (d + 2);   // row = coords, logp, accepted
            const size_t state_words = 1 + (size_t)WT * (d + 1);                   // err | coords | logp
            if (err == hipSuccess) err = hipMalloc(&e->hist, hist_words * sizeof(unsigned long long));
            if (err == hipSuccess) err = hipMalloc(&e->state_dev, state_words * sizeof(unsigned long long));
            if (err == hipSuccess) err = hipMemset(e->state_dev, 0, state_words * sizeof(unsigned long long));
            if (err == hipSuccess) err = hipHostMalloc(reinterpret_cast<void**>(&e->state_host), state_words * sizeof(unsigned long long), hipHostMallocDefault);
            if (err == hipSuccess) err = hipMalloc(&e->save, (size_t)WT * (d + 1) * sizeof(double) + (size_t)WT * sizeof(long long));
            if (err == hipSuccess) e->err = reinterpret_cast<int*>(e->state_dev);
            e->stream_ok = (err == hipSuccess) ? 1 : 0;
        }
    }
    if (err != hipSuccess) {
        alabi_ens_destroy(e);
        return hip_fail(err, "hipMalloc(ensemble buffers)", __FILE__, __LINE__);
    }
    *out = e;
    return ALABI_OK;
}

int alabi_ens_create(alabi_gp* gp, int W, int d, int n_ensembles, const double* bounds, unsigned long long seed,
                     alabi_ens** out) {
    return ens_create(gp, W, 2, d, n_ensembles, bounds, seed, out);
}

// A handle for Metropolis sets: one walker is enough.  With W < 2 every entry that would draw a red-blue record refuses a table
// that is not all Gaussian (alabi_ens_set_moves, alabi_ens_run, alabi_ens_draw).
int alabi_ens_create_metropolis(alabi_gp* gp, int W, int d, int n_ensembles, const double* bounds, unsigned long long seed,
                                alabi_ens** out) {
    return ens_create(gp, W, 1, d, n_ensembles, bounds, seed, out);
}

int alabi_ens_destroy(alabi_ens* e) {
    if (!e) return ALABI_OK;
    if (e->graph_exec) (void)hipGraphExecDestroy(e->graph_exec);
    if (e->side_stream) (void)hipStreamSynchronize(e->side_stream);   // draws made ahead for a call that never came
    free_draws(e->draws);
    free_draws(e->draws2);
    free_move_buffers(e->mv);
    free_kde_buffers(e->kde);
    if (e->gauss_C) (void)hipFree(e->gauss_C);
    if (e->side_stream) (void)hipStreamDestroy(e->side_stream);
    if (e->ev_free) (void)hipEventDestroy(e->ev_free);
    if (e->ev_drawn) (void)hipEventDestroy(e->ev_drawn);
    if (e->run_state) (void)hipFree(e->run_state);
    if (e->consts) (void)hipFree(e->consts);
    if (e->hist) (void)hipFree(e->hist);
    if (e->part) (void)hipFree(e->part);
    if (e->cand) (void)hipFree(e->cand);
    if (e->state_dev) (void)hipFree(e->state_dev);       // e->err is its first word
    if (e->state_host) (void)hipHostFree(e->state_host);
    if (e->save) (void)hipFree(e->save);
    ens_pair_release(e);
    delete e;
    return ALABI_OK;
}

int alabi_ens_set_normal_prior(alabi_ens* e, const double* mean, const double* std) {
    if (!e || !mean || !std) return ALABI_BAD_ARGUMENT;
    e->has_prior = 0; e->prior_const = 0.0;
    for (int k = 0; k < ALABI_MAX_DIM; ++k) { e->prior_mean[k] = 0.0; e->prior_istd[k] = 0.0; }
    for (int k = 0; k < e->d; ++k) {
        if (std::isfinite(mean[k]) && std::isfinite(std[k]) && std[k] > 0.0) {
            e->prior_mean[k] = mean[k];
            e->prior_istd[k] = 1.0 / std[k];
            e->prior_const += -std::log(std[k]) - 0.9189385332046727;   // -log(std) - log(2 pi) / 2, as norm.logpdf
            e->has_prior = 1;
        }
    }
    e->consts_gen = -1;                                                  // re-upload
    e->settings_gen++;
    if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }
    return ALABI_OK;
}

int alabi_ens_set_logp_affine(alabi_ens* e, double scale, double shift) {
    if (!e || !(scale > 0.0) || !std::isfinite(scale) || !std::isfinite(shift)) return ALABI_BAD_ARGUMENT;
    e->lp_scale = scale; e->lp_shift = shift;
    e->settings_gen++;
    if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }   // captured launches carry the old values
    return ALABI_OK;
}

int alabi_ens_set_logp_map(alabi_ens* e, int kind) {
    if (!e || kind < 0 || kind > 2) return ALABI_BAD_ARGUMENT;
    e->ymap = kind;
    e->settings_gen++;
    if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }   // captured launches carry the old value
    return ALABI_OK;
}

int alabi_ens_set_moves(alabi_ens* e, int n, const int* kind, const double* cum, const double* p0, const double* p1) {
    if (!e || n < 0 || n > ALABI_MAX_MOVES || (n > 0 && (!kind || !cum || !p0 || !p1))) return ALABI_BAD_ARGUMENT;
    MoveTable mt{};
    bool de = false, snooker = false, walk = false, kde = false, gauss = false, all_gauss = n > 0, hmc = false, all_hmc = n > 0;
    const int nc_min = e->W / 2, nc_max = (e->W + 1) / 2;   // the two complementary halves
    double prev = 0.0;
    for (int k = 0; k < n; ++k) {
        if (!(cum[k] >= prev) || !std::isfinite(cum[k])) return ALABI_BAD_ARGUMENT;   // cumulative weights do not decrease
        prev = cum[k];
        if (kind[k] == 0) { if (!(p0[k] > 1.0) || !std::isfinite(p0[k])) return ALABI_BAD_ARGUMENT; }          // stretch: a > 1
        else if (kind[k] == 1) { if (!std::isfinite(p0[k]) || !std::isfinite(p1[k])) return ALABI_BAD_ARGUMENT; de = true; }
        else if (kind[k] == 2) { if (!std::isfinite(p0[k])) return ALABI_BAD_ARGUMENT; snooker = true; }                // snooker: gammas
        else if (kind[k] == 3) {                             // walk: p0 = s0 (0: the whole half), 2 <= s0 <= the smaller half
            const double s0 = p0[k] == 0.0 ? (double)nc_min : p0[k];
            if (!(s0 >= 2.0) || !(s0 <= (double)nc_min) || s0 != std::floor(s0) || nc_max > 2048) return ALABI_BAD_ARGUMENT;
            walk = true;
        } else if (kind[k] == 4) {                           // KDE: the bandwidth factors of the two splits; more rows than dimensions
            if (!(p0[k] > 0.0) || !std::isfinite(p0[k]) || !(p1[k] > 0.0) || !std::isfinite(p1[k]) || nc_min < e->d + 1) return ALABI_BAD_ARGUMENT;
            kde = true;
        } else if (kind[k] == 5) {                           // Gaussian: p0 = ln factor >= 0 (0: none), p1 = mode 0 / 1 / 2
            if (!(p0[k] >= 0.0) || !std::isfinite(p0[k]) || !(p1[k] == 0.0 || p1[k] == 1.0 || p1[k] == 2.0)) return ALABI_BAD_ARGUMENT;
            // its scale factor has been handed over for this slot (alabi_ens_set_move_scale), diagonal where one coordinate moves
            if (!((e->gauss_staged >> k) & 1) || (p1[k] != 0.0 && !((e->gauss_diag >> k) & 1))) return ALABI_BAD_ARGUMENT;
            gauss = true;
        } else if (kind[k] == 6) {                           // HMC: p0 = step size > 0, p1 = n_leapfrog (1 ... 64) + ln jitter / 512
            if (!(p0[k] > 0.0) || !std::isfinite(p0[k]) || !std::isfinite(p1[k]) || !(p1[k] >= 1.0) || !(p1[k] < 65.0)) return ALABI_BAD_ARGUMENT;
            if (!((e->gauss_staged >> k) & 1)) return ALABI_BAD_ARGUMENT;   // its scale factor has been handed over for this slot
            hmc = true;
        }
        else return ALABI_BAD_ARGUMENT;
        if (kind[k] != 5) all_gauss = false;
        if (kind[k] != 6) all_hmc = false;
        mt.kind[k] = kind[k]; mt.cum[k] = cum[k]; mt.p0[k] = p0[k]; mt.p1[k] = p1[k];
    }
    if (n > 0 && !(prev > 0.0)) return ALABI_BAD_ARGUMENT;
    if (hmc && !all_hmc) return ALABI_BAD_ARGUMENT;      // an HMC move runs on ens_hmc_kernel alone: no mixture with another kind
    if (e->W < 2 && !all_gauss && !all_hmc) return ALABI_BAD_ARGUMENT;   // a red-blue move needs a complementary half
    if (de && e->W < 4) return ALABI_BAD_ARGUMENT;       // two distinct partners in a complementary list of W / 2 walkers
    if (snooker && e->W < 6) return ALABI_BAD_ARGUMENT;  // three distinct partners
    if (n > 0 && !hmc) { const int st = ensure_move_buffers(e, snooker || walk || kde || gauss, walk || kde || gauss); if (st != ALABI_OK) return st; }
    if (kde) { const int st = ensure_kde_buffers(e); if (st != ALABI_OK) return st; }
    mt.n = n;
    e->moves = mt;
    e->has_de = de || snooker || walk || kde || gauss;   // more than one partner row, or none: one launch per half step
    e->has_snooker = snooker;
    e->has_wk = walk || kde || gauss;                    // proposals formed where they are used: the whole-half instantiations
    e->has_kde = kde;
    e->has_gauss = gauss; e->all_gauss = gauss && all_gauss;
    e->all_hmc = hmc && all_hmc;
    e->gauss_staged = 0;                                 // scale factors belong to the table they were handed over for
    e->drawn_n = 0;                                      // records drawn under the old move set are not the new set's
    e->ahead_valid = false;                              // nor are those made ahead for the next stream call
    e->moves_gen++;
    e->settings_gen++;
    if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }   // captured draw launches carry the old table
    return ALABI_OK;
}

int alabi_ens_set_move_scale(alabi_ens* e, int k, const double* C, int diagonal) {
    if (!e || !C || k < 0 || k >= ALABI_MAX_MOVES) return ALABI_BAD_ARGUMENT;
    const int d = e->d;
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
            const double v = C[(size_t)i * d + j];
            if (!std::isfinite(v) || (j > i && v != 0.0) || (diagonal && j != i && v != 0.0) || (j == i && !(v > 0.0))) return ALABI_BAD_ARGUMENT;
        }
    // slot k of the current table is in use by a Gaussian move that moves one coordinate per step: a diagonal factor, as in emcee
    if (k < e->moves.n && e->moves.kind[k] == 5 && e->moves.p1[k] != 0.0 && !diagonal) return ALABI_BAD_ARGUMENT;
    if (!e->gauss_C) {
        hipError_t err = hipMalloc(&e->gauss_C, (size_t)ALABI_MAX_MOVES * ALABI_MAX_DIM * ALABI_MAX_DIM * sizeof(double));
        if (err != hipSuccess) { e->gauss_C = nullptr; return hip_fail(err, "hipMalloc(move scale factors)", __FILE__, __LINE__); }
    }
    ALABI_HIP_CHECK(hipDeviceSynchronize());               // nothing in flight reads the old factor
    ALABI_HIP_CHECK(hipMemcpy(e->gauss_C + (size_t)k * d * d, C, (size_t)d * d * sizeof(double), hipMemcpyHostToDevice));
    e->gauss_staged |= 1 << k;
    if (diagonal) e->gauss_diag |= 1 << k; else e->gauss_diag &= ~(1 << k);
    e->settings_gen++;
    if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }   // captured launches carry gauss_diag
    return ALABI_OK;
}

int alabi_ens_mh_plan(alabi_ens* e, int* out) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    for (int i = 0; i < 4; ++i) out[i] = e->mh_plan[i];
    return ALABI_OK;
}

int alabi_ens_set_stream(alabi_ens* e, int enabled) {
    if (!e) return ALABI_BAD_ARGUMENT;
    // The switch belongs to the handle, not to the move table: it covers the persistent kernels of a red-blue table (they need
    // the version history) and ens_mh_kernel of an all-Gaussian one (it needs nothing), whichever table the next run finds.
    const bool can_stream = e->hist && e->err;
    if (enabled && !can_stream && !e->all_gauss && !e->all_hmc) return ALABI_BAD_ARGUMENT;
    e->mh_ok = enabled ? 1 : 0;
    e->stream_ok = (enabled && can_stream) ? 1 : 0;
    e->settings_gen++;
    return ALABI_OK;
}

int alabi_ens_stream_variant(alabi_ens* e, int* variant) {
    if (!e || !variant) return ALABI_BAD_ARGUMENT;
    *variant = (e->last_path == 1) ? e->last_variant : 0;
    return ALABI_OK;
}

// The pair kernel's debug counters (alabi_ens::pair_stats); counting starts with the next run
static int pair_stats_alloc(alabi_ens* e) {
    if (e->pair_stats) return ALABI_OK;
    ALABI_HIP_CHECK(hipMalloc(&e->pair_stats, ALABI_PAIR_STATS_WORDS * sizeof(unsigned long long)));
    ALABI_HIP_CHECK(hipMemset(e->pair_stats, 0, ALABI_PAIR_STATS_WORDS * sizeof(unsigned long long)));
    return ALABI_OK;
}

int alabi_ens_pair_stats(alabi_ens* e, long long* out, int reset) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    int st;
    if ((st = pair_stats_alloc(e)) != ALABI_OK) return st;
    ALABI_HIP_CHECK(hipDeviceSynchronize());
    ALABI_HIP_CHECK(hipMemcpy(out, e->pair_stats, 9 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (reset) ALABI_HIP_CHECK(hipMemset(e->pair_stats, 0, 9 * sizeof(unsigned long long)));
    return ALABI_OK;
}

int alabi_ens_place_stats(alabi_ens* e, long long* out, int reset) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    out[0] = e->place_state > 0; out[1] = out[2] = 0;
    if (!e->place_stats) return ALABI_OK;
    ALABI_HIP_CHECK(hipDeviceSynchronize());
    ALABI_HIP_CHECK(hipMemcpy(out + 1, e->place_stats, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (reset) ALABI_HIP_CHECK(hipMemset(e->place_stats, 0, 2 * sizeof(unsigned long long)));
    return ALABI_OK;
}

int alabi_ens_export_placement(alabi_ens* e, long long step0, int nsteps, double a, int* place, unsigned long long* packed,
                               unsigned long long* packed_x, void* stream) {
    if (!e || !place || nsteps <= 0 || nsteps > e->chunk_cap || !(a > 1.0)) return ALABI_BAD_ARGUMENT;
    if (e->place_state <= 0) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = launch_ens_draw_at(e, e->draws, nsteps, a, false, step0, s)) != ALABI_OK) return st;
    if ((st = launch_ens_place(e, e->draws, nsteps, false, s)) != ALABI_OK) return st;
    e->drawn_n = 0;                                   // (the buffers no longer hold what alabi_ens_draw put there)
    const size_t n = (size_t)nsteps * e->W * e->E;
    ALABI_HIP_CHECK(hipMemcpyAsync(place, e->draws.place, n * sizeof(int), hipMemcpyDeviceToDevice, s));
    if (packed) ALABI_HIP_CHECK(hipMemcpyAsync(packed, e->draws.packed, 4 * n * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    if (packed_x) ALABI_HIP_CHECK(hipMemcpyAsync(packed_x, e->draws.packed_x, 4 * n * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    return ALABI_OK;
}

int alabi_ens_pair_stats2(alabi_ens* e, long long* out, int enable) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    int st;
    if (enable && (st = pair_stats_alloc(e)) != ALABI_OK) return st;
    for (int i = 0; i < 6; ++i) out[i] = 0;
    if (!e->pair_stats) return ALABI_OK;
    ALABI_HIP_CHECK(hipDeviceSynchronize());
    ALABI_HIP_CHECK(hipMemcpy(out, e->pair_stats + 9, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    ALABI_HIP_CHECK(hipMemset(e->pair_stats + 9, 0, 6 * sizeof(unsigned long long)));
    return ALABI_OK;
}

int alabi_ens_pair_stats3(alabi_ens* e, long long* out, int enable) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    int st;
    if (enable && (st = pair_stats_alloc(e)) != ALABI_OK) return st;
    for (int i = 0; i < 20; ++i) out[i] = 0;
    if (!e->pair_stats) return ALABI_OK;
    ALABI_HIP_CHECK(hipDeviceSynchronize());
    long long raw[20];                                // per role, by lane of the kernel's counter: [0] verdict looks, [2..4] verdict bins,
                                                      // [5] input looks, [6] inputs complete without a reload, [7..9] input bins
    ALABI_HIP_CHECK(hipMemcpy(raw, e->pair_stats + 16, 20 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int r = 0; r < 2; ++r) {
        const long long* q = raw + 10 * r;
        long long* o = out + 10 * r;
        o[0] = q[2] + q[3] + q[4]; o[1] = q[0]; o[2] = q[2]; o[3] = q[3]; o[4] = q[4];
        o[5] = q[7] + q[8] + q[9]; o[6] = q[5]; o[7] = q[7]; o[8] = q[8]; o[9] = q[9];
    }
    ALABI_HIP_CHECK(hipMemset(e->pair_stats + 16, 0, 20 * sizeof(unsigned long long)));
    return ALABI_OK;
}

int alabi_ens_last_path(alabi_ens* e, int* path) {
    if (!e || !path) return ALABI_BAD_ARGUMENT;
    *path = e->last_path;
    return ALABI_OK;
}

int alabi_ens_group_plan(alabi_ens* e, int* out) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    for (int i = 0; i < 8; ++i) out[i] = e->group_plan[i];
    return ALABI_OK;
}

// (inv_len, lo, hi) live in device memory; refreshed whenever the GP's hyper-parameters changed.
static int sync_consts(alabi_ens* e, hipStream_t s) {
    // squared exponential: the half-step kernels read the centred inputs and h = |x - c|^2 / 2 - ln|alpha| (ens_se_prepare; per GP,
    // rebuilt when the inputs, y or the hyper-parameters moved) -- here, i.e. before any stream capture
    if (e->gp->kf.type == 0 && e->gp->has_alpha) { const int st = ens_se_prepare(e->gp, s); if (st != ALABI_OK) return st; }
    if (e->consts_gen == e->gp->gen) return ALABI_OK;
    double host[5 * ALABI_MAX_DIM];
    for (int k = 0; k < ALABI_MAX_DIM; ++k) {
        host[k] = e->gp->inv_len.v[k];
        host[ALABI_MAX_DIM + k] = e->lo[k];
        host[2 * ALABI_MAX_DIM + k] = e->hi[k];
        host[3 * ALABI_MAX_DIM + k] = e->prior_mean[k];
        host[4 * ALABI_MAX_DIM + k] = e->prior_istd[k];
    }
    ALABI_HIP_CHECK(hipMemcpyAsync(e->consts, host, sizeof(host), hipMemcpyHostToDevice, s));
    ALABI_HIP_CHECK(hipStreamSynchronize(s));  // `host` is a stack buffer
    e->consts_gen = e->gp->gen;
    return ALABI_OK;
}

int alabi_ens_lnprob(alabi_ens* e, const double* coords, double* logp, void* stream) {
    if (!e || !coords || !logp) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    int st = sync_consts(e, as_stream(stream));
    if (st != ALABI_OK) return st;
    return launch_ens_lnprob(e, coords, e->W * e->E, logp, 1, as_stream(stream));
}

int alabi_ens_surrogate(alabi_ens* e, const double* points, int M, double* like, void* stream) {
    if (!e || !points || !like || M < 0) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    if (M == 0) return ALABI_OK;
    int st = sync_consts(e, as_stream(stream));
    if (st != ALABI_OK) return st;
    // the normal-prior rows are part of the fused log-probability, not of the surrogate: evaluate without them
    const int hp = e->has_prior; const double pc = e->prior_const;
    e->has_prior = 0; e->prior_const = 0.0;
    st = launch_ens_lnprob(e, points, M, like, 0, as_stream(stream));
    e->has_prior = hp; e->prior_const = pc;
    return st;
}

static HalfArgs base_args(alabi_ens* e, double* coords, double* logp) {
    HalfArgs h{};
    alabi_gp* gp = e->gp;
    h.coords = coords; h.logp = logp; h.consts = e->consts;
    h.Xt = gp->Xt; h.alpha = gp->alpha; h.Npad = gp->Npad;
    h.Xc = gp->Xc; h.ens_h = gp->ens_h; h.centre = gp->xa_centre;
    // the affine map of the log-probability folds into the amplitude and the mean: c (amp s + m) + e = (c amp) s + (c m + e)
    h.amp = e->lp_scale * std::exp(gp->log_amp); h.mean = std::fma(e->lp_scale, gp->mean, e->lp_shift); h.kf = gp->kf;
    h.W = e->W; h.d = e->d; h.n0 = (e->W + 1) / 2;
    h.thin_by = 1; h.run_state = e->run_state;
    h.has_prior = e->has_prior; h.prior_const = e->prior_const; h.ymap = e->ymap;
    return h;
}

static int set_run_state(alabi_ens* e, long long step0, long long done, hipStream_t s) {
    long long host[2] = {step0, done};
    ALABI_HIP_CHECK(hipMemcpyAsync(e->run_state, host, sizeof(host), hipMemcpyHostToDevice, s));
    ALABI_HIP_CHECK(hipStreamSynchronize(s));  // `host` is a stack buffer
    return ALABI_OK;
}

// enqueue `n` steps that consume the chunk buffers (draw + 2n half steps + advance)
static int enqueue_chunk(alabi_ens* e, HalfArgs h, int n, double a, hipStream_t s) {
    int st;
    if ((st = launch_ens_draw(e, n, a, s)) != ALABI_OK) return st;
    const int n0 = h.n0, n1 = e->W - n0;
    const size_t WT = (size_t)e->W * e->E;
    for (int t = 0; t < n; ++t) {
        h.rec = offset_draws(e->draws, (size_t)t * WT);
        set_move_args(e, h, (size_t)t);
        h.local_t = t; h.part_begin = 0;
        h.split = 0;
        if (e->has_kde && (st = launch_ens_kde_prepass(e, h, s)) != ALABI_OK) return st;
        if ((st = launch_ens_half_args(e, h, n0, s)) != ALABI_OK) return st;
        h.split = 1;
        if (e->has_kde && n1 > 0 && (st = launch_ens_kde_prepass(e, h, s)) != ALABI_OK) return st;
        if ((st = launch_ens_half_args(e, h, n1, s)) != ALABI_OK) return st;
    }
    return launch_ens_advance(e, n, s);
}

// (coords, logp, n_accept) <- what ens_call_prologue_kernel saved at the start of the last persistent call
static int ens_restore(alabi_ens* e, double* coords, double* logp, long long* n_accept, hipStream_t s) {
    if (!e->save || !e->save_valid) return ALABI_NOT_COMPUTED;
    const size_t WT = (size_t)e->W * e->E;
    const double* sv = e->save;
    ALABI_HIP_CHECK(hipMemcpyAsync(coords, sv, WT * e->d * sizeof(double), hipMemcpyDeviceToDevice, s));
    ALABI_HIP_CHECK(hipMemcpyAsync(logp, sv + WT * e->d, WT * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (n_accept && e->save_accept)
        ALABI_HIP_CHECK(hipMemcpyAsync(n_accept, sv + WT * (e->d + 1), WT * sizeof(long long), hipMemcpyDeviceToDevice, s));
    return ALABI_OK;
}

int alabi_ens_restore(alabi_ens* e, double* coords, double* logp, long long* n_accept, void* stream) {
    if (!e || !coords || !logp) return ALABI_BAD_ARGUMENT;
    return ens_restore(e, coords, logp, n_accept, as_stream(stream));
}

int alabi_ens_last_state(alabi_ens* e, double* coords_out, double* logp_out) {
    if (!e || !coords_out || !logp_out) return ALABI_BAD_ARGUMENT;
    if (!e->last_state_ok || !e->state_host) return ALABI_NOT_COMPUTED;
    const size_t WT = (size_t)e->W * e->E;
    memcpy(coords_out, e->state_host + 1, WT * e->d * sizeof(double));
    memcpy(logp_out, e->state_host + 1 + WT * e->d, WT * sizeof(double));
    return ALABI_OK;
}

int alabi_ens_boundary_stats(alabi_ens* e, long long* out) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    for (int i = 0; i < 4; ++i) out[i] = e->boundary_stats[i];
    return ALABI_OK;
}

int alabi_ens_run(alabi_ens* e, double* coords, double* logp, long long step0, long long nsteps, int thin_by,
                  double a, double* chain, double* chain_logp, long long* n_accept, void* stream) {
    if (!e || !coords || !logp || nsteps < 0 || thin_by < 1 || !(a > 1.0)) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    if (nsteps == 0) return ALABI_OK;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = sync_consts(e, s)) != ALABI_OK) return st;
    // An all-HMC set: ens_hmc_kernel or nothing -- there is no launch-per-half-step form, and alabi_ens_set_stream does not apply.
    if (e->all_hmc) {
        const int chunk = ens_hmc_chunk(e);
        if (chunk <= 0) return ALABI_BAD_ARGUMENT;                    // the factors and weights exceed the LDS, or no dimension bucket
        e->last_path = 5;
        e->last_state_ok = false;
        for (long long done = 0; done < nsteps; done += chunk) {
            const int K = (int)(nsteps - done < chunk ? nsteps - done : chunk);
            if ((st = launch_ens_hmc(e, coords, logp, step0, done, K, thin_by, chain, chain_logp, n_accept, 0, 0.0, nullptr, nullptr, s)) != ALABI_OK) return st;
        }
        e->hmc_plan[1] = chunk;
        return ALABI_OK;
    }
    if (e->W < 2 && !e->all_gauss) return ALABI_BAD_ARGUMENT;         // a red-blue move needs a complementary half
    // An all-Gaussian set: W independent chains, one workgroup per walker, every step of a chunk in one launch (ens_mh_kernel).
    // The step counters travel by value; nothing is read back.
    if (e->all_gauss && e->mh_ok) {
        const int chunk = ens_mh_chunk(e);
        if (chunk > 0) {
            e->last_path = 4;
            e->last_state_ok = false;
            for (long long done = 0; done < nsteps; done += chunk) {
                const int K = (int)(nsteps - done < chunk ? nsteps - done : chunk);
                if ((st = launch_ens_mh(e, coords, logp, step0, done, K, thin_by, chain, chain_logp, n_accept, s)) != ALABI_OK) return st;
            }
            e->mh_plan[1] = chunk;
            return ALABI_OK;
        }
    }
    // Persistent dataflow path: training set pinned in registers (Npad <= 2048: 256 compute lanes x up to 4 point pairs), one
    // workgroup per list position.  It synchronises at the end to read the time-out flag.
    e->last_path = 0;
    e->last_state_ok = false;
    // Which persistent kernel: ens_stream_kernel where the training set fits one workgroup's registers (N <= 2048, small d),
    // ens_group_kernel (training set partitioned over groups of workgroups, matrix-core kernel sums) beyond that;
    // ALABI_ENS_GROUP=0 disables the latter, =1 prefers it wherever its blocking is feasible.
    const char* genv = getenv("ALABI_ENS_GROUP");
    const bool group_off = genv && genv[0] == '0', group_pref = genv && genv[0] == '1';
    const bool can_stream = ens_stream_fits(e);
    // ens_stream_kernel takes ceil(W/2 / stream_grid) proposals per workgroup one after the other (2.0 / 3.7 / 7.1 us per half step at
    // 1 / 2 / 4 of them, N = 2000); from four on the group kernel is ahead (5.3 us at W = 2048: 1.9e8 against 1.4e8 samples/s)
    const bool crowded = can_stream && e->stream_grid > 0 && ((e->W + 1) / 2 + e->stream_grid - 1) / e->stream_grid >= 4;
    const bool use_group = !e->has_de && e->stream_ok && s != nullptr && !group_off && (group_pref || !can_stream || crowded) && ens_group_fits(e) &&
                           ens_group_buffers(e, s);
    // A differential-evolution record reads two partner rows, a snooker record three: the persistent kernels hand one over, so
    // such a move set (has_de) runs with one launch per half step (and its graph replay).  Stretch-only sets differ in the draw kernel alone.
    if (!e->has_de && e->stream_ok && s != nullptr && (can_stream || use_group)) {
        e->last_path = use_group ? 3 : 1;
        // ens_stream_kernel's chunks take the step counters by value and their epilogue leaves run_state as the other paths
        // would (no upload, no host synchronisation in front of the first launch); the history is trusted to hold the
        // sentinel only when this handle's last use of it was a stream call that ended without a time-out
        const int need = (int)(nsteps < e->chunk_cap ? nsteps : e->chunk_cap);   // rows 1..need are polled by this call
        const int clean_rows = e->hist_clean;
        e->hist_clean = 0;
        // Two workgroups per list position (ens_pair_kernel) where 2 ceil(W/2) E of them fit one per CU.  That leaves no spare CU, so
        // a time-out of the pair variant is retried below on ens_stream_kernel, from the walkers saved here, before it is reported.
        const bool use_pair = !use_group && can_stream && ens_pair_ready(e);
        e->last_variant = use_pair ? 1 : 0;
        const int prop_clean_rows = use_pair ? e->prop_clean : 0;
        if (use_pair) e->prop_clean = 0;
        if (use_group && (st = set_run_state(e, step0, 0, s)) != ALABI_OK) return st;
        // The draws depend on nothing but the step counter.  In a call of several chunks those of the next chunk are made on the
        // side stream while this chunk's persistent kernel runs (it occupies half of the CUs), into the buffer set the previous
        // chunk has released; behind the call's last persistent kernel the same is done for the first chunk of the NEXT call,
        // which by then finds them in draws2 if it continues where this one ends (step, a, move table).
        const bool two_sets = !use_group && ens_draw_ahead_ready(e);
        // Pair kernel: every chunk's records go through ens_place_kernel right behind their draws, on the stream that drew them.
        // A time-out's second run is on ens_stream_kernel and reads the records as they were drawn.
        const bool place = use_pair && ens_place_ready(e);
        bool ahead_issued = false;
        if (!use_group) {
            const bool hit = two_sets && e->ahead_valid && e->ahead_step == step0 && e->ahead_a == a && e->ahead_moves_gen == e->moves_gen &&
                             need <= e->ahead_n;
            // hit or not, the main stream goes on behind the pending launch of the side stream: draws2 is never written from two streams
            if (e->ahead_pending) ALABI_HIP_CHECK(hipStreamWaitEvent(s, e->ev_drawn, 0));
            e->ahead_pending = false; e->ahead_valid = false;
            e->draw_set = hit ? 1 : 0;
            e->boundary_stats[hit ? 0 : 1]++;
            if (!hit && (st = launch_ens_draw_at(e, e->draws, need, a, false, step0, s)) != ALABI_OK) return st;
            if (place && !(hit && e->ahead_placed) && (st = launch_ens_place(e, hit ? e->draws2 : e->draws, need, true, s)) != ALABI_OK) return st;
        }
        // one launch: the walkers saved (a time-out is repeated from there), the flag cleared, row 0 of the history
        if ((st = launch_ens_call_prologue(e, coords, logp, n_accept, !use_group, s)) != ALABI_OK) return st;
        long long remaining = nsteps;
        while (remaining > 0) {
            const int K = (int)(remaining < e->chunk_cap ? remaining : e->chunk_cap);
            const long long done = nsteps - remaining;
            if (use_group) {
                if ((st = launch_ens_draw(e, K, a, s)) != ALABI_OK) return st;
                if ((st = launch_ens_group(e, coords, logp, K, thin_by, chain, chain_logp, n_accept, s)) != ALABI_OK) return st;
                if ((st = launch_ens_advance(e, K, s)) != ALABI_OK) return st;
            } else {
                const bool last = remaining == K;
                const bool ahead = two_sets;              // the next chunk's draws, or (last) those of the next call's first chunk
                DrawBuffers& cur = e->draw_set ? e->draws2 : e->draws;
                if (ahead_issued) ALABI_HIP_CHECK(hipStreamWaitEvent(s, e->ev_drawn, 0));
                else if (done > 0) {
                    if ((st = launch_ens_draw_at(e, cur, K, a, false, step0 + done, s)) != ALABI_OK) return st;
                    if (place && (st = launch_ens_place(e, cur, K, true, s)) != ALABI_OK) return st;
                }
                ahead_issued = false;
                // everything that read the other buffer set is behind this point.  The draws for the next call go into draws2
                // whichever set this chunk reads, and start behind its persistent kernel, not beside it
                if (ahead && !last) ALABI_HIP_CHECK(hipEventRecord(e->ev_free, s));
                const int fill_rows = (done == 0 && clean_rows < need) ? need : 0;
                const int prop_fill_rows = (done == 0 && prop_clean_rows < need) ? need : 0;
                if ((st = use_pair ? launch_ens_pair_kernel(e, cur, K, fill_rows, prop_fill_rows, place, s)
                                   : launch_ens_stream_kernel(e, cur, K, fill_rows, s)) != ALABI_OK)
                    return st;
                if (ahead && last) ALABI_HIP_CHECK(hipEventRecord(e->ev_free, s));
                if (ahead) {
                    const long long rem2 = remaining - K;
                    const int K2 = last ? e->chunk_cap : (int)(rem2 < e->chunk_cap ? rem2 : e->chunk_cap);
                    ALABI_HIP_CHECK(hipStreamWaitEvent(e->side_stream, e->ev_free, 0));
                    DrawBuffers& into = (last || e->draw_set == 0) ? e->draws2 : e->draws;
                    if ((st = launch_ens_draw_at(e, into, K2, a, false, step0 + done + K, e->side_stream)) != ALABI_OK) return st;
                    if (place && (st = launch_ens_place(e, into, K2, !last, e->side_stream)) != ALABI_OK) return st;
                    ALABI_HIP_CHECK(hipEventRecord(e->ev_drawn, e->side_stream));
                    if (last) {
                        e->ahead_pending = true; e->ahead_valid = true;
                        e->ahead_step = step0 + nsteps; e->ahead_a = a; e->ahead_moves_gen = e->moves_gen; e->ahead_n = K2;
                        e->ahead_placed = place;
                    } else {
                        ahead_issued = true;
                    }
                }
                if ((st = launch_ens_stream_epilogue(e, coords, logp, K, thin_by, chain, chain_logp, n_accept, step0 + done + K, done,
                                                     use_pair, last, s)) != ALABI_OK)
                    return st;
                if (two_sets) e->draw_set ^= 1;
            }
            remaining -= K;
        }
        // one read-back: the flag and, on ens_stream_kernel / ens_pair_kernel, the walkers the last epilogue left beside it
        const size_t WTs = (size_t)e->W * e->E;
        const size_t back = use_group ? sizeof(unsigned long long) : (1 + WTs * (e->d + 1)) * sizeof(unsigned long long);
        ALABI_HIP_CHECK(hipMemcpyAsync(e->state_host, e->state_dev, back, hipMemcpyDeviceToHost, s));
        ALABI_HIP_CHECK(hipStreamSynchronize(s));
        const int flag = *reinterpret_cast<const int*>(e->state_host);
        e->hist_clean = (!use_group && !flag) ? (clean_rows > need ? clean_rows : need) : 0;
        if (use_pair) e->prop_clean = !flag ? (prop_clean_rows > need ? prop_clean_rows : need) : 0;
        e->last_state_ok = !use_group && !flag;
        if (flag) e->ahead_valid = false;             // (the launch stays pending: the next call waits for it before it draws)
        if (flag && use_pair) {
            // restore the walkers, turn the pair variant off for this handle and run the call again on ens_stream_kernel (the history
            // is marked dirty above, the flag is cleared at the start of the call); a second time-out is reported as before
            if ((st = ens_restore(e, coords, logp, n_accept, s)) != ALABI_OK) return st;
            e->pair_state = -1;
            return alabi_ens_run(e, coords, logp, step0, nsteps, thin_by, a, chain, chain_logp, n_accept, stream);
        }
        return flag ? ALABI_TIMEOUT : ALABI_OK;
    }
    if ((st = set_run_state(e, step0, 0, s)) != ALABI_OK) return st;
    HalfArgs h = base_args(e, coords, logp);
    h.chain = chain; h.chain_logp = chain_logp; h.n_accept = n_accept; h.thin_by = thin_by;

    const char* env = getenv("ALABI_ENS_GRAPH");
    const bool want_graph = (s != nullptr) && !(env && env[0] == '0');
    int gsteps = e->chunk_cap < 256 ? e->chunk_cap : 256;
    if (const char* gs = getenv("ALABI_ENS_GRAPH_STEPS")) {
        int v = atoi(gs);
        if (v > 0 && v <= e->chunk_cap) gsteps = v;
    }
    long long remaining = nsteps;
    if (want_graph && remaining >= 2LL * gsteps) {
        alabi_ens::GraphKey key{coords, logp, chain, chain_logp, n_accept, thin_by, gsteps, a, e->gp->gen};
        const bool same = e->graph_exec && memcmp(&key, &e->graph_key, sizeof(key)) == 0;
        if (!same) {
            if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }
            hipGraph_t graph = nullptr;
            ALABI_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            st = enqueue_chunk(e, h, gsteps, a, s);
            hipError_t ce = hipStreamEndCapture(s, &graph);
            if (st != ALABI_OK) { if (graph) (void)hipGraphDestroy(graph); return st; }
            if (ce != hipSuccess) return hip_fail(ce, "hipStreamEndCapture", __FILE__, __LINE__);
            hipError_t ie = hipGraphInstantiate(&e->graph_exec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (ie != hipSuccess) { e->graph_exec = nullptr; return hip_fail(ie, "hipGraphInstantiate", __FILE__, __LINE__); }
            e->graph_key = key;
            e->graph_steps = gsteps;
        }
        while (remaining >= gsteps) {
            ALABI_HIP_CHECK(hipGraphLaunch(e->graph_exec, s));
            remaining -= gsteps;
        }
    }
    while (remaining > 0) {
        const int n = (int)(remaining < e->chunk_cap ? remaining : e->chunk_cap);
        if ((st = enqueue_chunk(e, h, n, a, s)) != ALABI_OK) return st;
        remaining -= n;
    }
    return ALABI_OK;
}

int alabi_ens_draw(alabi_ens* e, long long step0, int nsteps, double a, void* stream) {
    if (!e || nsteps <= 0 || nsteps > e->chunk_cap || !(a > 1.0)) return ALABI_BAD_ARGUMENT;
    if (e->W < 2 && !e->all_gauss) return ALABI_BAD_ARGUMENT;         // a red-blue record names a walker of the other half
    if (e->all_hmc) return ALABI_BAD_ARGUMENT;                        // an HMC step has no record: its draws are made where it runs
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = set_run_state(e, step0, 0, s)) != ALABI_OK) return st;
    e->drawn_n = nsteps;
    return launch_ens_draw(e, nsteps, a, s);
}

int alabi_ens_half_step(alabi_ens* e, double* coords, double* logp, int t, int split, int part_begin, int part_end,
                        long long* n_accept, void* stream) {
    if (!e || !coords || !logp || t < 0 || t >= e->drawn_n || (split != 0 && split != 1) || e->E != 1)
        return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    int st = sync_consts(e, as_stream(stream));
    if (st != ALABI_OK) return st;
    HalfArgs h = base_args(e, coords, logp);
    const int nS = split == 0 ? h.n0 : e->W - h.n0;
    if (part_begin < 0 || part_end > nS || part_begin > part_end) return ALABI_BAD_ARGUMENT;
    h.rec = offset_draws(e->draws, (size_t)t * e->W);
    set_move_args(e, h, (size_t)t);
    h.local_t = t; h.split = split; h.part_begin = part_begin; h.n_accept = n_accept;
    if (e->has_kde && part_end > part_begin && (st = launch_ens_kde_prepass(e, h, as_stream(stream))) != ALABI_OK) return st;
    return launch_ens_half_args(e, h, part_end - part_begin, as_stream(stream));
}

}  // extern "C" (reopened below)
namespace alabi {
int ens_sync_consts(alabi_ens* e, hipStream_t s) { return sync_consts(e, s); }
int alabi_ens_half_step_hist(alabi_ens* e, const double* coords, const double* logp, int t, int split, int part_begin, int part_end,
                             const double* shist, double* out, hipStream_t s) {
    if (!e || t < 0 || t >= e->drawn_n || e->E != 1 || !shist || !out || e->has_de) return ALABI_BAD_ARGUMENT;
    int st = sync_consts(e, s);
    if (st != ALABI_OK) return st;
    HalfArgs h = base_args(e, const_cast<double*>(coords), const_cast<double*>(logp));
    h.rec = offset_draws(e->draws, (size_t)t * e->W);
    h.local_t = t; h.split = split; h.part_begin = part_begin;
    h.shist = shist; h.sout = out;
    return launch_ens_half_args(e, h, part_end - part_begin, s);
}
}  // namespace alabi
extern "C" {

int alabi_ens_propose(alabi_ens* e, const double* coords, int t, int split, int gate_box, double* q, double* like,
                      void* stream) {
    if (!e || !coords || !q || t < 0 || t >= e->drawn_n || (split != 0 && split != 1) || e->E != 1) return ALABI_BAD_ARGUMENT;
    if (like && (!e->gp->computed || !e->gp->has_alpha)) return ALABI_NOT_COMPUTED;
    int st = sync_consts(e, as_stream(stream));
    if (st != ALABI_OK) return st;
    HalfArgs h = base_args(e, const_cast<double*>(coords), nullptr);
    const int nS = split == 0 ? h.n0 : e->W - h.n0;
    h.rec = offset_draws(e->draws, (size_t)t * e->W);
    set_move_args(e, h, (size_t)t);
    h.local_t = t; h.split = split; h.part_begin = 0;
    if (e->has_kde && nS > 0 && (st = launch_ens_kde_prepass(e, h, as_stream(stream))) != ALABI_OK) return st;
    return launch_ens_propose(e, h, nS, gate_box, q, like, as_stream(stream));
}

int alabi_ens_accept(alabi_ens* e, double* coords, double* logp, int t, int split, const double* q, const double* lp_new,
                     long long* n_accept, void* stream) {
    if (!e || !coords || !logp || !q || !lp_new || t < 0 || t >= e->drawn_n || (split != 0 && split != 1) || e->E != 1)
        return ALABI_BAD_ARGUMENT;
    HalfArgs h = base_args(e, coords, logp);
    const int nS = split == 0 ? h.n0 : e->W - h.n0;
    h.rec = offset_draws(e->draws, (size_t)t * e->W);
    h.local_t = t; h.split = split; h.part_begin = 0; h.n_accept = n_accept;
    return launch_ens_accept(e, h, nS, q, lp_new, as_stream(stream));
}

int alabi_ens_step_lists(alabi_ens* e, int t, int* order_out, int* n0, void* stream) {
    if (!e || t < 0 || t >= e->drawn_n || !order_out || !n0 || e->E != 1) return ALABI_BAD_ARGUMENT;
    ALABI_HIP_CHECK(hipMemcpyAsync(order_out, e->draws.order + (size_t)t * e->W, (size_t)e->W * sizeof(int),
                                   hipMemcpyDeviceToDevice, as_stream(stream)));
    *n0 = (e->W + 1) / 2;
    return ALABI_OK;
}

int alabi_ens_step_with_randoms(alabi_ens* e, double* coords, double* logp, const int* order, int n0,
                                const double* u_z, const int* partner, const double* u_acc, double a,
                                long long* n_accept, void* stream) {
    if (!e || !coords || !logp || !order || !u_z || !partner || !u_acc || n0 < 0 || n0 > e->W || !(a > 1.0) || e->E != 1)
        return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = sync_consts(e, s)) != ALABI_OK) return st;
    if ((st = launch_ens_prep(e, order, n0, u_z, partner, u_acc, a, s)) != ALABI_OK) return st;
    e->drawn_n = 0;  // row 0 of the draw buffers now holds caller data
    HalfArgs h = base_args(e, coords, logp);
    h.rec = e->draws; h.n0 = n0; h.n_accept = n_accept; h.local_t = 0; h.part_begin = 0;
    h.split = 0;
    if ((st = launch_ens_half_args(e, h, n0, s)) != ALABI_OK) return st;
    h.split = 1;
    return launch_ens_half_args(e, h, e->W - n0, s);
}

int alabi_ens_step_with_randoms_de(alabi_ens* e, double* coords, double* logp, const int* order, int n0, const int* j1,
                                   const int* j2, const double* gamma, const double* u_acc, long long* n_accept, void* stream) {
    if (!e || !coords || !logp || !order || !j1 || !j2 || !gamma || !u_acc || n0 < 0 || n0 > e->W || e->E != 1)
        return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = sync_consts(e, s)) != ALABI_OK) return st;
    if ((st = ensure_move_buffers(e)) != ALABI_OK) return st;
    if ((st = launch_ens_prep_de(e, order, n0, j1, j2, gamma, u_acc, s)) != ALABI_OK) return st;
    e->drawn_n = 0;  // row 0 of the draw buffers now holds caller data
    HalfArgs h = base_args(e, coords, logp);
    h.rec = e->draws; h.cw2 = e->mv.cw2; h.n0 = n0; h.n_accept = n_accept; h.local_t = 0; h.part_begin = 0;
    h.split = 0;
    if ((st = launch_ens_half_args(e, h, n0, s)) != ALABI_OK) return st;
    h.split = 1;
    return launch_ens_half_args(e, h, e->W - n0, s);
}

int alabi_ens_step_with_randoms_snooker(alabi_ens* e, double* coords, double* logp, const int* order, int n0, const int* j1,
                                        const int* j2, const int* j3, double gamma, const double* u_acc, long long* n_accept,
                                        void* stream) {
    if (!e || !coords || !logp || !order || !j1 || !j2 || !j3 || !u_acc || !std::isfinite(gamma) || n0 < 0 || n0 > e->W || e->E != 1)
        return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = sync_consts(e, s)) != ALABI_OK) return st;
    if ((st = ensure_move_buffers(e, true)) != ALABI_OK) return st;
    if ((st = launch_ens_prep_snooker(e, order, n0, j1, j2, j3, gamma, u_acc, s)) != ALABI_OK) return st;
    e->drawn_n = 0;  // row 0 of the draw buffers now holds caller data
    HalfArgs h = base_args(e, coords, logp);
    h.rec = e->draws; h.cw2 = e->mv.cw2; h.cw3 = e->mv.cw3; h.n0 = n0; h.n_accept = n_accept; h.local_t = 0; h.part_begin = 0;
    h.split = 0;
    if ((st = launch_ens_half_args(e, h, n0, s)) != ALABI_OK) return st;
    h.split = 1;
    return launch_ens_half_args(e, h, e->W - n0, s);
}

// one full step of the whole-half instantiation on row 0 of the draw buffers, from a test entry's draws
static int step_injected_wk(alabi_ens* e, double* coords, double* logp, const int* order, int n0, int kind, double p0, double p1,
                            const WkInject& inj, const double* u_acc, long long* n_accept, hipStream_t s) {
    int st;
    if ((st = sync_consts(e, s)) != ALABI_OK) return st;
    if ((st = ensure_move_buffers(e, true, true)) != ALABI_OK) return st;
    if (kind == 4 && (st = ensure_kde_buffers(e)) != ALABI_OK) return st;
    if ((st = launch_ens_prep_wk(e, order, u_acc, s)) != ALABI_OK) return st;
    if ((st = launch_ens_set_step_move(e, kind, p0, p1, s)) != ALABI_OK) return st;
    e->drawn_n = 0;  // row 0 of the draw buffers now holds caller data
    HalfArgs h = base_args(e, coords, logp);
    h.rec = e->draws; h.cw2 = e->mv.cw2; h.cw3 = e->mv.cw3; h.mvkind = e->mv.kind; h.mvpar = e->mv.par; h.kde = e->kde; h.seed = e->seed;
    h.inj = inj;
    h.n0 = n0; h.n_accept = n_accept; h.local_t = 0; h.part_begin = 0;
    for (int split = 0; split < 2; ++split) {
        const int nS = split == 0 ? n0 : e->W - n0;
        if (nS == 0) continue;
        h.split = split;
        if (kind == 4 && (st = launch_ens_kde_prepass(e, h, s)) != ALABI_OK) return st;
        if ((st = launch_ens_half_args(e, h, nS, s)) != ALABI_OK) return st;
    }
    return ALABI_OK;
}

int alabi_ens_step_with_randoms_walk(alabi_ens* e, double* coords, double* logp, const int* order, int n0, int s0, const int* subset,
                                     const double* z, const double* u_acc, long long* n_accept, void* stream) {
    if (!e || !coords || !logp || !order || !subset || !z || !u_acc || n0 < 0 || n0 > e->W || e->E != 1) return ALABI_BAD_ARGUMENT;
    // every active half needs s0 rows in the other one, which the kernel's lists must hold
    const int n1 = e->W - n0;
    if (s0 < 2 || (n0 > 0 && s0 > n1) || (n1 > 0 && s0 > n0) || n0 > 2048 || n1 > 2048) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    WkInject inj{subset, z, nullptr};
    return step_injected_wk(e, coords, logp, order, n0, 3, (double)s0, 0.0, inj, u_acc, n_accept, as_stream(stream));
}

int alabi_ens_step_with_randoms_kde(alabi_ens* e, double* coords, double* logp, const int* order, int n0, double factor, const int* r,
                                    const double* z, const double* u_acc, double* lnfac_out, long long* n_accept, void* stream) {
    if (!e || !coords || !logp || !order || !r || !z || !u_acc || n0 < 0 || n0 > e->W || e->E != 1) return ALABI_BAD_ARGUMENT;
    const int n1 = e->W - n0;
    // the pre-pass buffers hold (W + 1) / 2 rows; scipy's gaussian_kde refuses fewer rows than d + 1 as well
    if (!(factor > 0.0) || !std::isfinite(factor) || n0 > (e->W + 1) / 2 || n1 > (e->W + 1) / 2 || n0 < e->d + 1 || n1 < e->d + 1)
        return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    WkInject inj{r, z, lnfac_out};
    return step_injected_wk(e, coords, logp, order, n0, 4, factor, factor, inj, u_acc, n_accept, as_stream(stream));
}

int alabi_ens_step_with_randoms_gauss(alabi_ens* e, double* coords, double* logp, const int* order, int n0, int k_move, double f,
                                      const int* coord, const double* z, const double* u_acc, long long* n_accept, void* stream) {
    if (!e || !coords || !logp || !order || !coord || !z || !u_acc || n0 < 0 || n0 > e->W || e->E != 1) return ALABI_BAD_ARGUMENT;
    if (k_move < 0 || k_move >= e->moves.n || e->moves.kind[k_move] != 5 || !std::isfinite(f))
        return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = sync_consts(e, s)) != ALABI_OK) return st;
    if ((st = ensure_move_buffers(e, true, true)) != ALABI_OK) return st;
    if ((st = launch_ens_prep_wk(e, order, u_acc, s)) != ALABI_OK) return st;
    if ((st = launch_ens_set_step_move(e, 5, e->moves.p0[k_move], e->moves.p1[k_move], s)) != ALABI_OK) return st;
    e->drawn_n = 0;  // row 0 of the draw buffers now holds caller data
    HalfArgs h = base_args(e, coords, logp);
    h.rec = e->draws; h.cw2 = e->mv.cw2; h.cw3 = e->mv.cw3; h.mvkind = e->mv.kind; h.mvpar = e->mv.par; h.kde = e->kde; h.seed = e->seed;
    h.inj = WkInject{coord, z, nullptr};
    h.gauss_C = e->gauss_C; h.gauss_diag = e->gauss_diag; h.gauss_k = k_move; h.gauss_f = f;
    h.n0 = n0; h.n_accept = n_accept; h.local_t = 0; h.part_begin = 0;
    for (int split = 0; split < 2; ++split) {
        const int nS = split == 0 ? n0 : e->W - n0;
        h.split = split;
        if ((st = launch_ens_half_args(e, h, nS, s)) != ALABI_OK) return st;
    }
    return ALABI_OK;
}

int alabi_ens_export_gauss_draws(alabi_ens* e, double* f, int* coord, double* z, void* stream) {
    if (!e || !f || !coord || !z || e->drawn_n < 1 || !e->mv.kind) return ALABI_BAD_ARGUMENT;
    return launch_ens_gauss_export(e, f, coord, z, as_stream(stream));
}

int alabi_ens_hmc_plan(alabi_ens* e, int* out) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    for (int i = 0; i < 4; ++i) out[i] = e->hmc_plan[i];
    return ALABI_OK;
}

int alabi_ens_log_prob_grad(alabi_ens* e, const double* coords, int M, double* logp, double* grad, void* stream) {
    if (!e || !coords || !logp || !grad || M < 0) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    if (M == 0) return ALABI_OK;
    const int st = sync_consts(e, as_stream(stream));
    if (st != ALABI_OK) return st;
    return launch_ens_lp_grad(e, coords, M, logp, grad, as_stream(stream));
}

int alabi_ens_step_with_randoms_hmc(alabi_ens* e, double* coords, double* logp, int k_move, double eps, const double* z,
                                    const double* u_acc, long long* n_accept, void* stream) {
    if (!e || !coords || !logp || !z || !u_acc || e->E != 1 || !e->all_hmc) return ALABI_BAD_ARGUMENT;
    if (k_move < 0 || k_move >= e->moves.n || !(eps > 0.0) || !std::isfinite(eps)) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    const int st = sync_consts(e, s);
    if (st != ALABI_OK) return st;
    return launch_ens_hmc(e, coords, logp, 0, 0, 1, 1, nullptr, nullptr, n_accept, k_move, eps, z, u_acc, s);
}

int alabi_ens_export_hmc_draws(alabi_ens* e, long long step, int* move, double* eps, double* z, double* u_acc, void* stream) {
    if (!e || !move || !eps || !z || !e->all_hmc) return ALABI_BAD_ARGUMENT;
    return launch_ens_hmc_export(e, step, move, eps, z, u_acc, as_stream(stream));
}

int alabi_ens_kde_singular(alabi_ens* e, long long* count) {
    if (!e || !count) return ALABI_BAD_ARGUMENT;
    *count = 0;
    if (!e->kde.singular) return ALABI_OK;
    unsigned long long v = 0;
    ALABI_HIP_CHECK(hipDeviceSynchronize());
    ALABI_HIP_CHECK(hipMemcpy(&v, e->kde.singular, sizeof(v), hipMemcpyDeviceToHost));
    *count = (long long)v;
    return ALABI_OK;
}

int alabi_ens_export_snooker_draws(alabi_ens* e, int* j3, void* stream) {
    if (!e || !j3 || e->drawn_n < 1 || !e->mv.cw3) return ALABI_BAD_ARGUMENT;
    ALABI_HIP_CHECK(hipMemcpyAsync(j3, e->mv.partner3, (size_t)e->W * e->E * sizeof(int), hipMemcpyDeviceToDevice, as_stream(stream)));
    return ALABI_OK;
}

int alabi_ens_export_partner_ids(alabi_ens* e, int* cw2, int* cw3, void* stream) {
    if (!e || e->drawn_n < 1 || (cw2 && !e->mv.cw2) || (cw3 && !e->mv.cw3)) return ALABI_BAD_ARGUMENT;
    const size_t bytes = (size_t)e->W * e->E * sizeof(int);
    if (cw2) ALABI_HIP_CHECK(hipMemcpyAsync(cw2, e->mv.cw2, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
    if (cw3) ALABI_HIP_CHECK(hipMemcpyAsync(cw3, e->mv.cw3, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
    return ALABI_OK;
}

int alabi_ens_export_move_draws(alabi_ens* e, int* move, int* j2, double* gamma, void* stream) {
    if (!e || !move || !j2 || !gamma || e->drawn_n < 1 || !e->mv.cw2) return ALABI_BAD_ARGUMENT;
    hipStream_t s = as_stream(stream);
    const size_t WT = (size_t)e->W * e->E;
    ALABI_HIP_CHECK(hipMemcpyAsync(move, e->mv.move, (size_t)e->E * sizeof(int), hipMemcpyDeviceToDevice, s));
    ALABI_HIP_CHECK(hipMemcpyAsync(j2, e->mv.partner2, WT * sizeof(int), hipMemcpyDeviceToDevice, s));
    ALABI_HIP_CHECK(hipMemcpyAsync(gamma, e->draws.zz, WT * sizeof(double), hipMemcpyDeviceToDevice, s));
    return ALABI_OK;
}

int alabi_ens_export_draws(alabi_ens* e, long long step, double a, int* order, int* n0, double* u_z, int* partner,
                           double* u_acc, int* cw, double* zz, void* stream) {
    if (!e || !order || !n0 || !u_z || !partner || !u_acc) return ALABI_BAD_ARGUMENT;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = alabi_ens_draw(e, step, 1, a, stream)) != ALABI_OK) return st;
    const size_t WT = (size_t)e->W * e->E;
    ALABI_HIP_CHECK(hipMemcpyAsync(order, e->draws.order, WT * sizeof(int), hipMemcpyDeviceToDevice, s));
    ALABI_HIP_CHECK(hipMemcpyAsync(partner, e->draws.partner, WT * sizeof(int), hipMemcpyDeviceToDevice, s));
    ALABI_HIP_CHECK(hipMemcpyAsync(u_z, e->draws.u_z, WT * sizeof(double), hipMemcpyDeviceToDevice, s));
    ALABI_HIP_CHECK(hipMemcpyAsync(u_acc, e->draws.u_acc, WT * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (cw) ALABI_HIP_CHECK(hipMemcpyAsync(cw, e->draws.cw, WT * sizeof(int), hipMemcpyDeviceToDevice, s));
    if (zz) ALABI_HIP_CHECK(hipMemcpyAsync(zz, e->draws.zz, WT * sizeof(double), hipMemcpyDeviceToDevice, s));
    *n0 = (e->W + 1) / 2;
    return ALABI_OK;
}

}  // extern "C"
