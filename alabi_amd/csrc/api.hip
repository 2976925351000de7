// extern "C" entry points of libalabi_hip.so (declared in include/alabi_hip.h): the ABI and device info, the process-wide buffer cache,
// the GP and the utility entry points.  The ensemble sampler's are in ens_api.hip and ens_run.hip.
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

}  // extern "C"
