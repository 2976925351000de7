// Batched GP prediction for gfx950: mu* = k(X*,X) alpha + m and var* = k** - |L^-1 k*|^2.  The launchers.
//
// Replaces george's gp.predict(y, X*, return_var=) reached from the reference at
// alabi/core.py:85, :95 (cached likelihood), :1441, :1486 (surrogate_log_likelihood),
// :1601 (acquisition), :1812/:1828 (bookkeeping).  K* is never materialised in HBM.
//
// Which kernel a request runs, and with what grid, is decided in predict_plan.hip (plain C++; the only reader of the predict
// path's environment switches); the functions here allocate, launch what the plan says and keep the out-of-memory fallbacks.
//
//   launch_predict_mean        predict_mean.hpp.  Up to 4096 queries one workgroup per query (predict_mean_rowwise_kernel), beyond
//                              that 64 queries per workgroup with the training points staged in LDS (predict_mean_tile_kernel);
//                              from 2048 queries on with d + 2 <= 32 the dot products run on the matrix cores
//                              (predict_mean_mfma_kernel over the rows ensure_xa builds).  Too few workgroups to fill the chip:
//                              the training points are split over gridDim.y and mean_combine_kernel adds the parts.
//   launch_predict_var_small   predict_var_winv.hpp.  Up to 128 queries (alabi_gp_predict only): groups of 16 queries multiply
//                              with the cached W = L^-1, K* evaluated in place (predict_var_small_kernel, _final_kernel); the
//                              mean comes from launch_predict_mean.
//   launch_predict_var         d <= 32: the K* pre-pass (predict_kstar_tile_kernel, predict_var_subst.hpp) writes K* and the mean,
//                              then var = amp - colnorm^2(W K*^T) as a product with the cached W (predict_var_w_kernel, from 32
//                              tiles on predict_var_w2_kernel, then predict_var_w_final_kernel; predict_var_winv.hpp).  Without
//                              the cache (ALABI_PV_W=0, or no room for it) the wave-specialised blocked forward substitution
//                              V = L^-1 K*^T (predict_var_ws_kernel<16 / 64>, predict_var_subst.hpp).  d > 32 or ALABI_PV_LEGACY=1:
//                              the first-generation substitution kernel, K* evaluated on the fly (predict_var_kernel).
//   ensure_winv,               W = L^-1 of the current factor, tile-major: the recursive block inversion of gp_inverse.hip, or
//   launch_factor_inverse*     (ALABI_WINV_DNC=0) the columns of the identity pushed through predict_var_ws_kernel<16> between
//                              ident_seed_kernel and retile_16_to_64_kernel (below, next to their only launcher), or
//                              predict_var_kernel<1, true> when there is no workspace for either.
//
// All DEVICE code of the predict path is compiled in this one translation unit: the code generated for these kernels depends on
// their module mates, and the module-scope LDS stages of predict_var_subst.hpp are shared with predict_var_winv.hpp.
// tools/isa_diff.py compares the device assembly of two builds symbol by symbol; a refactor of these files should leave it
// without a difference.
#include "gp_device.hpp"
#include "predict_plan.hpp"
#include "predict_mean.hpp"
#include "predict_var_subst.hpp"
#include "predict_var_winv.hpp"

namespace alabi {

int ensure_xa(alabi_gp* gp, hipStream_t s) {
    const int rows = round_up(gp->d + 2, 4);
    if (!gp->Xa) ALABI_HIP_CHECK(hipMalloc(&gp->Xa, (size_t)rows * gp->n_cap * sizeof(double)));
    if (!gp->xa_centre) ALABI_HIP_CHECK(hipMalloc(&gp->xa_centre, ALABI_MAX_DIM * sizeof(double)));
    if (gp->xa_gen != gp->factor_gen) {
        hipLaunchKernelGGL(xa_centre_kernel, dim3(gp->d), dim3(256), 0, s, gp->Xt, gp->Npad, gp->N, gp->xa_centre);
        hipLaunchKernelGGL(build_xa_kernel, dim3((gp->Npad + 255) / 256), dim3(256), 0, s, gp->Xt, gp->Npad, gp->d, rows,
                           gp->xa_centre, gp->Xa);
        ALABI_LAUNCH_CHECK();
        gp->xa_gen = gp->factor_gen;
    }
    return ALABI_OK;
}

#define ALABI_DISPATCH_KS(KS_, ...)                                                             \
    switch (KS_) {                                                                              \
        case 1: { constexpr int KS = 1; __VA_ARGS__; } break;                                   \
        case 2: { constexpr int KS = 2; __VA_ARGS__; } break;                                   \
        case 3: { constexpr int KS = 3; __VA_ARGS__; } break;                                   \
        case 4: { constexpr int KS = 4; __VA_ARGS__; } break;                                   \
        case 5: { constexpr int KS = 5; __VA_ARGS__; } break;                                   \
        case 6: { constexpr int KS = 6; __VA_ARGS__; } break;                                   \
        case 7: { constexpr int KS = 7; __VA_ARGS__; } break;                                   \
        case 8: { constexpr int KS = 8; __VA_ARGS__; } break;                                   \
        default: return ALABI_BAD_ARGUMENT;                                                     \
    }

int launch_predict_mean(alabi_gp* gp, const double* Xs, long long M, double* mu, const PredictSwitches& sw, hipStream_t s) {
    if (M <= 0) return ALABI_OK;
    const int db = dim_bucket(gp->d);
    const double amp = exp(gp->log_amp);
    if (predict_mean_route(M, gp->d, sw) == PM_ROWWISE) {     // (the route of per-point calls: decided without a device query)
        ALABI_DISPATCH_DIM(db, hipLaunchKernelGGL(predict_mean_rowwise_kernel<D>, dim3((unsigned)M), dim3(256), 0, s,
                                                  gp->Xt, gp->alpha, gp->Npad, Xs, gp->d, gp->inv_len, amp,
                                                  gp->mean, gp->kf, mu));
        ALABI_LAUNCH_CHECK();
        return ALABI_OK;
    }
    const MeanPlan p = predict_mean_plan(M, gp->Npad, gp->d, device_cu_count(), sw);
    int st;
    if (p.route == PM_MFMA && (st = ensure_xa(gp, s)) != ALABI_OK) return st;
    if (p.gx > 0x7fffffffLL) return ALABI_BAD_ARGUMENT;
    if (p.parts > 1 && (st = grow_plain(&gp->mupart, &gp->mupart_bytes, (size_t)p.parts * p.mu_stride * sizeof(double), s)) != ALABI_OK) return st;
    if (p.route == PM_MFMA) {
        ALABI_DISPATCH_KS(p.ks, ALABI_DISPATCH_KERNEL(gp->kf.type, hipLaunchKernelGGL((predict_mean_mfma_kernel<KS, GENERIC>), dim3((unsigned)p.gx, p.parts),
            dim3(256), 0, s, gp->Xa, gp->alpha, gp->Npad, Xs, gp->d, M, gp->inv_len, gp->xa_centre, amp, gp->mean, gp->kf, mu,
            p.parts > 1 ? gp->mupart : (double*)nullptr, p.mu_stride, p.pts_per_part)));
    } else {
        ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(gp->kf.type, hipLaunchKernelGGL((predict_mean_tile_kernel<D, GENERIC>), dim3((unsigned)p.gx, p.parts), dim3(256), 0, s,
                                                  gp->Xt, gp->alpha, gp->Npad, Xs, gp->d, M, gp->inv_len, amp,
                                                  gp->mean, gp->kf, mu, gp->mupart, p.mu_stride)));
    }
    if (p.parts > 1)
        hipLaunchKernelGGL(mean_combine_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, gp->mupart, p.parts, p.mu_stride, M, amp,
                           gp->mean, mu);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

// ALABI_WINV_DNC=0 only: the seeds and the re-tiling around predict_var_ws_kernel<16> in launch_factor_inverse_into
__global__ void __launch_bounds__(256)
ident_seed_kernel(double* __restrict__ seeds, int Npad) {
    // 16-wide tiles: seeds[t][n][c] = (n == 16 t + c)
    const size_t n_el = (size_t)Npad * Npad;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n_el; e += (size_t)gridDim.x * 256) {
        const size_t t = e / ((size_t)Npad * 16), rem = e % ((size_t)Npad * 16);
        seeds[e] = ((rem >> 4) == 16 * t + (rem & 15)) ? 1.0 : 0.0;
    }
}

__global__ void __launch_bounds__(256)
retile_16_to_64_kernel(const double* __restrict__ src, double* __restrict__ dst, int Npad) {
    // src[t16][n][16] -> dst[t64][n][64]
    const size_t n_el = (size_t)Npad * Npad;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n_el; e += (size_t)gridDim.x * 256) {
        const size_t t64 = e / ((size_t)Npad * 64), rem = e % ((size_t)Npad * 64);
        const size_t n = rem >> 6, c = rem & 63;
        dst[e] = src[((t64 * 4 + (c >> 4)) * Npad + n) * 16 + (c & 15)];
    }
}

// L^-1 tile-major into dst: dst[t] = L^-1[:, 64t:64t+64] as [Npad][64].  The columns of the identity are pushed through the
// wave-specialised substitution kernel as 16-wide tiles (Npad / 16 independent workgroups, 1.3 us per stage) into the
// variance workspace and re-tiled; the first-generation kernel (Npad / 64 workgroups, 3.3 us per stage) when the workspace
// cannot be had.
int launch_factor_inverse_into(alabi_gp* gp, double* dst, hipStream_t s) {
    const int nb = gp->Npad / 64;
    const size_t need = (size_t)gp->Npad * gp->Npad * sizeof(double);
    bool fast = dst != gp->ws && nb >= 2;
    if (fast) {
        const int st = grow_cached(&gp->ws, &gp->ws_bytes, need, s);
        if (st == ALABI_NOT_COMPUTED) fast = false;
        else if (st != ALABI_OK) return st;
    }
    if (fast) {
        // recursive block inversion on the matrix cores (gp_inverse.hip); ALABI_WINV_DNC=0 keeps the substitution chains
        if (predict_winv_dnc(predict_switches())) return launch_factor_inverse_dnc(gp, gp->ws, dst, s);
        const int n_cu = device_cu_count();
        const int tiles = gp->Npad / 16;
        hipLaunchKernelGGL(ident_seed_kernel, dim3(1024), dim3(256), 0, s, gp->ws, gp->Npad);
        hipLaunchKernelGGL(predict_var_ws_kernel<16>, dim3(tiles < n_cu ? tiles : n_cu), dim3(512), 0, s, gp->L, gp->dinv, gp->Npad,
                           (long long)gp->Npad, 0.0, gp->ws, gp->work, 1);
        hipLaunchKernelGGL(retile_16_to_64_kernel, dim3(1024), dim3(256), 0, s, gp->ws, dst, gp->Npad);
        ALABI_LAUNCH_CHECK();
        return ALABI_OK;
    }
    hipLaunchKernelGGL((predict_var_kernel<1, true>), dim3(nb), dim3(256), 0, s, gp->L, gp->dinv, gp->Xt, gp->alpha, gp->N,
                       gp->Npad, (const double*)nullptr, gp->d, (long long)gp->Npad, gp->inv_len, 1.0, 0.0, dst,
                       (double*)nullptr, (double*)nullptr, 0, gp->kf);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

// ... into the variance workspace (the gradient's use)
int launch_factor_inverse(alabi_gp* gp, hipStream_t s) {
    if (grow_cached(&gp->ws, &gp->ws_bytes, (size_t)gp->Npad * gp->Npad * sizeof(double), s) != ALABI_OK) return ALABI_HIP_ERROR;
    return launch_factor_inverse_into(gp, gp->ws, s);
}

// The cached W = L^-1 of the current factor (tile-major, Npad^2 doubles); ALABI_NOT_COMPUTED when there is no room for it.
int ensure_winv(alabi_gp* gp, hipStream_t s) {
    const size_t need = (size_t)gp->Npad * gp->Npad * sizeof(double);
    if (need > gp->winv_bytes) {
        const int st = grow_cached(&gp->winv, &gp->winv_bytes, need, s);
        if (st != ALABI_OK) return st;
        gp->winv_gen = -1;
    }
    if (gp->winv_gen != gp->factor_gen) {
        int st = launch_factor_inverse_into(gp, gp->winv, s);
        if (st != ALABI_OK) return st;
        gp->winv_gen = gp->factor_gen;
    }
    return ALABI_OK;
}

int launch_predict_var(alabi_gp* gp, const double* Xs, long long M, double* mu, double* var, const PredictSwitches& sw, hipStream_t s) {
    if (M <= 0) return ALABI_OK;
    const int db = dim_bucket(gp->d);
    const int n_cu = device_cu_count();
    const VarPlan p = predict_var_plan(M, gp->Npad, gp->d, n_cu, sw);
    const double amp = exp(gp->log_amp);
    if (p.route == PV_FIRSTGEN) {
        if (grow_cached(&gp->ws, &gp->ws_bytes, (size_t)p.grid * gp->Npad * 64 * sizeof(double), s) != ALABI_OK) return ALABI_HIP_ERROR;
        const int split = 0;   // a run-time zero the kernel tests against (see its first comment): keeps two code regions apart
        ALABI_DISPATCH_DIM(db, hipLaunchKernelGGL(predict_var_kernel<D>, dim3(p.grid), dim3(256), 0, s, gp->L, gp->dinv, gp->Xt,
                                                  gp->alpha, gp->N, gp->Npad, Xs, gp->d, M, gp->inv_len, amp,
                                                  gp->mean, gp->ws, mu, var, split, gp->kf));
        ALABI_LAUNCH_CHECK();
        return ALABI_OK;
    }
    // every tile owns Npad x 64 doubles of workspace (K* seeds in, V out).  Short of memory: halve the chunk down to one round
    // over the CUs before giving up
    long long chunk = p.chunk;
    int st;
    while ((st = grow_cached(&gp->ws, &gp->ws_bytes, (size_t)(chunk / 64) * gp->Npad * 64 * sizeof(double), s)) == ALABI_NOT_COMPUTED) {
        if (chunk <= 64LL * n_cu) return ALABI_HIP_ERROR;
        chunk = (chunk / 2 + 63) / 64 * 64;
        if (chunk < 64LL * n_cu) chunk = 64LL * n_cu;
    }
    if (st != ALABI_OK) return st;
    // Product with the cached L^-1 (no dependency between stages, block rows of a tile split over `parts` workgroups when the
    // tiles alone cannot fill the chip); the substitution kernel when the plan says so or there is no room for the cache.
    bool use_w = p.route == PV_W;
    if (use_w) {
        st = ensure_winv(gp, s);
        if (st == ALABI_NOT_COMPUTED) use_w = false;
        else if (st != ALABI_OK) return st;
    }
    for (long long m0 = 0; m0 < M; m0 += chunk) {
        const long long mc = (M - m0 < chunk) ? M - m0 : chunk;
        const VarChunk c = predict_var_chunk(mc, gp->Npad, n_cu, use_w, p.TM, sw);
        const long long mu_stride = c.groups * 64;
        double* mu_part = nullptr;
        if (c.nsplit > 1) {
            if ((st = grow_plain(&gp->mupart, &gp->mupart_bytes, (size_t)c.nsplit * mu_stride * sizeof(double), s)) != ALABI_OK) return st;
            mu_part = gp->mupart;
        }
        ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(gp->kf.type, hipLaunchKernelGGL((predict_kstar_tile_kernel<D, GENERIC>),
            dim3((unsigned)c.groups, c.nsplit), dim3(256), 0, s, gp->Xt, gp->alpha, gp->N, gp->Npad, Xs + m0 * gp->d, gp->d, mc,
            gp->inv_len, amp, gp->mean, gp->kf, gp->ws, mu + m0, use_w ? 64 : p.TM, mu_part, mu_stride)));
        if (use_w) {
            if ((st = grow_plain(&gp->small, &gp->small_bytes, (size_t)c.groups * c.parts * 64 * sizeof(double), s)) != ALABI_OK) return st;
            if (c.w2)
                hipLaunchKernelGGL(predict_var_w2_kernel, dim3(c.gx, c.parts), dim3(768), 0, s, gp->winv, gp->ws, gp->Npad, c.groups,
                                   c.parts, gp->small);
            else
                hipLaunchKernelGGL(predict_var_w_kernel, dim3(c.gx, c.parts), dim3(512), 0, s, gp->winv, gp->ws, gp->Npad, c.groups,
                                   c.parts, gp->small);
            hipLaunchKernelGGL(predict_var_w_final_kernel, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, s, gp->small, c.parts, mc,
                               amp, var + m0, mu_part, c.nsplit, mu_stride, gp->mean, mu + m0);
        } else if (p.TM == 16) {
            hipLaunchKernelGGL(predict_var_ws_kernel<16>, dim3(c.grid_c), dim3(512), 0, s, gp->L, gp->dinv, gp->Npad, mc, amp,
                               gp->ws, var + m0, 0);
        } else {
            hipLaunchKernelGGL(predict_var_ws_kernel<64>, dim3(c.grid_c), dim3(512), 0, s, gp->L, gp->dinv, gp->Npad, mc, amp,
                               gp->ws, var + m0, 0);
        }
    }
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_predict_var_small(alabi_gp* gp, const double* Xs, int M, double* mu, double* var, const PredictSwitches& sw, hipStream_t s) {
    const int nb = gp->Npad / 64, db = dim_bucket(gp->d);
    int st = ensure_winv(gp, s);
    if (st == ALABI_NOT_COMPUTED) return launch_predict_var(gp, Xs, M, mu, var, sw, s);   // no room: substitution kernel
    if (st != ALABI_OK) return st;
    const int groups = (M + 15) / 16;
    if ((st = grow_plain(&gp->small, &gp->small_bytes, (size_t)groups * nb * 16 * sizeof(double), s)) != ALABI_OK) return st;
    if ((st = launch_predict_mean(gp, Xs, M, mu, sw, s)) != ALABI_OK) return st;
    const double amp = exp(gp->log_amp);
    ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(gp->kf.type, hipLaunchKernelGGL((predict_var_small_kernel<D, GENERIC>), dim3(nb, groups),
        dim3(256), 0, s, gp->winv, gp->Xt, gp->N, gp->Npad, Xs, gp->d, M, gp->inv_len, amp, gp->kf, gp->small)));
    hipLaunchKernelGGL(predict_var_small_final_kernel, dim3((M + 63) / 64), dim3(64), 0, s, gp->small, nb, M, amp, var);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // namespace alabi
