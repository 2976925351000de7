// Which kernel a predict request runs and with what launch geometry: the environment switches of the predict path (read in ONE
// place, predict_plan.hip) and pure functions of (M, Npad, d, n_cu, switches).  gp_predict.hip launches what they return.
// Plain C++: no HIP header, so predict_plan.hip compiles with any host compiler and runs under a host sanitizer.
#pragma once

namespace alabi {

// ---- the environment switches.  predict_switches() reads them afresh on every call (tests flip them inside one process) and is
// the only function of the predict path that reads the environment.  A flag is kept as read: PRED_UNSET when the variable is not
// set, otherwise the first character of its value ('\0' for an empty one); the predicates below say which characters mean what.
constexpr int PRED_UNSET = -1;
struct PredictSwitches {
    int pm_mfma = PRED_UNSET;       // ALABI_PM_MFMA: '0' predict-mean on the vector kernels for every batch size
    int pv_small = PRED_UNSET;      // ALABI_PV_SMALL: '0' no small-batch variance kernel
    int pv_w = PRED_UNSET;          // ALABI_PV_W: '0' substitution kernels instead of the product with the cached L^-1
    int pv_w2 = PRED_UNSET;         // ALABI_PV_W2: '0' one matrix-core wave per SIMD at every batch size
    int pv_legacy = PRED_UNSET;     // ALABI_PV_LEGACY: '1' the first-generation substitution kernel
    int winv_dnc = PRED_UNSET;      // ALABI_WINV_DNC: '0' L^-1 by substitution chains instead of the recursive block inversion
    long long pv_chunk_tiles = 0;   // ALABI_PV_CHUNK_TILES > 0: 64-query tiles per chunk of a variance request (0: by size)
};
PredictSwitches predict_switches();

// With the recursive block inversion the cached L^-1 costs less than the dependency chain of ONE substitution launch (0.24 vs
// 0.6 ms at N = 2000, 2.1 vs 3.5 ms at N = 5000), so every variance request goes through it unless the switch forbids it; the
// substitution kernels remain the fallback when the two Npad^2 buffers cannot be had (the launcher's decision: it allocates).
inline bool predict_use_winv(const PredictSwitches& sw) { return sw.pv_w != '0'; }
inline bool predict_winv_dnc(const PredictSwitches& sw) { return sw.winv_dnc != '0'; }

// ---- mean
enum { PM_ROWWISE = 0, PM_TILE = 1, PM_MFMA = 2 };
struct MeanPlan {
    int route;            // PM_ROWWISE predict_mean_rowwise_kernel, PM_TILE predict_mean_tile_kernel, PM_MFMA predict_mean_mfma_kernel
    long long gx;         // gridDim.x: queries (rowwise), 64-query tiles (tile), 256-query workgroups (matrix cores)
    int parts;            // gridDim.y: workgroups the training points are split over (> 1: mean_combine_kernel adds the parts)
    int pts_per_part;     // matrix cores: training points per part (a multiple of 16)
    int ks;               // matrix cores: k-steps of four coordinates of the augmented rows
    long long mu_stride;  // stride of the partial sums
};
int predict_mean_route(long long M, int d, const PredictSwitches& sw);
MeanPlan predict_mean_plan(long long M, int Npad, int d, int n_cu, const PredictSwitches& sw);

// Fewer 64-query tiles than two per CU: the 256-point stages of the training set are dealt to this many workgroups per tile
// (predict_mean_tile_kernel, and the K* pre-pass in front of the product with L^-1).
int predict_nsplit(long long tiles, int Npad, int n_cu);

// ---- variance
// Up to 128 queries (64 beyond Npad = 2048): groups of 16 multiply with the cached L^-1, K* evaluated in place
// (predict_var_small_kernel).  Asked by alabi_gp_predict only; the utility scan always takes the tile kernels.
bool predict_var_small(long long M, int Npad, int d, const PredictSwitches& sw);

enum { PV_W = 1, PV_SUBST = 2, PV_FIRSTGEN = 3 };
struct VarPlan {
    int route;            // PV_W product with the cached L^-1 (PV_SUBST when it cannot be had), PV_SUBST wave-specialised substitution,
                          // PV_FIRSTGEN predict_var_kernel
    int TM;               // PV_SUBST: queries per tile of predict_var_ws_kernel, 16 or 64
    long long chunk;      // PV_W / PV_SUBST: queries per chunk before any out-of-memory halving (a multiple of 64)
    int grid;             // PV_FIRSTGEN: workgroups
};
VarPlan predict_var_plan(long long M, int Npad, int d, int n_cu, const PredictSwitches& sw);

struct VarChunk {
    long long groups;     // K* workgroups of 64 queries
    int nsplit;           // gridDim.y of the K* pre-pass (product route only)
    bool w2;              // predict_var_w2_kernel (two matrix-core waves per SIMD, 128 queries per workgroup)
    int parts, gx;        // product route: grid (gx, parts), block rows of a tile split over `parts` workgroups
    int grid_c;           // substitution route: workgroups of predict_var_ws_kernel
};
VarChunk predict_var_chunk(long long mc, int Npad, int n_cu, bool use_w, int TM, const PredictSwitches& sw);

}  // namespace alabi
