// What the ensemble kernels and the host-only plan (ens_plan.hip) both read: the dimension buckets, the fit table of the persistent
// kernels, the group kernel's LDS layout and the LDS bounds of the Metropolis kernels.  Compiles without a HIP header: ALABI_HD is
// `__host__ __device__` under hipcc and nothing elsewhere, so the kernels and a plain C++ compiler see the same functions.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define ALABI_HD __host__ __device__
#else
#define ALABI_HD
#endif

namespace alabi {

// Compile-time dimension buckets: a GP of dimension d runs the instantiation for the
// smallest bucket >= d; Xt rows beyond d are zero and so contribute nothing to r^2.
ALABI_HD inline int dim_bucket(int d) {
    const int b[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64};
    for (int i = 0; i < 15; ++i)
        if (d <= b[i]) return b[i];
    return -1;
}

// ---- persistent kernels (ens_stream.hpp: the launch table)
// T compute lanes (+ the hand-off wave and the record wave), PPT point pairs per lane.  The fit rule: the largest dimension
// bucket of a (T, PPT, kernel family) row that compiles without VGPR spills (hipcc -Rpass-analysis=kernel-resource-usage;
// 256 VGPRs at 384 threads, 168 at 640); 0: no such row.  ens_stream_ppt and the dispatch both read it, so an instantiation
// that can never be chosen is not compiled.
constexpr int ens_stream_max_db(int T, int ppt, bool generic) {
    if (T == 512) return ppt == 1 ? (generic ? 12 : 16) : ppt == 2 ? (generic ? 6 : 10) : 0;
    if (T == 256) return ppt == 1 ? 16 : ppt == 2 ? (generic ? 12 : 16) : ppt == 3 ? (generic ? 8 : 12) : ppt == 4 ? (generic ? 6 : 10) : 0;
    return 0;
}

// ---- group kernel (ens_group.hip)
#define ALABI_GRP_NW 8                           // waves per workgroup (512 threads, two per SIMD)
#define ALABI_GRP_RT 5                           // point tiles per wave held in registers by the G8 instantiations

// LDS layout (units of 8 bytes), the same formula on the host.
struct GroupLds {
    int etab, xb, al, aop, wsum, rec, ctl, total;
};
ALABI_HD inline GroupLds group_lds(int KS, int QPAD, int lds_tiles) {
    const int S = 16 * lds_tiles;
    GroupLds L;
    int o = 0;
    L.etab = o; o += 256;
    L.xb = o; o += S * KS * 4;            // lds_tiles (= 8 waves x tiles per wave in LDS) x KS k-steps x 64 lanes
    L.al = o; o += S;
    L.aop = o; o += QPAD * KS * 4;
    L.wsum = o; o += ALABI_GRP_NW * QPAD;
    L.rec = o; o += 4 * QPAD * 6;         // ring of 4 half steps: 4 record words + 2 link words per proposal
    L.ctl = o; o += 2;
    L.total = o;
    return L;
}

// ---- Metropolis kernels (ens_mh.hip, ens_hmc.hip): the most dynamic LDS a launch may ask for
#define ALABI_MH_MAX_LDS (128 * 1024)
#define ALABI_HMC_MAX_LDS (128 * 1024)
// p1 of an HMC row of the move table is n_leapfrog + ln jitter / 512 (ens_grad_device.hpp: hmc_ln_jitter_of)
ALABI_HD inline int hmc_leapfrog_of(double p1) { return (int)floor(p1); }
// ---- NUTS kernel (ens_nuts.hip): p1 of a kind-7 row is max_depth + ln jitter / 512, read by the same two functions; the deepest
// tree has 2^10 - 1 leaves, and the U-turn checkpoints of a subtree [2][ALABI_NUTS_MAX_DEPTH][64] doubles lie in dynamic LDS
#define ALABI_NUTS_MAX_DEPTH 10

}  // namespace alabi
