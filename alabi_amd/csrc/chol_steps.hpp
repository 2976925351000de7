// The launch-per-step factorisation: four kernels, launched by launch_cholesky_steps (gp_cholesky.hip).
// Per 64-column block step kb (two launches; the first diagonal block has its own one-wave launch):
//   1. trsm_panel   : A[i,kb] <- A[i,kb] * L_kk^-T.  One lane owns one row: the substitution along the
//                     row is right-looking in registers (two dependent operations per column), L_kk is
//                     read from LDS as broadcasts, divisions are multiplications by dinv = 1/L_jj.
//   2. syrk_update  : A[i,j] -= A[i,kb] * A[j,kb]^T for kb < j <= i, one 64x64 tile per workgroup,
//                     4 waves x (16 rows x 64 cols) x K=64 on MFMA.  The workgroup of tile (kb+1,kb+1)
//                     then FACTORISES that tile while it is still in LDS (potrf_tile_lds_wg: wave 0 the
//                     16-column slabs in registers, v_readlane broadcasts, rank-16 MFMA updates between
//                     slabs on all waves), so the diagonal factorisation costs no launch of its own.
//   Large matrices take panels of several block columns; syrk_panel_kernel applies a whole panel to the trailing matrix at once.
// Device code only; compiled as part of gp_cholesky.hip (one translation unit for all Cholesky device code, see there).
#pragma once
#include "chol_tiles.hpp"

namespace alabi {

// First diagonal block (the later ones are factorised inside syrk_update_kernel by the workgroup that finishes them).
__global__ void __launch_bounds__(64)
potrf_diag_kernel(double* __restrict__ A, int ld, int kb, int* __restrict__ info, double* __restrict__ dinv) {
    __shared__ double Ls[64][65];
    const int lane = threadIdx.x;
    double* Ab = A + (size_t)(kb * 64) * ld + kb * 64;
#pragma unroll
    for (int r = 0; r < 64; ++r) Ls[r][lane] = Ab[(size_t)r * ld + lane];   // coalesced rows, all 64 loads in flight
    __syncthreads();
    dinv[kb * 64 + lane] = potrf_tile_lds<65>(Ls, lane, kb, info);
#pragma unroll
    for (int r = 0; r < 64; ++r)
        if (lane <= r) Ab[(size_t)r * ld + lane] = Ls[r][lane];
}

// X * L_kk^T = B for 64 rows; four wavefronts, wave w owns rows 16w..16w+15.  16-column slabs: inside a slab one lane
// runs one row's recurrence (trsm_slab_row: L_kk read from LDS as broadcasts, divisions are multiplications by dinv, no
// cross-lane traffic); the slab's effect on the remaining columns is a rank-16 update on the matrix cores, one row tile per
// wave.
__global__ void __launch_bounds__(256)
trsm_panel_kernel(double* __restrict__ A, int ld, int kb, const double* __restrict__ dinv) {
    __shared__ double lkk[64][65];
    __shared__ double bs[64][65];
    __shared__ double di[64];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const double* Lb = A + (size_t)(kb * 64) * ld + kb * 64;
    double* Bb = A + (size_t)((kb + 1 + blockIdx.x) * 64) * ld + kb * 64;
    #pragma unroll
    for (int e_ = 0; e_ < 16; ++e_) {
        const int e = tid + 256 * e_;
        const int r = e >> 6, c = e & 63;
        lkk[r][c] = Lb[(size_t)r * ld + c];
        bs[r][c] = Bb[(size_t)r * ld + c];
    }
    if (tid < 64) di[tid] = dinv[kb * 64 + tid];
    __syncthreads();
    const int row = 16 * w + (lane & 15);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int c0 = 16 * s;
        if (lane < 16) trsm_slab_row<65>(lkk, bs, di, row, c0);
        __syncthreads();
        // B[rows of this wave, later slabs] -= X_s * L_kk[later rows, slab]^T
#pragma unroll
        for (int t = s + 1; t < 4; ++t) tile_update_16<65>(bs, 16 * w, 16 * t, bs, 16 * w, lkk, 16 * t, c0, lane);
        __syncthreads();
    }
    #pragma unroll
    for (int e_ = 0; e_ < 16; ++e_) {
        const int e = tid + 256 * e_;
        const int r = e >> 6, c = e & 63;
        Bb[(size_t)r * ld + c] = bs[r][c];
    }
}

// C[bi,bj] -= P[bi] * P[bj]^T with P[b] = A[b-block rows, kb-block cols].  Workgroup 0 owns the tile (kb+1, kb+1), which is
// complete after this update: it factorises it on the spot (one wave, potrf_tile_lds), so the next block step starts with
// its panel solve and the diagonal factorisation costs no launch, no reload and overlaps the other tiles' updates.
// jc > 0 restricts the update to the first jc block columns of the trailing matrix (the rest of a 256-column panel; the
// columns beyond it receive the whole panel at once from syrk_panel_kernel): tiles are then numbered column by column.
__global__ void __launch_bounds__(256)
syrk_update_kernel(double* __restrict__ A, int ld, int kb, int* __restrict__ info, double* __restrict__ dinv, int jc, int T) {
    __shared__ double Pi[64][66];
    __shared__ double Pj[64][66];
    int t = blockIdx.x;
    int ti, tj;
    if (jc > 0) {
        tj = 0;
        int off = 0;
        while (tj + 1 < jc && t >= off + (T - tj)) { off += T - tj; ++tj; }
        ti = tj + (t - off);
    } else {
        ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
        while (ti * (ti + 1) / 2 > t) --ti;
        tj = t - ti * (ti + 1) / 2;
    }
    const int bi = kb + 1 + ti, bj = kb + 1 + tj;
    const int tid = threadIdx.x;
    const double* Ai = A + (size_t)(bi * 64) * ld + kb * 64;
    const double* Aj = A + (size_t)(bj * 64) * ld + kb * 64;
    #pragma unroll
    for (int e_ = 0; e_ < 16; ++e_) {
        const int e = tid + 256 * e_;
        int r = e >> 6, c = e & 63;
        Pi[r][c] = Ai[(size_t)r * ld + c];
        Pj[r][c] = Aj[(size_t)r * ld + c];
    }
    const int w = tid >> 6, l = tid & 63;
    const int lr = l & 15, lk = l >> 4;
    double* C = A + (size_t)(bi * 64 + 16 * w) * ld + bj * 64;
    v4f64 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[n][i] = C[(size_t)(lk + 4 * i) * ld + 16 * n + lr];
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        double a = -Pi[16 * w + lr][4 * ks + lk];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            double b = Pj[16 * n + lr][4 * ks + lk];
            acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[n], 0, 0, 0);
        }
    }
    if (t == 0) {
        __syncthreads();                                   // every wave is done reading Pi / Pj
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int i = 0; i < 4; ++i) Pi[16 * w + lk + 4 * i][16 * n + lr] = acc[n][i];
        __syncthreads();
        const double rinv = potrf_tile_lds_wg<66>(Pi, tid, bi, info);
        if (w == 0) dinv[bi * 64 + l] = rinv;
        double* D = A + (size_t)(bi * 64) * ld + bi * 64;
#pragma unroll
        for (int r0_ = 0; r0_ < 64; r0_ += 4) {
            const int r = r0_ + w;
            if (l <= r) D[(size_t)r * ld + l] = Pi[r][l];
        }
        return;
    }
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) C[(size_t)(lk + 4 * i) * ld + 16 * n + lr] = acc[n][i];
}

// Trailing update with a whole 256-column panel: C[I,J] -= P_I P_J^T for 128 x 128 tiles (I >= J) of the matrix behind the
// panel, P_X = A[rows of tile X, panel columns] (128 x KP, KP = 64 * width of the panel in blocks <= 256).  Rank-64 updates
// re-read and re-write every trailing tile once per block column (5-7x the algorithmic traffic); here a
// tile is read and written ONCE per four block columns and each staged panel byte feeds a 128-wide output: 11 flop per
// byte of L2 traffic instead of 4.  Four wavefronts, each owns a 64 x 64 quadrant = 4 x 4 accumulator tiles of
// v_mfma_f64_16x16x4 (128 VGPRs); the panel rows are staged 16 columns at a time through two LDS buffers (row stride 18
// doubles: conflict-free ds_read_b64 for the fragment layout), the next slice is fetched into registers while the current
// one is multiplied; one barrier per slice.  Tile columns [tc0, tc1) of the trailing matrix are processed (look-ahead: the
// columns of the next panel on the main stream, the rest on a second stream).
// FUSE_POTRF = false is the bulk instantiation (the look-ahead remainder): without the factorisation code it stays below
// 256 registers, so TWO workgroups share a CU and one's barriers and fetch waits hide behind the other's MFMAs (with the
// fused code in the same kernel the allocation was 392 registers: one wave per SIMD, 48 % matrix-core occupancy,
// profiles/r02_cholesky_n10000_timeline.txt).  Tiles that lie wholly inside the matrix (all but the last tile row) take
// loads and stores without per-element guards; a wave whose 64 x 64 quadrant is the upper block of a diagonal tile idles.
// The accumulators hold -C, so the products are added as they come and the sign is restored with the store.
template <bool FUSE_POTRF>
__global__ void __launch_bounds__(256, FUSE_POTRF ? 1 : 2)
syrk_panel_kernel(double* __restrict__ A, int ld, int n, int col0, int kp, int row0, int tc0, int tc1, int ntr,
                  int* __restrict__ info, double* __restrict__ dinv) {
    __shared__ __attribute__((aligned(16))) double Ps[2][2][128][18];   // [buffer][I / J][row][k]
    // tile (ti, tj), tc0 <= tj < tc1, tj <= ti < ntr, numbered column by column
    int t = blockIdx.x, tj = tc0, off = 0;
    while (tj + 1 < tc1 && t >= off + (ntr - tj)) { off += ntr - tj; ++tj; }
    const int ti = tj + (t - off);
    const int ri = row0 + 128 * ti, rj = row0 + 128 * tj;            // first row of P_I / P_J (= first column of the C tile)
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, lk = l >> 4;
    const int wr = w >> 1, wc = w & 1;
    const bool full = ri + 128 <= n;                                 // rj <= ri: the tile needs no row / column guards
    const bool quad = ti > tj || wc <= wr;                           // this wave's quadrant is part of the lower block triangle
    // staging map: thread -> (row sr + 32 pass, 2 consecutive k), 8 threads per 128-byte row slice
    const int sr = tid >> 3, sk = (tid & 7) * 2;
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    f64x2 gi[4], gj[4];
    const double* pI = A + (size_t)(ri + sr) * ld + col0 + sk;
    const double* pJ = A + (size_t)(rj + sr) * ld + col0 + sk;
    const size_t rs = (size_t)32 * ld;
    auto fetch = [&](int k0) {
        if (full) {
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) {
                gi[ps] = *reinterpret_cast<const f64x2*>(pI + ps * rs + k0);
                gj[ps] = *reinterpret_cast<const f64x2*>(pJ + ps * rs + k0);
            }
        } else {
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) {
                const int r = sr + 32 * ps;
                gi[ps] = (ri + r < n) ? *reinterpret_cast<const f64x2*>(pI + ps * rs + k0) : f64x2{0.0, 0.0};
                gj[ps] = (rj + r < n) ? *reinterpret_cast<const f64x2*>(pJ + ps * rs + k0) : f64x2{0.0, 0.0};
            }
        }
    };
    auto stage = [&](int b) {
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            const int r = sr + 32 * ps;
            *reinterpret_cast<f64x2*>(&Ps[b][0][r][sk]) = gi[ps];
            *reinterpret_cast<f64x2*>(&Ps[b][1][r][sk]) = gj[ps];
        }
    };
    fetch(0);
    // accumulators start from -C (rows ri + 64 wr + 16 m + lk + 4 i, columns rj + 64 wc + 16 nn + lr)
    double* Cw = A + (size_t)(ri + 64 * wr + lk) * ld + rj + 64 * wc + lr;
    v4f64 acc[4][4];
    if (full && quad) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double* row = Cw + (size_t)(16 * m + 4 * i) * ld;
#pragma unroll
                for (int nn = 0; nn < 4; ++nn) acc[m][nn][i] = -row[16 * nn];
            }
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nn = 0; nn < 4; ++nn)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = ri + 64 * wr + 16 * m + lk + 4 * i, c = rj + 64 * wc + 16 * nn + lr;
                    acc[m][nn][i] = (quad && r < n && c < n) ? -A[(size_t)r * ld + c] : 0.0;
                }
    }
    stage(0);
    __syncthreads();
    const int nslices = kp / 16;
    for (int sl = 0; sl < nslices; ++sl) {
        const int b = sl & 1;
        if (sl + 1 < nslices) fetch(16 * (sl + 1));
        if (quad) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                double a[4], bb[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) a[m] = Ps[b][0][64 * wr + 16 * m + lr][4 * kk + lk];
#pragma unroll
                for (int nn = 0; nn < 4; ++nn) bb[nn] = Ps[b][1][64 * wc + 16 * nn + lr][4 * kk + lk];
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int nn = 0; nn < 4; ++nn) acc[m][nn] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], bb[nn], acc[m][nn], 0, 0, 0);
            }
        }
        if (sl + 1 < nslices) stage(b ^ 1);
        __syncthreads();
    }
    // The first tile holds the diagonal block of the NEXT panel in the quadrant of wave 0: it is complete now, so it is
    // factorised on the spot (potrf_tile_lds_wg, all four waves) instead of by a launch of its own.
    if (FUSE_POTRF && t == 0 && tc0 == 0 && dinv) {
        double (*Ls)[66] = reinterpret_cast<double (*)[66]>(&Ps[0][0][0][0]);     // 64 x 66 doubles: fits the staging buffers
        if (w == 0) {
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int nn = 0; nn < 4; ++nn)
#pragma unroll
                    for (int i = 0; i < 4; ++i) Ls[16 * m + lk + 4 * i][16 * nn + lr] = -acc[m][nn][i];
        }
        __syncthreads();
        const double rinv = potrf_tile_lds_wg<66>(Ls, tid, row0 / 64, info);
        if (w == 0) {
            dinv[row0 + l] = rinv;
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int nn = 0; nn < 4; ++nn)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[m][nn][i] = -Ls[16 * m + lk + 4 * i][16 * nn + lr];
        }
    }
    // only block columns <= block rows belong to the factorisation: the upper 64-block of a diagonal tile is left alone
    if (full && quad) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double* row = Cw + (size_t)(16 * m + 4 * i) * ld;
#pragma unroll
                for (int nn = 0; nn < 4; ++nn) row[16 * nn] = -acc[m][nn][i];
            }
    } else if (quad) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nn = 0; nn < 4; ++nn)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = ri + 64 * wr + 16 * m + lk + 4 * i, c = rj + 64 * wc + 16 * nn + lr;
                    if (r < n && c < n) A[(size_t)r * ld + c] = -acc[m][nn][i];
                }
    }
}

}  // namespace alabi
