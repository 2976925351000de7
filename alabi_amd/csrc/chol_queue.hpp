// Task-queue factorisation for 3..256 block columns (the default for all of them, N = 129..16384: ALABI_CHOL_W8_MIN_NB,
// ALABI_CHOL_TASKS_MAX_NB, cholesky_tasks_prepare): ONE launch instead of 2 nb - 1.  This file is the queue's device code;
// the task record and its type encoding are in chol_tasks.hpp, the lists in chol_tasklist.hip, the launchers in gp_cholesky.hip,
// of which this header is a part (one translation unit for all Cholesky device code, see there).
//
// The launch-per-step path (chol_steps.hpp) is a chain of dependent kernels: per block column a panel solve (11 us) and an update with
// the next diagonal factorisation fused in (19.6 us), each behind a kernel boundary -- 1.02 ms at N = 2000 for 2.67 GFLOP.
// Here the same 64 x 64 tile operations are TASKS in a static topological order; persistent workgroups draw the next task
// index from one atomic counter, wait (bounded) until the tile versions it depends on have been published, run it and
// publish its own tile version.  A workgroup only ever waits for tasks with a smaller index, and every drawn task is held by
// a running workgroup, so the queue cannot deadlock even when not all workgroups are resident.  Hand-off between workgroups:
// tiles are written with write-through (sc1) stores, every wave drains its stores, one barrier, then ONE lane publishes
// the tile's version with an sc1 store; readers poll the version words and read the tiles with sc1 loads
// (cdna_hip_programming.md Guideline 16, R1 with sc1 loads in place of the acquire).
//   CHAIN(k)      k >= 1: solve tile (k, k-1) against L[k-1,k-1], publish it, apply it to tile (k, k) and factorise that
//                 tile on the spot -- the whole critical path of a block column in ONE workgroup without leaving LDS;
//                 CHAIN(0) factorises tile (0, 0).
//   TRSM(i, k)    i >= k + 2: the other tiles of the panel.
//   UPDATE(i,j,k) tile (i, j) -= tile (i, k) tile (j, k)^T for i >= j > k except (k+1, k+1).
// Order per block column k: CHAIN(k+1) first, then the panel solves, then the updates of column k+1 (the next chain's
// inputs), then the rest -- the chain never queues behind bulk updates.  ver[i][j] = number of steps applied to tile (i, j);
// j + 1 means final.
//
// Control words (`ctl`, cleared by the assembly kernel that runs just before; cholesky_tasks_prepare sizes them):
//   [0]                   head of the queue: the next task index, drawn with one atomicAdd per task
//   [1]                   time-out flag
//   [2 + i nb + j]        ver[i][j], the tile versions
//   [2 + nb nb + k]       sver[k]: slabs of L[k,k] published so far (0..4)
//   then 130 words        alignment + the phase timers of an ALABI_CHOL_PROF build
//   then, 8-byte aligned  the slab buffers, [nb][4][64][16] doubles: what the panel solves read of a diagonal tile (ct_solve).  The
//                         assembly kernel fills them with ALABI_CHOL_TAG; a piece counts as published once it no longer carries the tag.
// Batched queue (chol_batch_prepare): [32 q] head of list q (q < nlists <= 8, a 128-byte line each), [1] time-out flag, from [256] on
// per matrix its tile versions and slab counters (CholMat::ver / sver); the slab buffers are an allocation of their own and are NOT
// tagged -- the batch polls the slab counters.
// Time-out: every wait is bounded by `spin_limit` polls (ALABI_CHOL_SPIN_LIMIT).  The workgroup whose wait runs out sets ctl[1] and leaves;
// the others find the flag set while they wait and leave too.  The matrix (every matrix of a batch) is then in an UNDEFINED state: the
// caller reads ctl[1] after its synchronisation and, if it is set, assembles and factorises again on the launch-per-step path
// (alabi_gp_compute in api.hip, gp_batch.hip).  The queue cannot deadlock, so this is a guard against a fault, not a regular exit.
//
// NT = 256: four waves, one per SIMD, up to 512 registers per lane (the shape the chain-bound sizes were tuned on).
// NT = 512 (round 3, many block columns): four HELPER waves join for the UPDATE tasks -- two matrix-core waves per SIMD (66-70
// instead of 56-59 TFLOP/s of v_mfma_f64_16x16x4, tools/micro/mfma_f64_rate), wave w owning rows 16 (w & 3).., columns
// 32 (w >> 2).. of the tile -- and for every tile load / store; in the serial parts of CHAIN and TRSM tasks they only keep the
// barriers company, so the chain runs as fast as with four waves (two workgroups of four waves per CU were measured instead:
// the grouped updates gained 27 %, but every recurrence that shared its SIMD with the other workgroup's matrix-core
// instructions took 1.5-1.8x as long and the singles waited five times longer for their inputs; N = 10000 9.86 -> 9.59 ms only).
// BATCH: the queue holds the interleaved task lists of many independent matrices (the hyper-parameter search: candidates x folds,
// gp_utils.py:511-700).  A task names its matrix (`mats`); the queue is cut into `nlists` lists, each with a head counter of its own
// on a 128-byte line of its own (ctl[32 q]; one word saturates at ~88 draws per microsecond, MI355X_MICROARCH.md `dequeue`) and each
// holding whole matrices, so a matrix's tiles stay in one XCD's L2: a workgroup starts on the list of its XCD and moves on to the
// next list when one is exhausted.  Every list is a topological order of its own tasks and a workgroup only waits for tasks in
// front of the one it drew, each of them drawn by a running workgroup: no deadlock, whatever the placement.
#pragma once
#include <type_traits>
#include "chol_tasks.hpp"
#include "chol_tiles.hpp"

namespace alabi {

// Every coherent load / store of the queue names the GLOBAL address space: inside the non-inlined phase functions, and in the batched
// kernel (whose matrix pointers are loaded from a table), the pointers are generic to the compiler and the accesses became flat_load /
// flat_store -- the slab stores of the diagonal factorisation took 0.1 us each.
typedef __attribute__((address_space(1))) unsigned long long* ct_gptr64;
typedef __attribute__((address_space(1))) int* ct_gptr32;
__device__ inline ct_gptr64 ct_g64(const double* p) { return (ct_gptr64)(unsigned long long*)const_cast<double*>(p); }
__device__ inline ct_gptr32 ct_g32(const int* p) { return (ct_gptr32)const_cast<int*>(p); }
// ... and the tiles, slabs and inverse blocks that are handed on go out in 16-byte pieces: a coherent (write-through) store is one fabric
// write per lane, and an 8-byte one costs 2.7x the time per byte of a 16-byte one (MI355X_MICROARCH.md).  A 64-row block at `base` with
// row stride ld as a buffer: (row, column) -> byte offset.
typedef unsigned int ct_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int ct_u32x2 __attribute__((ext_vector_type(2)));
__device__ inline __amdgpu_buffer_rsrc_t ct_block_rsrc(double* base, int ld) {
    return __builtin_amdgcn_make_buffer_rsrc(base, 0, (unsigned)(63 * ld + 64) * 8u, 0x00020000);
}
// the pair (r, c), (r, c + 1) of a block, c even; lower = only what lies on or below the diagonal of the block
__device__ inline void ct_store_pair(__amdgpu_buffer_rsrc_t rs, int ld, int r, int c, ct_u32x4 v, bool lower) {
    const unsigned off = (unsigned)(r * ld + c) * 8u;
    if (!lower || c + 1 <= r) __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, 16);
    else if (c == r) { ct_u32x2 h = {v.x, v.y}; __builtin_amdgcn_raw_buffer_store_b64(h, rs, off, 0, 16); }
}

template <int NT>
__device__ inline void tile_load_sc1(double (*T)[66], const double* __restrict__ src, int ld, int tid) {
#pragma unroll
    for (int e_ = 0; e_ < 4096 / NT; ++e_) {
        const int e = tid + NT * e_, r = e >> 6, c = e & 63;
        T[r][c] = __longlong_as_double((long long)__hip_atomic_load(ct_g64(src + (size_t)r * ld + c),
                                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
}
template <int NT>
__device__ inline void tile_store_sc1(double* __restrict__ dst, int ld, double (*T)[66], int tid, bool lower_only) {
    // every LDS read first, unconditionally, then the stores: written as "if (lower) store(T[r][c])" the compiler reads, waits and stores
    // element by element under the predicate -- 16 LDS round trips in a row
    const __amdgpu_buffer_rsrc_t rs = ct_block_rsrc(dst, ld);
    ct_u32x4 v[2048 / NT];
#pragma unroll
    for (int e_ = 0; e_ < 2048 / NT; ++e_) {
        const int e = tid + NT * e_;
        v[e_] = *reinterpret_cast<const ct_u32x4*>(&T[e >> 5][2 * (e & 31)]);
    }
#pragma unroll
    for (int e_ = 0; e_ < 2048 / NT; ++e_) asm volatile("" : "+v"(v[e_]));
#pragma unroll
    for (int e_ = 0; e_ < 2048 / NT; ++e_) {
        const int e = tid + NT * e_;
        ct_store_pair(rs, ld, e >> 5, 2 * (e & 31), v[e_], lower_only);
    }
}
// every wave has drained its stores and passed the barrier before ONE lane publishes the version
__device__ inline void publish_version(int* ver, int value, int tid) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_store(ct_g32(ver), value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Module-scope LDS, named directly by the non-inlined phase functions (as pointer arguments they would degrade to generic
// pointers).  The panel solve and the diagonal factorisation are separate noinline functions: inlined into the task loop their
// live ranges merge with the loop's and the serial recurrences fill up with AGPR moves (8.6 / 13.1 us instead of 5 / 9).
__shared__ double ct_pool[8 * 64 * 34];                               // one array: four 64 x 66 tiles, or (UPDATE2 / UPDATE4) six / eight 64 x 34 half tiles
#define ct_T0 (reinterpret_cast<double (*)[66]>(ct_pool))
#define ct_T1 (reinterpret_cast<double (*)[66]>(ct_pool + 64 * 66))
#define ct_T2 (reinterpret_cast<double (*)[66]>(ct_pool + 2 * 64 * 66))   // CHAIN: the diagonal tile, parked while the panel tile is solved
#define ct_T3 (reinterpret_cast<double (*)[66]>(ct_pool + 3 * 64 * 66))   // UPDATE over several block columns: second operand pair (T2, T3)
__shared__ int ct_task_s[16];                                          // the task loop's words (chol_tasks_body) + [9]: slabs of L[kk,kk] seen by a solve
#ifdef ALABI_CHOL_LOG
// Event log of the CHAIN tasks (tools/run_chol_log.sh): 10-ns time stamps written with plain stores by thread 0 -- no read-modify-write on
// the chain, unlike the ALABI_CHOL_PROF counters.  [k][0] drawn, [1] dependencies met, [2] tiles in LDS, [3..6] slab s of L[k-1,k-1] seen,
// [7] solve + diagonal update done, [8] panel tile published, [9] factorisation starts, [10..13] slab recurrence s done, [14] last inverse
// block out, [15] tile stored and published.
__device__ long long g_chain_log[256][32];   // [16 + 2 s] / [17 + 2 s]: factorisation past barrier A / B of slab s
__shared__ int ct_log_kb;
#define CT_LOG(i) do { if (threadIdx.x == 0) g_chain_log[ct_log_kb][i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define CT_LOGW(i) do { if ((threadIdx.x & 63) == 0) g_chain_log[ct_log_kb][i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define CT_LOGW(i) do { } while (0)
#define CT_LOG(i) do { } while (0)
#endif
// Lower-triangle tile j of the 4 x 4 grid of 16 x 16 tiles of a diagonal tile: (0,0) (1,0) (1,1) (2,0) (2,1) (2,2) (3,0) .. (3,3)
__device__ inline void ct_diag_tile(int j, int& rt, int& ct) { rt = j >= 6 ? 3 : j >= 3 ? 2 : j >= 1 ? 1 : 0; ct = j - rt * (rt + 1) / 2; }
// What a panel solve needs of L[kk,kk] travels through the column's SLAB BUFFER, sbuf[4][64][16] doubles (32 KB per block column, beside the
// matrix): slab s holds, in rows 16 s .. 16 s + 15, the INVERSE of the slab's diagonal block and below them the slab's columns of L (rows above
// are unused) -- contiguous, in 16-byte pieces, piece e of a slab = row e >> 3, columns 2 (e & 7) ..  The solve never reads L[s,s] itself; in
// ct_T0 the inverse stands in its place.
#define ALABI_CHOL_TAG 0x7FF8DEADu   // both 32-bit halves of a "not written yet" double of the slab buffer: a NaN no arithmetic produces
template <int NT>
__device__ inline ct_u32x4 ct_slab_piece(__amdgpu_buffer_rsrc_t rs, int q, int e) {
    return __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)(q * 1024 + 2 * e) * 8u, 0, 16);
}
__device__ inline void ct_slab_piece_put(int q, int e, ct_u32x4 v) { *reinterpret_cast<ct_u32x4*>(&ct_T0[e >> 3][16 * q + 2 * (e & 7)]) = v; }
// the slabs [s0, s1) into ct_T0 in ONE memory round trip (a coherent load takes 0.7-1 us, whatever it fetches); run-time bounds: one copy of the code
template <int NT>
__device__ inline void ct_fetch_slabs(const double* __restrict__ sbuf, int tid, int s0, int s1) {
    constexpr int NE = 512 / NT;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(sbuf), 0, 32768u, 0x00020000);
    ct_u32x4 v[4][NE];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (q >= s0 && q < s1) {
#pragma unroll
            for (int e_ = 0; e_ < NE; ++e_) {
                const int e = tid + NT * e_;
                if ((e >> 3) >= 16 * q) v[q][e_] = ct_slab_piece<NT>(rs, q, e);
            }
        }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (q >= s0 && q < s1) {
#pragma unroll
            for (int e_ = 0; e_ < NE; ++e_) {
                const int e = tid + NT * e_;
                if ((e >> 3) >= 16 * q) ct_slab_piece_put(q, e, v[q][e_]);
            }
        }
}
// Panel solve X L_kk^T = B of the tile in ct_T1 ENTIRELY ON THE MATRIX CORES (round 4; before: a 16-step recurrence per slab in one
// wave, 1.8 us per slab, 7.2 us per tile -- 30 % of the workgroup time of a batch of N = 1600 matrices and the tail of every CHAIN).
// The diagonal factorisation publishes, per 16-column slab s, the inverse of the slab's 16 x 16 diagonal block (ct_potrf_publish:
// wave 1 runs the slab's recurrence on the block's rows and on the rows of the identity beside wave 0, so the inverse costs the
// chain nothing); with it
//     X_s = (B_s - sum_{u<s} X_u L_su^T) inv(L_ss)^T.
// Wave w (< 4) owns rows 16 w .. of the tile and works on the TRANSPOSE, Y = X^T: Y_s = inv(L_ss) (B_s^T - sum_u L_su Y_u).  Then the
// result of a product (C/D layout: row 4 i + (lane >> 4), column lane & 15) is, register i for k-step i, exactly the B operand of the
// next one (B[k = lane >> 4][n = lane & 15]), so the four slab steps chain in registers: 4 + 4 (3 - s) matrix-core instructions per slab
// and wave, 40 per tile = 1.1 us, no cross-lane traffic and no barrier between the slabs.  The slabs of L[kk,kk] are taken as they are
// published (sver[kk] = slabs available; all that are there in ONE fetch when the tile is final).  Error of a slab: that of a product
// with the explicit inverse of a 16 x 16 block, eps cond(L_ss) -- the blocks are small, tests hold ||L L^T - K|| <= 1e-12 ||K||.
// (Measured and not kept: the LAST inverse block polled itself -- pre-filled with a tag by the assembly kernel, valid once it differs -- instead
// of through the slab counter, one memory round trip instead of three behind the producer's last store: N = 2000 0.492 vs 0.495 ms.  The event
// log (ALABI_CHOL_LOG) shows why: the next CHAIN task gets its own tiles only 3 us before the previous factorisation ends -- they come from
// the single-column updates behind the previous panel solve -- and then works through the slabs at two round trips each, poll and fetch:
// slab 2 is in LDS 2 us AFTER that end, whatever the last block does.)
// DIAG (CHAIN): tile (k,k), parked in ct_T2, takes - X X^T slab by slab behind the solve (its ten lower 16 x 16 tiles dealt to all
// waves, accumulators in registers) and ends up in ct_T0 for the factorisation; the solved tile is written to Xdst while the last
// of that runs.  Returns false when a wait ran out (err set, every thread leaves).
// TAG (single matrix): no counter is polled at all.  The assembly kernel fills the slab buffers with a tag; the solve requests ALL FOUR slabs
// at once when it starts, and a slab counts as there when none of its pieces carries the tag any more (8 bytes at a time; a piece that
// does is requested again) -- one memory round trip behind the producer's stores instead of three (drain + counter, poll, fetch), and the
// slabs that were there already cost no round trip of their own.  (The event log, ALABI_CHOL_LOG, had shown the chain's next step getting its
// own tiles only 3 us before the previous factorisation ended, and then working through the slabs at two round trips each: the last slab was in
// LDS 4 us after that end.)  !TAG (batch): sver[kk] = slabs published so far, polled; everything that is there fetched in one round trip.
template <int NT, bool DIAG, bool TAG>
__device__ __attribute__((noinline)) bool ct_solve(int ld, const double* __restrict__ sbuf, int* sver, int* err,
                                                   int spin_limit, int ntasks, double* __restrict__ Xdst) {
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, lk = l >> 4;
    constexpr int NW = NT / 64, NQ = (10 + NW - 1) / NW;       // lower 16 x 16 tiles of the diagonal tile per wave: 3 (four waves) / 2 (eight)
    constexpr int NE = 512 / NT;                               // 16-byte pieces of a slab per thread
    v4f64 Y[4], dacc[NQ];
    int have = 0;                                              // slabs of L[kk,kk] in ct_T0
    ct_u32x4 pv[4][NE];
    const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(sbuf), 0, 32768u, 0x00020000);
    if constexpr (TAG) {
        if (tid == 0) ct_task_s[15] = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e_ = 0; e_ < NE; ++e_) {
                const int e = tid + NT * e_;
                if ((e >> 3) >= 16 * q) pv[q][e_] = ct_slab_piece<NT>(prs, q, e);
            }
    }
    auto slab = [&](auto s_tag) -> bool {
        constexpr int S = decltype(s_tag)::value;
        if constexpr (TAG) {
            int spins = 0;
            for (;;) {
                bool good = true;
#pragma unroll
                for (int e_ = 0; e_ < NE; ++e_) {
                    const int e = tid + NT * e_;
                    const ct_u32x4 v = pv[S][e_];
                    if ((e >> 3) >= 16 * S && ((v.x == ALABI_CHOL_TAG && v.y == ALABI_CHOL_TAG) || (v.z == ALABI_CHOL_TAG && v.w == ALABI_CHOL_TAG))) good = false;
                }
                if (__all(good)) break;
                if (++spins > spin_limit || ((spins & 63) == 0 && __hip_atomic_load(ct_g32(err), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                    if (l == 0) { __hip_atomic_store(ct_g32(err), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); ct_task_s[4] = ntasks; ct_task_s[15] = 1; }
                    break;
                }
                asm volatile("" ::: "memory");                   // (a fresh load every time round: the builtin is not volatile)
#pragma unroll
                for (int e_ = 0; e_ < NE; ++e_) {
                    const int e = tid + NT * e_;
                    if ((e >> 3) >= 16 * S) pv[S][e_] = ct_slab_piece<NT>(prs, S, e);
                }
            }
#pragma unroll
            for (int e_ = 0; e_ < NE; ++e_) {
                const int e = tid + NT * e_;
                if ((e >> 3) >= 16 * S) ct_slab_piece_put(S, e, pv[S][e_]);
            }
            __syncthreads();                                   // the slab -- and at S = 0 the caller's tiles -- are in LDS
            if (ct_task_s[15] != 0) return false;
            if constexpr (DIAG) CT_LOG(3 + S);
            have = S + 1;
        }
        if (have <= S) {
            if (tid == 0) {
                int v, spins = 0;
                while ((v = __hip_atomic_load(ct_g32(sver), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < S + 1) {
                    if (++spins > spin_limit || ((spins & 63) == 0 && __hip_atomic_load(ct_g32(err), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                        __hip_atomic_store(ct_g32(err), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        ct_task_s[4] = ntasks;
                        v = -1;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                ct_task_s[9] = v;
            }
            __syncthreads();
            const int got = ct_task_s[9];
            if (got < 0) return false;
            have = got < 4 ? got : 4;                          // everything that is there, in one round trip
            ct_fetch_slabs<NT>(sbuf, tid, S, have);
            __syncthreads();                                   // the slab(s) -- and at S = 0 the caller's tiles -- are in LDS
            if constexpr (DIAG) { for (int q_ = S; q_ < have; ++q_) CT_LOG(3 + q_); }
        }
        if (w < 4) {
            if (S == 0) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int i = 0; i < 4; ++i) Y[t][i] = ct_T1[16 * w + lr][16 * t + 4 * i + lk];
            }
            v4f64 Z = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) Z = __builtin_amdgcn_mfma_f64_16x16x4f64(ct_T0[16 * S + lr][16 * S + 4 * kk + lk], Y[S][kk], Z, 0, 0, 0);
#pragma unroll
            for (int t = S + 1; t < 4; ++t)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    Y[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ct_T0[16 * t + lr][16 * S + 4 * kk + lk], Z[kk], Y[t], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) ct_T1[16 * w + lr][16 * S + 4 * i + lk] = Z[i];
        }
        if constexpr (DIAG) {
            __syncthreads();                                   // slab S of X is in ct_T1 for all 64 rows (and nobody reads ct_T0's slab S any more)
            if (S == 3) tile_store_sc1<NT>(Xdst, ld, ct_T1, tid, false);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int j = w + NW * q;
                if (j < 10) {
                    int rt, ct;
                    ct_diag_tile(j, rt, ct);
                    if (S == 0) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) dacc[q][i] = ct_T2[16 * rt + lk + 4 * i][16 * ct + lr];
                    }
#pragma unroll
                    for (int kq = 0; kq < 4; ++kq) {
                        const int ks = 4 * S + kq;
                        dacc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ct_T1[16 * rt + lr][4 * ks + lk], ct_T1[16 * ct + lr][4 * ks + lk], dacc[q], 0, 0, 0);
                    }
                    if (S == 3) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) ct_T0[16 * rt + lk + 4 * i][16 * ct + lr] = dacc[q][i];
                    }
                }
            }
        }
        return true;
    };
    if (!slab(std::integral_constant<int, 0>{})) return false;
    if (!slab(std::integral_constant<int, 1>{})) return false;
    if (!slab(std::integral_constant<int, 2>{})) return false;
    if (!slab(std::integral_constant<int, 3>{})) return false;
    if constexpr (!DIAG) {
        __syncthreads();
        tile_store_sc1<NT>(Xdst, ld, ct_T1, tid, false);
    }
    return true;
}
// The diagonal factorisation of CHAIN(k) (potrf_tile_lds_wg on ct_T0) that hands its result on SLAB BY SLAB: the 16 columns
// of a slab are final for all 64 rows as soon as wave 0 has run the slab's recurrence, and the panel solve of the next chain
// task consumes L[k,k] in exactly that order -- so wave 3, idle while wave 0 runs the next recurrence, writes the slab (and
// its 16 reciprocals) through to memory and, one barrier later when its stores have drained, publishes sver[k] = slab + 1.
// The next CHAIN task then solves slab s while this one factorises slab s + 1 .. 3 instead of starting after the whole tile.
#ifdef ALABI_CHOL_PROF
__device__ long long g_potrf_prof[8];                          // 10-ns ticks inside wave 0's slab recurrences, slabs; [2] start -> barrier A, [3] A -> B, [4] last slab incl. its stores, [5] count
#endif
// The inverses of the slabs' 16 x 16 diagonal blocks, which the matrix-core panel solves multiply by (ct_solve), cost the chain nothing:
//   slabs 1..3: lanes 0..15 of wave 0 -- rows above the slab, idle in its recurrence -- carry the rows of the identity through the SAME
//     recurrence (x L_ss^T = e_i by forward substitution) and come out as the rows of inv(L_ss)^T; the last block, all the next panel solve
//     waits for at the end, goes out at once, the others with their slab;
//   slab 0 (no idle lanes): wave 0 gives up rows 48..63 for the identity, and wave 1 runs the same recurrence beside it for those rows
//     (lanes 16..31; its lanes 0..15 repeat rows 0..15, the source of the multipliers, bit for bit).
// The function must stay within the caller-saved registers and call nothing: with a substitution of ~215 live registers inside it (or a
// call to one) every CHAIN task saved and restored up to 79 registers through scratch memory -- the factorisation took 12-13 us instead of 9.
// (Also measured and not kept: ONE non-inlined copy of the recurrence for every slab, with the slab offset at run time: 1.52 instead of
// 1.26 us per slab.)
// Inside the function the waves do not meet at barriers but follow each other through LDS words (ct_task_s[10..14]; every wait bounded):
//   wave 0          the four slab recurrences; before recurrence s it waits until tile column s carries slab s - 1 ([12])
//   wave 1          slab 0: rows 48..63 behind a copy of rows 0..15 ([13]: 1 = rows read, 2 = rows written back); then owner A
//   owners A, B, C  (waves 1, 2 and 6 -- with four waves 3) the rank-16 updates of the trailing 16 x 16 tiles, every slab of a tile by ONE
//                   wave in order: A (1,1) (2,2), B (2,1) (3,2), C (3,1) (3,3).  When slab s is in LDS ([11] = s + 1) an owner first updates its
//                   tile of column s + 1 -- all the next recurrence needs; counted in [12] -- then its tiles further right, under that recurrence
//   waves 3 (and 7) write slab s -- rows 16 s.., its columns (lower part), the inverse of its diagonal block, its reciprocals -- through to
//                   memory in 16-byte pieces, wait for the stores to drain ([10]: wave 7's half) and publish sver = s + 1 ([14]: inverse
//                   blocks read, before wave 0 reuses the buffer)
// With two barriers per slab instead -- recurrence | stores + every trailing tile | next recurrence -- all eight waves waited 0.6-1.0 us
// per slab for the two storing waves (write-through stores hold the issuing wave), the factorisation took 9.9 us for 4.8 us of recurrences.
// Spinning waves share no SIMD with the recurrences of waves 0 and 1 (waves 4 and 5 sleep at the final barrier).
#define CT_FLAG(i) (*(volatile __attribute__((address_space(3))) int*)&ct_task_s[i])
__device__ inline bool ct_flag_wait(int i, int want, bool sleep) {
    int spins = 0;
    while (CT_FLAG(i) < want) {
        if (++spins > (1 << 22)) return false;                 // (a protocol error, not a slow neighbour: every wave here makes progress on its own)
        if (sleep) __builtin_amdgcn_s_sleep(1);
    }
    asm volatile("" ::: "memory");
    return true;
}
__device__ inline void ct_flag_set(int i, int v, int lane) {      // (LDS operations of one wave are executed in order: the data first)
    asm volatile("" ::: "memory");
    if (lane == 0) CT_FLAG(i) = v;
}
__device__ inline void ct_flag_add(int i, int lane) {
    asm volatile("" ::: "memory");
    if (lane == 0) __hip_atomic_fetch_add(&ct_task_s[i], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __attribute__((noinline)) double ct_potrf_publish(int kb, int* info, double* __restrict__ D, int ld, double* __restrict__ dinv,
                                                            int* sver, double* __restrict__ linv, int* err) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool eight = blockDim.x == 512;
    double* const inv_s = ct_pool + 3 * 64 * 66;              // T3: inverses of the slabs' diagonal blocks, [slab & 1][n][k]
    kb = __builtin_amdgcn_readfirstlane(kb);
    if (tid < 5) ct_task_s[10 + tid] = 0;
    __syncthreads();
    bool ok = true;
    // one owner's share of slab S: its tile of column S + 1 first (counted), then its tiles further right
    auto owner_slab = [&](auto s_tag, int which) {
        constexpr int S = decltype(s_tag)::value;
        if (!ct_flag_wait(11, S + 1, true)) { ok = false; return; }
        const int t1r = which + 1, t2r = which == 0 ? 2 : 3, t2c = which == 2 ? 3 : 2;    // (t1r, 1) and (t2r, t2c)
        if (S == 0) {
            tile_update_16<66>(ct_T0, 16 * t1r, 16, ct_T0, 16 * t1r, ct_T0, 16, 0, lane);
            ct_flag_add(12, lane);
            tile_update_16<66>(ct_T0, 16 * t2r, 16 * t2c, ct_T0, 16 * t2r, ct_T0, 16 * t2c, 0, lane);
        } else if (t2c == S + 1) {
            tile_update_16<66>(ct_T0, 16 * t2r, 16 * t2c, ct_T0, 16 * t2r, ct_T0, 16 * t2c, 16 * S, lane);
            ct_flag_add(12, lane);
        } else if (t2c > S + 1) {
            tile_update_16<66>(ct_T0, 16 * t2r, 16 * t2c, ct_T0, 16 * t2r, ct_T0, 16 * t2c, 16 * S, lane);
        }
    };
    // the storing waves' share of slab S
    auto store_slab = [&](auto s_tag) {
        constexpr int S = decltype(s_tag)::value;
        constexpr int c0 = 16 * S;
        if (!ct_flag_wait(11, S + 1, true)) { ok = false; return; }
        if (w == 7) CT_LOGW(16 + 4 * S);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(linv, 0, 32768u, 0x00020000);   // the column's slab buffer
        ct_u32x4 v[8];                                         // every LDS read first (see tile_store_sc1); piece e = lane + 64 p_: row e >> 3 >= c0
        double dl = 1.0;
#pragma unroll
        for (int p_ = 2 * S; p_ < 8; ++p_) {
            const int e = lane + 64 * p_, r = e >> 3, c = 2 * (e & 7);
            if (p_ < 2 * S + 2) { if (w == 3) v[p_] = *reinterpret_cast<const ct_u32x4*>(&inv_s[256 * (S & 1) + (r - c0) * 16 + c]); }   // rows c0 .. c0 + 15: the inverse block (wave 3 alone: [14])
            else v[p_] = *reinterpret_cast<const ct_u32x4*>(&ct_T0[r][c0 + c]);
        }
        if (w == 3) dl = ct_T0[c0 + (lane & 15)][c0 + (lane & 15)];
#pragma unroll
        for (int p_ = 2 * S; p_ < 8; ++p_) asm volatile("" : "+v"(v[p_]));
        if (w == 3) ct_flag_set(14, S + 1, lane);
        if (w == 7) CT_LOGW(17 + 4 * S);
#pragma unroll
        for (int p_ = 2 * S; p_ < 8; ++p_) {
            const int e = lane + 64 * p_;
            if (p_ < 2 * S + 2 ? w == 3 : (!eight || (p_ & 1) == (w >> 2))) __builtin_amdgcn_raw_buffer_store_b128(v[p_], rs, (unsigned)(S * 1024 + 2 * e) * 8u, 0, 16);
        }
        if (w == 3 && lane < 16)
            __hip_atomic_store(ct_g64(dinv + kb * 64 + c0 + lane), (unsigned long long)__double_as_longlong(potrf_dinv(dl)),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (w == 7) CT_LOGW(18 + 4 * S);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (w == 7) CT_LOGW(19 + 4 * S);
        if (w == 7) ct_flag_set(10, S + 1, lane);
        else {
            if (eight && !ct_flag_wait(10, S + 1, true)) { ok = false; return; }
            if (lane == 0) __hip_atomic_store(ct_g32(sver), S + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (S == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // in front of the "4" below
        }
    };
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
    if (w == 0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int c0 = 16 * s;
            if (s > 0 && ok) ok = ct_flag_wait(12, s == 1 ? 3 : s == 2 ? 5 : 6, false);   // tile column s carries slab s - 1
            double a[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) a[j] = ct_T0[lane][c0 + j];
            {                                                  // rows of the identity: lanes 0..15 (slab 0: lanes 48..63, wave 1 has those rows)
                const int il = s > 0 ? lane : lane - 48;
#pragma unroll
                for (int j = 0; j < 16; ++j) a[j] = (il >= 0 && il < 16) ? (j == il ? 1.0 : 0.0) : a[j];
            }
            potrf_slab(a, c0);
            CT_LOG(10 + s);
            if (s == 0 && ok) ok = ct_flag_wait(13, 1, false);        // wave 1 has read rows 0..15 before they are written back
            if (s >= 2 && ok) ok = ct_flag_wait(14, s - 1, false);    // wave 3 has read block s - 2 out of this half of the buffer
            if (s > 0 ? lane < 16 : lane >= 48) {
#pragma unroll
                for (int j = 0; j < 16; ++j) inv_s[256 * (s & 1) + j * 16 + (lane & 15)] = a[j];   // identity lane i holds row i of inv(L_ss)^T
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) ct_T0[lane][c0 + j] = a[j];
            }
            if (s == 0 && ok) ok = ct_flag_wait(13, 2, false);        // rows 48..63 of slab 0 are in LDS too
            if (s < 3) ct_flag_set(11, s + 1, lane);
            else {                                             // the last inverse block is all the next panel solve waits for: out at once
                const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc(linv, 0, 32768u, 0x00020000);
                ct_u32x4 iv[2];
#pragma unroll
                for (int q = 0; q < 2; ++q) iv[q] = *reinterpret_cast<const ct_u32x4*>(&inv_s[256 + 2 * (lane + 64 * q)]);
#pragma unroll
                for (int q = 0; q < 2; ++q) asm volatile("" : "+v"(iv[q]));
#pragma unroll
                for (int q = 0; q < 2; ++q)                    // slab 3 of the slab buffer, rows 48..63
                    __builtin_amdgcn_raw_buffer_store_b128(iv[q], rl, (unsigned)(3 * 1024 + 48 * 16 + 2 * (lane + 64 * q)) * 8u, 0, 16);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                CT_LOG(14);
            }
        }
    } else if (w == 1) {
        {                                                      // rows 48..63 of slab 0 (lanes 16..31) behind a copy of rows 0..15 (lanes 0..15)
            double a[16];
            const int row = (lane & 16) ? 48 + (lane & 15) : (lane & 15);
#pragma unroll
            for (int j = 0; j < 16; ++j) a[j] = ct_T0[row][j];
#pragma unroll
            for (int j = 0; j < 16; ++j) asm volatile("" : "+v"(a[j]));   // (the loads have landed)
            ct_flag_set(13, 1, lane);
            potrf_slab(a, 0);
            if (lane >= 16 && lane < 32) {
#pragma unroll
                for (int j = 0; j < 16; ++j) ct_T0[row][j] = a[j];
            }
            ct_flag_set(13, 2, lane);
        }
        owner_slab(I0{}, 0); owner_slab(I1{}, 0);
    } else if (w == 2) {
        owner_slab(I0{}, 1); owner_slab(I1{}, 1);
    } else if (eight ? w == 6 : w == 3) {
        owner_slab(I0{}, 2); if (!eight) store_slab(I0{});
        owner_slab(I1{}, 2); if (!eight) store_slab(I1{});
        owner_slab(I2{}, 2); if (!eight) store_slab(I2{});
    } else if (w == 3 || w == 7) {
        store_slab(I0{}); store_slab(I1{}); store_slab(I2{});
    }
    if (!ok && lane == 0) __hip_atomic_store(ct_g32(err), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    // every slab and every inverse block is out (wave 3 drained slab 2 before it published it, wave 0 block 3 above): the panel solves
    // need nothing else of this tile -- not the last diagonal block, which goes out with the whole tile behind this
    if (tid == 0) __hip_atomic_store(ct_g32(sver), 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (w != 0) return 1.0;
    const double lll = ct_T0[lane][lane];
    const int bad = potrf_first_bad(lll);
    if (bad != 0 && lane == 0) atomicCAS(info, 0, kb * 64 + bad);
    return potrf_dinv(lll);
}
// A tile in flight: all 16 loads of a thread are issued before the first one is consumed (several tiles are fetched
// back to back and only then written to LDS: one memory round trip instead of one per tile)
template <int NT> struct TileRegs { unsigned long long v[4096 / NT]; };
template <int NT>
__device__ inline void tile_fetch(TileRegs<NT>& r, const double* __restrict__ src, int ld, int tid) {
#pragma unroll
    for (int e_ = 0; e_ < 4096 / NT; ++e_) {
        const int e = tid + NT * e_;
        r.v[e_] = __hip_atomic_load(ct_g64(src + (size_t)(e >> 6) * ld + (e & 63)), __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
    }
}
template <int NT>
__device__ inline void tile_put(double (*T)[66], const TileRegs<NT>& r, int tid) {
#pragma unroll
    for (int e_ = 0; e_ < 4096 / NT; ++e_) {
        const int e = tid + NT * e_;
        T[e >> 6][e & 63] = __longlong_as_double((long long)r.v[e_]);
    }
}

// The same through 16-byte write-through-coherent (sc1) buffer loads: half the load instructions and twice the bytes per request
// (8-byte sc1 accesses run at 0.54-0.70 of the 16-byte rate, MI355X_MICROARCH.md) -- the operand stream of the bulk updates.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <int NT> struct TileRegs16 { u32x4 v[2048 / NT]; };
// PLAIN: ordinary (L2-cached) loads -- valid behind an agent-scope acquire of the hand-off that published the tile (Guideline 16)
template <bool PLAIN, int NT>
__device__ inline void tile_fetch16(TileRegs16<NT>& r, __amdgpu_buffer_rsrc_t rs, unsigned tile_bytes, int ld, int tid) {
#pragma unroll
    for (int e_ = 0; e_ < 2048 / NT; ++e_) {
        const int e = tid + NT * e_;
        r.v[e_] = __builtin_amdgcn_raw_buffer_load_b128(rs, tile_bytes + (unsigned)(((e >> 5) * ld + 2 * (e & 31)) * 8), 0, PLAIN ? 0 : 16);
    }
}
// element e_ of a tile's registers alone: the grouped updates spread the fetch and the LDS write of the next operands over the
// k-steps of the current block column (one of each per k-step pair) instead of issuing them as a burst around the barrier
template <bool PLAIN, int NT>
__device__ inline void tile_fetch16_one(TileRegs16<NT>& r, int e_, __amdgpu_buffer_rsrc_t rs, unsigned tile_bytes, int ld, int tid) {
    const int e = tid + NT * e_;
    r.v[e_] = __builtin_amdgcn_raw_buffer_load_b128(rs, tile_bytes + (unsigned)(((e >> 5) * ld + 2 * (e & 31)) * 8), 0, PLAIN ? 0 : 16);
}
template <int NT>
__device__ inline void tile_put16_one(double (*T)[66], const TileRegs16<NT>& r, int e_, int tid) {
    const int e = tid + NT * e_;
    *reinterpret_cast<u32x4*>(&T[e >> 5][2 * (e & 31)]) = r.v[e_];
}
template <int NT>
__device__ inline void tile_put16(double (*T)[66], const TileRegs16<NT>& r, int tid) {
#pragma unroll
    for (int e_ = 0; e_ < 2048 / NT; ++e_) {
        const int e = tid + NT * e_;
        *reinterpret_cast<u32x4*>(&T[e >> 5][2 * (e & 31)]) = r.v[e_];
    }
}

// The task loop of the three queue kernels (NT = 256 / 512 threads, BATCH: see the head of this file).
template <int NT, bool BATCH>
__device__ __forceinline__ void chol_tasks_body(double* __restrict__ A_, int ld_, int nb_, const CholTask* __restrict__ tasks, int ntasks,
                                                int* __restrict__ ctl, int* __restrict__ info_, double* __restrict__ dinv_, int spin_limit,
                                                const CholMat* __restrict__ mats, const int* __restrict__ list_off, int nlists) {
    double (*T0)[66] = ct_T0; double (*T1)[66] = ct_T1; double (*T2)[66] = ct_T2; double (*T3)[66] = ct_T3;
    int (&task_s)[16] = ct_task_s;
    // per task in a batch, fixed otherwise
    double* A = A_; int ld = ld_, nb = nb_; int* info = info_; double* dinv = dinv_;
    int* head = ctl; int* err = ctl + 1; int* ver = ctl + 2;          // ver[i * nb + j]
    int* sver = ctl + 2 + nb * nb;                                    // sver[k]: slabs of L[k,k] published so far (0..4)
    double* linv = BATCH ? nullptr : reinterpret_cast<double*>(ctl + ((2 + nb * nb + nb + 130 + 1) & ~1));   // the slab buffers, [nb][4][64][16] (ct_fetch_slabs)
    int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, lk = l >> 4;
    __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc(A, 0, (unsigned)ld * (unsigned)ld * 8u, 0x00020000);
    if constexpr (BATCH) {
        if (tid == 0) {                                               // task_s[6]: current list, [7]: lists found exhausted so far
            int xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
            task_s[6] = (xcc & 15) % nlists;
            task_s[7] = 0;
        }
    }
    // (Measured and not kept, round 3: CHAIN(k) applying block column k-2 to its panel tile itself instead of waiting for the
    // one-column UPDATE(k,k-1,k-2) task -- N = 2000 0.55 -> 0.58 ms with four waves, 0.54 -> 0.55 with eight: the period of the
    // chain is set by the 64-pivot factorisation handing its slabs to the next panel solve, not by that task.)
    // (Round 4, again with the matrix-core panel solves, tools/experiments/chol_chain_fused_lookahead.patch: the event log shows the next CHAIN task
    // receiving its tiles only 2.6 us before the previous factorisation ends -- publish, poll, fetch, 64 k-steps, store, publish, poll, fetch
    // behind the previous panel solve -- so the fused task reaches its dependencies 2.8 us earlier, but its own unpipelined update loop takes
    // 4.7 us against the 1 us the tile fetch took: N = 2000 0.518 instead of 0.488 ms.  A pipelined loop would gain ~0.9 us of 13 per step.)
    // (Measured and not kept: a grouped UPDATE drawing the NEXT task under its last block column, to take the queue's atomic round
    // trip off the workgroup's path -- still deadlock-free, and the four-wave kernel gained 3 % at N >= 5000, but the eight-wave
    // kernel lost 1-9 % at every size: a CHAIN task drawn ahead waits for its holder.)
    for (;;) {
        {
            // the per-thread tile offsets of every task type must not be hoisted out of the task loop (the compiler then keeps ~115
            // loop-invariant addresses alive and, with 256 registers per lane, spills them): re-derived per task from an opaque tid
            asm volatile("" : "+v"(tid));
            w = tid >> 6; l = tid & 63; lr = l & 15; lk = l >> 4;
        }
        __syncthreads();                                              // the previous task is done with LDS and task_s
        if (tid == 0) {
            int idx;
            if constexpr (BATCH) {
                int cur = task_s[6], gone = task_s[7];
                for (;;) {
                    if (gone >= nlists) { idx = ntasks; break; }
                    const int beg = list_off[cur], len = list_off[cur + 1] - beg;
                    idx = atomicAdd(ctl + 32 * cur, 1);
                    if (idx < len) { idx += beg; break; }
                    ++gone; cur = cur + 1 < nlists ? cur + 1 : 0;
                }
                task_s[6] = cur; task_s[7] = gone;
            } else {
                idx = atomicAdd(head, 1);
            }
            task_s[4] = idx;
            if (idx < ntasks) {
                const CholTask t = tasks[idx];
                task_s[0] = t.type & 255; task_s[1] = t.i; task_s[2] = t.j; task_s[3] = t.k; task_s[5] = (t.type >> 8) & 255; task_s[8] = t.type >> 16;
            }
        }
        __syncthreads();
        if (task_s[4] >= ntasks) return;
        const int type = task_s[0], ti = task_s[1], tj = task_s[2], tk = task_s[3];
#ifdef ALABI_CHOL_LOG
        const long long log_t0 = __builtin_amdgcn_s_memrealtime();
#endif
        const int tcnt = task_s[5] > 0 ? task_s[5] : 1;                 // UPDATE: block columns tk .. tk + tcnt - 1
        if constexpr (BATCH) {                                        // this task's matrix (wave-uniform: scalar loads)
            const CholMat cm = mats[__builtin_amdgcn_readfirstlane(task_s[8])];
            A = cm.A; ld = cm.ld; nb = cm.nb; ver = cm.ver; sver = cm.sver; info = cm.info; dinv = cm.dinv; linv = cm.linv;
            arsrc = __builtin_amdgcn_make_buffer_rsrc(A, 0, (unsigned)ld * (unsigned)ld * 8u, 0x00020000);
        }
#ifdef ALABI_CHOL_PROF
        const long long pw0 = __builtin_amdgcn_s_memrealtime();
#endif
        // ---- dependencies: up to eight (tile, version) pairs, polled by lanes 0..7 of wave 0
        if (w == 0) {
            int di_ = 0, dj_ = 0, need = 0;                           // lane 0 / 1 / 2
            if (type == 0) {                                          // CHAIN(k): tile (k,k-1) and (k,k) at k-1
                // (L[k-1,k-1] is NOT waited for here: its slabs are taken one by one below)
                if (l == 1) { di_ = tk; dj_ = tk - 1; need = tk - 1; }
                if (l == 2) { di_ = tk; dj_ = tk; need = tk - 1; }
                if (tk == 0) need = 0;
                if (tk == 0) { di_ = 0; dj_ = 0; }
            } else if (type == 1) {                                   // TRSM(i,k): tile (i,k) at k (L[k,k] is taken slab by slab)
                if (l == 1) { di_ = ti; dj_ = tk; need = tk; }
            } else {                                                  // UPDATE(i,j,k..kl): (i,kl), (j,kl) final (then so are the
                const int kl = tk + tcnt - 1;                         // panels before them), tile (i,j) at version k
                if (l == 0) { di_ = ti; dj_ = kl; need = kl + 1; }
                if (l == 1) { di_ = tj; dj_ = kl; need = kl + 1; }
                if (l == 2) { di_ = ti; dj_ = tj; need = tk; }
                if (type >= 4) {                                      // UPDATE2 / UPDATE4: the same for tile row i + 1
                    if (l == 3) { di_ = ti + 1; dj_ = kl; need = kl + 1; }
                    if (l == 4) { di_ = ti + 1; dj_ = tj; need = tk; }
                }
                if (type == 5) {                                      // UPDATE4: and for tile column j + 1
                    if (l == 5) { di_ = tj + 1; dj_ = kl; need = kl + 1; }
                    if (l == 6) { di_ = ti; dj_ = tj + 1; need = tk; }
                    if (l == 7) { di_ = ti + 1; dj_ = tj + 1; need = tk; }
                }
            }
            const bool active = l < 8 && need > 0;
            int spins = 0, ok = 1;
            while (true) {
                int have = need;
                if (active) have = __hip_atomic_load(ct_g32(ver + di_ * nb + dj_), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__all(have >= need)) break;
                if (++spins > spin_limit || ((spins & 63) == 0 && __hip_atomic_load(ct_g32(err), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                    ok = 0;
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            if (!ok && l == 0) { __hip_atomic_store(ct_g32(err), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); task_s[4] = ntasks; }
            // an UPDATE over a whole group of block columns streams its operand tiles with ordinary loads (they can hit in the XCD's
            // L2, where the neighbouring tasks of the same tile column have just put them; write-through-coherent loads always go
            // out to the fabric, and the bulk updates are bound by exactly that traffic): one acquire per task makes that valid
            if ((type == 2 && tcnt >= ALABI_CHOL_PLAIN_MIN) || type >= 4) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        __syncthreads();
#ifdef ALABI_CHOL_PROF
        if (tid == 0 && type == 0 && tk > 0) reinterpret_cast<long long*>(ctl + ((2 + nb * nb + nb + 1) & ~1))[7] += __builtin_amdgcn_s_memrealtime() - pw0;
#endif
        if (task_s[4] >= ntasks) return;                              // a wait ran out: every workgroup leaves at its next check
        if (type == 2) {
            // ---------------- UPDATE(i, j, k .. k + tcnt - 1): C(i,j) -= sum_k' A(i,k') A(j,k')^T, accumulated in registers over
            // the whole range (C is read and written ONCE per task); the operand tiles of column k' + 1 are in flight while the
            // matrix cores work on column k' (two LDS operand pairs).  Measured and not kept: operands two columns ahead (a
            // second register set; as part of this kernel it spills, as a function of its own the call costs every task more than
            // the deeper prefetch gains -- the grouped tasks were no faster, so the fetch latency is not what bounds them).
#ifdef ALABI_CHOL_PROF
            const long long u0 = __builtin_amdgcn_s_memrealtime();
            long long u1 = u0, u2 = u0;
#endif
            auto update_range = [&](auto plain_tag) {
                constexpr bool PL = decltype(plain_tag)::value;
                constexpr int NN = NT == 512 ? 2 : 4;                  // 16 x 16 tiles per wave: 16 rows x (64 or 32) columns
                const int wr = w & 3, c0w = NT == 512 ? 32 * (w >> 2) : 0;
                TileRegs16<NT> ra, rb;
                const unsigned row_i = (unsigned)(ti * 64) * (unsigned)ld * 8u, row_j = (unsigned)(tj * 64) * (unsigned)ld * 8u;
                tile_fetch16<PL, NT>(ra, arsrc, row_i + (unsigned)tk * 512u, ld, tid);
                tile_fetch16<PL, NT>(rb, arsrc, row_j + (unsigned)tk * 512u, ld, tid);
                double* C = A + (size_t)(ti * 64 + 16 * wr) * ld + tj * 64 + c0w;
                v4f64 acc[NN];
    #pragma unroll
                for (int n = 0; n < NN; ++n)
    #pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc[n][i] = __longlong_as_double((long long)__hip_atomic_load(
                            ct_g64(C + (size_t)(lk + 4 * i) * ld + 16 * n + lr), __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_AGENT));
                tile_put16<NT>(T0, ra, tid); tile_put16<NT>(T1, rb, tid);
                // Column k' + 1 waits in LDS and column k' + 2 is in flight while the matrix cores work on column k': the registers of
                // a fetch are written to the other operand pair at the START of the next iteration (its last readers passed the
                // barrier before) and refilled at once, so no wave waits for memory or for the LDS writes between two columns.
                // The C tile has landed before the loop starts: otherwise the compiler's wait for it sits INSIDE the loop (vmcnt is one
                // in-order counter) and drains the operand prefetch of every iteration.
                if (tcnt > 1) {
                    tile_fetch16<PL, NT>(ra, arsrc, row_i + (unsigned)(tk + 1) * 512u, ld, tid);
                    tile_fetch16<PL, NT>(rb, arsrc, row_j + (unsigned)(tk + 1) * 512u, ld, tid);
                }
    #pragma unroll
                for (int n = 0; n < NN; ++n) asm volatile("" : "+v"(acc[n]));   // C is waited for HERE (the fetch above stays in flight)
                __syncthreads();
#ifdef ALABI_CHOL_PROF
                u1 = __builtin_amdgcn_s_memrealtime();
#endif
                // One block column: MORE = column c + 1 exists (its pieces go registers -> the other LDS pair), MORE2 = column c + 2 exists
                // (memory -> the same registers).  Compile-time flags, so that a column is straight-line code and the compiler can count
                // vmcnt exactly: behind a branch it waits for vmcnt(0) in front of every piece, i.e. for the load issued one k-step pair ago.
                auto column = [&](auto more_tag, auto more2_tag, int c) {
                    constexpr bool MORE = decltype(more_tag)::value, MORE2 = decltype(more2_tag)::value;
                    const unsigned col2 = (unsigned)(tk + c + 2) * 512u;
                    double (*Pa)[66] = (c & 1) ? T0 : T2;                 // the other pair: block column c + 1 goes there
                    double (*Pb)[66] = (c & 1) ? T1 : T3;
                    double (*Ta)[66] = (c & 1) ? T2 : T0;
                    double (*Tb)[66] = (c & 1) ? T3 : T1;
                    // software pipeline over pairs of k-steps: the LDS reads of pair kp + 1 are issued before the matrix-core instructions
                    // of pair kp (two register sets; sched_barrier keeps the compiler from sinking the reads next to their uses --
                    // it otherwise reads, waits, multiplies, and every pair of k-steps exposes one LDS round trip)
                    double pa[2][2], pb[2][2][NN];
                    auto lds_pair = [&](int set, int kp) {
    #pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            // volatile: ONE ds_read_b64 per operand (conflict-free with the row stride of 66: 2 LDS cycles).  Left to
                            // itself the compiler pairs them into ds_read2_b64, which is banked modulo 32 and serviced in groups of 16
                            // lanes: rows r and r + 8 collide, 16 LDS cycles per instruction -- the LDS then co-limits the loop
                            pa[set][h] = lds_read_b64(&Ta[16 * wr + lr][4 * (2 * kp + h) + lk]);
    #pragma unroll
                            for (int n = 0; n < NN; ++n)
                                pb[set][h][n] = lds_read_b64(&Tb[c0w + 16 * n + lr][4 * (2 * kp + h) + lk]);
                        }
                    };
                    lds_pair(0, 0);
    #pragma unroll
                    for (int kp = 0; kp < 8; ++kp) {
                        if (kp < 7) lds_pair((kp + 1) & 1, kp + 1);
                        // one piece of block column c + 1 and of column c + 2 per k-step pair (NE pieces per operand tile, 2 NE / 8 per
                        // pair) instead of a burst of LDS writes and loads around the barrier, when no wave has matrix-core work
                        {
                            constexpr int NE = 2048 / NT, PER = 2 * NE / 8;
    #pragma unroll
                            for (int q = PER * kp; q < PER * (kp + 1); ++q) {
                                if (q < NE) {
                                    if (MORE) tile_put16_one<NT>(Pa, ra, q, tid);
                                    if (MORE2) tile_fetch16_one<PL, NT>(ra, q, arsrc, row_i + col2, ld, tid);
                                } else {
                                    if (MORE) tile_put16_one<NT>(Pb, rb, q - NE, tid);
                                    if (MORE2) tile_fetch16_one<PL, NT>(rb, q - NE, arsrc, row_j + col2, ld, tid);
                                }
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
                        for (int h = 0; h < 2; ++h)
    #pragma unroll
                            for (int n = 0; n < NN; ++n)
                                acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pa[kp & 1][h], pb[kp & 1][h][n], acc[n], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                };
                for (int c = 0; c < tcnt; ++c) {
                    const bool more = c + 1 < tcnt;
                    if (c + 2 < tcnt) column(std::true_type{}, std::true_type{}, c);
                    else if (more) column(std::true_type{}, std::false_type{}, c);
                    else column(std::false_type{}, std::false_type{}, c);
                    if (more) __syncthreads();                            // pair (c + 1) is complete, pair c may be overwritten
                }
    #pragma unroll
                for (int n = 0; n < NN; ++n)
    #pragma unroll
                    for (int i = 0; i < 4; ++i)
                        __hip_atomic_store(ct_g64(C + (size_t)(lk + 4 * i) * ld + 16 * n + lr),
                                           (unsigned long long)__double_as_longlong(acc[n][i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            };
            if (tcnt >= ALABI_CHOL_PLAIN_MIN) update_range(std::true_type{}); else update_range(std::false_type{});
#ifdef ALABI_CHOL_PROF
            u2 = __builtin_amdgcn_s_memrealtime();
#endif
            publish_version(ver + ti * nb + tj, tk + tcnt, tid);
#ifdef ALABI_CHOL_PROF
            if (tid == 0) {   // 10-ns units, grouped updates [8..13], single-column updates [16..21]: wait for deps, first fetch + C, loop, store + publish, count, columns
                unsigned long long* up = reinterpret_cast<unsigned long long*>(ctl + ((2 + nb * nb + nb + 1) & ~1)) + (tcnt >= ALABI_CHOL_PLAIN_MIN ? 8 : 16);
                const long long u3 = __builtin_amdgcn_s_memrealtime();
                atomicAdd(up + 0, (unsigned long long)(u0 - pw0)); atomicAdd(up + 1, (unsigned long long)(u1 - u0));
                atomicAdd(up + 2, (unsigned long long)(u2 - u1)); atomicAdd(up + 3, (unsigned long long)(u3 - u2));
                atomicAdd(up + 4, 1ull); atomicAdd(up + 5, (unsigned long long)tcnt);
            }
#endif
        } else if (type == 5) {
            // ---------------- UPDATE4(i, j, k .. k + tcnt - 1): tiles (i, j), (i + 1, j), (i, j + 1), (i + 1, j + 1) in one task -- a 128 x 128
            // output, wave w owning rows 32 (w & 3) .., columns 64 (w >> 2) .. (2 x 4 accumulator tiles: six operand reads feed eight
            // matrix-core instructions), four operand tiles per block column for four output tiles, the fixed cost of a task once per
            // four tiles.  Eight 64 x 34 half tiles (two buffers of four) fill the pool; otherwise as UPDATE2.  i >= j + 1, so that
            // tile (i, j + 1) is in the lower triangle ((j + 1, j + 1) is a diagonal tile: its update is the whole symmetric tile).
            if constexpr (NT == 512) {
                double (*H)[34] = reinterpret_cast<double (*)[34]>(ct_pool);
                const int wr2 = w & 3, wc = w >> 2;
                const int prow = tid >> 3, pcol = 2 * (tid & 7);
                const unsigned rowb[4] = {(unsigned)(ti * 64 + prow) * (unsigned)ld * 8u, (unsigned)((ti + 1) * 64 + prow) * (unsigned)ld * 8u,
                                          (unsigned)(tj * 64 + prow) * (unsigned)ld * 8u, (unsigned)((tj + 1) * 64 + prow) * (unsigned)ld * 8u};
                u32x4 pc[8];
                auto request = [&](int p, int hs) {
                    pc[p] = __builtin_amdgcn_raw_buffer_load_b128(arsrc, rowb[p >> 1] + (unsigned)(((tk + (hs >> 1)) * 64 + 32 * (hs & 1) + 16 * (p & 1) + pcol) * 8), 0, 0);
                };
                auto to_lds = [&](int p, int buf) {
                    *reinterpret_cast<u32x4*>(&H[(buf * 4 + (p >> 1)) * 64 + prow][16 * (p & 1) + pcol]) = pc[p];
                };
                const int nhs = 2 * tcnt;
#pragma unroll
                for (int p = 0; p < 8; ++p) request(p, 0);
                // C: rows 32 wr2 .. of the 128-row pair (tile i or i + 1), columns of tile j + wc
                double* C = A + (size_t)(ti * 64 + 32 * wr2) * ld + (tj + wc) * 64;
                v4f64 acc[2][4];
#pragma unroll
                for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                    for (int n = 0; n < 4; ++n)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            acc[ri][n][i] = __longlong_as_double((long long)__hip_atomic_load(
                                ct_g64(C + (size_t)(16 * ri + lk + 4 * i) * ld + 16 * n + lr), __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
                for (int p = 0; p < 8; ++p) to_lds(p, 0);
#pragma unroll
                for (int p = 0; p < 8; ++p) request(p, 1);
#pragma unroll
                for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                    for (int n = 0; n < 4; ++n) asm volatile("" : "+v"(acc[ri][n]));        // C is waited for HERE
                __syncthreads();
                auto half_stage = [&](auto more_tag, auto more2_tag, int hs) {
                    constexpr bool MORE = decltype(more_tag)::value, MORE2 = decltype(more2_tag)::value;
                    const int buf = hs & 1;
                    double (*Ha)[34] = H + (buf * 4 + (wr2 >> 1)) * 64 + 32 * (wr2 & 1);   // this wave's 32 rows of A(i) or A(i+1)
                    double (*Hb)[34] = H + (buf * 4 + 2 + wc) * 64;                         // its 64 columns = the rows of A(j) or A(j+1)
                    double pa[2][2][2], pb[2][2][4];
                    auto lds_pair = [&](int set, int kp) {
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int kk = 4 * (2 * kp + h) + lk;
                            pa[set][h][0] = lds_read_b64(&Ha[lr][kk]); pa[set][h][1] = lds_read_b64(&Ha[16 + lr][kk]);
#pragma unroll
                            for (int n = 0; n < 4; ++n) pb[set][h][n] = lds_read_b64(&Hb[16 * n + lr][kk]);
                        }
                    };
                    lds_pair(0, 0);
#pragma unroll
                    for (int kp = 0; kp < 4; ++kp) {
                        if (kp < 3) lds_pair((kp + 1) & 1, kp + 1);
#pragma unroll
                        for (int p = 2 * kp; p < 2 * kp + 2; ++p) {
                            if (MORE) to_lds(p, buf ^ 1);
                            if (MORE2) request(p, hs + 2);
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int h = 0; h < 2; ++h)
#pragma unroll
                            for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                                for (int n = 0; n < 4; ++n)
                                    acc[ri][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pa[kp & 1][h][ri], pb[kp & 1][h][n], acc[ri][n], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                };
                for (int hs = 0; hs < nhs; ++hs) {
                    const bool more = hs + 1 < nhs;
                    if (hs + 2 < nhs) half_stage(std::true_type{}, std::true_type{}, hs);
                    else if (more) half_stage(std::true_type{}, std::false_type{}, hs);
                    else half_stage(std::false_type{}, std::false_type{}, hs);
                    if (more) __syncthreads();
                }
#pragma unroll
                for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                    for (int n = 0; n < 4; ++n)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            __hip_atomic_store(ct_g64(C + (size_t)(16 * ri + lk + 4 * i) * ld + 16 * n + lr),
                                               (unsigned long long)__double_as_longlong(acc[ri][n][i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid < 4)
                __hip_atomic_store(ct_g32(ver + (ti + (tid & 1)) * nb + tj + (tid >> 1)), tk + tcnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (type == 4) {
            // ---------------- UPDATE2(i, j, k .. k + tcnt - 1): the grouped update of tiles (i, j) AND (i + 1, j) in one task (eight-wave
            // kernel only).  A 128 x 64 output: wave w owns rows 32 (w & 3) .., columns 32 (w >> 2) .. (2 x 2 accumulator tiles: two A
            // and two B operand reads feed four matrix-core instructions, 1.0 LDS read per instruction instead of 1.5), the operand
            // tile A(j, k') is fetched once for both rows, and the fixed cost of a task (queue draw, dependency poll, first fetch, C round
            // trip, publish: 4.3 us) is paid once per two tiles.  Three operand tiles per block column do not fit twice beside each other
            // in 135 KB, so a stage is HALF a block column (32 k-values): six 64 x 34 half tiles = two buffers in the pool; while the
            // k-steps of half-stage s run, half-stage s + 1 goes from registers to the other buffer and s + 2 from memory into the same
            // registers, piece by piece (six 16-byte pieces per thread: vmcnt(5) in front of each).  Every output element receives its
            // k-steps in the same order as in UPDATE: the same bits.
            if constexpr (NT == 512) {
                double (*H)[34] = reinterpret_cast<double (*)[34]>(ct_pool);                  // half tile q: rows 64 q .. 64 q + 63
                const int wr2 = w & 3, wc = w >> 2;
                const int prow = tid >> 3, pcol = 2 * (tid & 7);                             // this thread's piece of a half tile: 16 bytes
                const unsigned rowb[3] = {(unsigned)(ti * 64 + prow) * (unsigned)ld * 8u, (unsigned)((ti + 1) * 64 + prow) * (unsigned)ld * 8u,
                                          (unsigned)(tj * 64 + prow) * (unsigned)ld * 8u};
                u32x4 pc[6];
                auto request = [&](int p, int hs) {                                          // half-stage hs = 2 (block column) + half
                    pc[p] = __builtin_amdgcn_raw_buffer_load_b128(arsrc, rowb[p >> 1] + (unsigned)(((tk + (hs >> 1)) * 64 + 32 * (hs & 1) + 16 * (p & 1) + pcol) * 8), 0, 0);
                };
                auto to_lds = [&](int p, int buf) {
                    *reinterpret_cast<u32x4*>(&H[(buf * 3 + (p >> 1)) * 64 + prow][16 * (p & 1) + pcol]) = pc[p];
                };
                const int nhs = 2 * tcnt;
#pragma unroll
                for (int p = 0; p < 6; ++p) request(p, 0);
                double* C = A + (size_t)(ti * 64 + 32 * wr2) * ld + tj * 64 + 32 * wc;      // rows 32 wr2 .. of the 128-row pair
                v4f64 acc[2][2];
#pragma unroll
                for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                    for (int n = 0; n < 2; ++n)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            acc[ri][n][i] = __longlong_as_double((long long)__hip_atomic_load(
                                ct_g64(C + (size_t)(16 * ri + lk + 4 * i) * ld + 16 * n + lr), __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
                for (int p = 0; p < 6; ++p) to_lds(p, 0);
#pragma unroll
                for (int p = 0; p < 6; ++p) request(p, 1);                                    // (nhs >= 2 always)
#pragma unroll
                for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                    for (int n = 0; n < 2; ++n) asm volatile("" : "+v"(acc[ri][n]));        // C is waited for HERE
                __syncthreads();
                auto half_stage = [&](auto more_tag, auto more2_tag, int hs) {
                    constexpr bool MORE = decltype(more_tag)::value, MORE2 = decltype(more2_tag)::value;
                    const int buf = hs & 1;
                    double (*Ha)[34] = H + (buf * 3 + (wr2 >> 1)) * 64 + 32 * (wr2 & 1);   // this wave's 32 rows of A(i) or A(i+1)
                    double (*Hb)[34] = H + (buf * 3 + 2) * 64 + 32 * wc;                    // its 32 columns = rows of A(j)
                    double pa[2][2][2], pb[2][2][2];
                    auto lds_pair = [&](int set, int kp) {
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int kk = 4 * (2 * kp + h) + lk;
                            pa[set][h][0] = lds_read_b64(&Ha[lr][kk]); pa[set][h][1] = lds_read_b64(&Ha[16 + lr][kk]);
                            pb[set][h][0] = lds_read_b64(&Hb[lr][kk]); pb[set][h][1] = lds_read_b64(&Hb[16 + lr][kk]);
                        }
                    };
                    lds_pair(0, 0);
#pragma unroll
                    for (int kp = 0; kp < 4; ++kp) {
                        if (kp < 3) lds_pair((kp + 1) & 1, kp + 1);
#pragma unroll
                        for (int p = 2 * kp; p < 2 * kp + 2 && p < 6; ++p) {
                            if (MORE) to_lds(p, buf ^ 1);
                            if (MORE2) request(p, hs + 2);
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int h = 0; h < 2; ++h)
#pragma unroll
                            for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                                for (int n = 0; n < 2; ++n)
                                    acc[ri][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pa[kp & 1][h][ri], pb[kp & 1][h][n], acc[ri][n], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                };
                for (int hs = 0; hs < nhs; ++hs) {
                    const bool more = hs + 1 < nhs;
                    if (hs + 2 < nhs) half_stage(std::true_type{}, std::true_type{}, hs);
                    else if (more) half_stage(std::true_type{}, std::false_type{}, hs);
                    else half_stage(std::false_type{}, std::false_type{}, hs);
                    if (more) __syncthreads();
                }
#pragma unroll
                for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                    for (int n = 0; n < 2; ++n)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            __hip_atomic_store(ct_g64(C + (size_t)(16 * ri + lk + 4 * i) * ld + 16 * n + lr),
                                               (unsigned long long)__double_as_longlong(acc[ri][n][i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                __hip_atomic_store(ct_g32(ver + ti * nb + tj), tk + tcnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(ct_g32(ver + (ti + 1) * nb + tj), tk + tcnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else if (type == 1) {
            // ---------------- TRSM(i, k)
            {   // (16-byte coherent loads: half the instructions of the 8-byte form, and the faster rate per byte)
                TileRegs16<NT> rb;
                tile_fetch16<false, NT>(rb, arsrc, (unsigned)(ti * 64) * (unsigned)ld * 8u + (unsigned)tk * 512u, ld, tid);
                tile_put16<NT>(T1, rb, tid);
            }
            if (!ct_solve<NT, false, !BATCH>(ld, linv + (size_t)tk * 4096, sver + tk, err, spin_limit, ntasks,
                                     A + (size_t)(ti * 64) * ld + tk * 64)) return;
            publish_version(ver + ti * nb + tk, tk + 1, tid);
        } else {
            // ---------------- CHAIN(k)
            double* D = A + (size_t)(tk * 64) * ld + tk * 64;
#ifdef ALABI_CHOL_LOG
            if (tid == 0) { ct_log_kb = tk; g_chain_log[tk][0] = log_t0; g_chain_log[tk][1] = __builtin_amdgcn_s_memrealtime(); }
            __syncthreads();
#endif
#ifdef ALABI_CHOL_PROF
            long long* prof = reinterpret_cast<long long*>(ctl + ((2 + nb * nb + nb + 1) & ~1));
            const long long p0 = __builtin_amdgcn_s_memrealtime();
            long long p1 = p0, p2 = p0, p3 = p0, p4 = p0;
#endif
            if (tk > 0) {
                {
                    TileRegs16<NT> rb, rc;
                    tile_fetch16<false, NT>(rb, arsrc, (unsigned)(tk * 64) * (unsigned)ld * 8u + (unsigned)(tk - 1) * 512u, ld, tid);
                    tile_fetch16<false, NT>(rc, arsrc, (unsigned)(tk * 64) * (unsigned)ld * 8u + (unsigned)tk * 512u, ld, tid);
                    tile_put16<NT>(T1, rb, tid); tile_put16<NT>(T2, rc, tid);
                }
#ifdef ALABI_CHOL_PROF
                p1 = __builtin_amdgcn_s_memrealtime();
#endif
                CT_LOG(2);
                // the panel solve on the matrix cores, slab by slab as CHAIN(k-1) publishes the slabs of L[k-1,k-1] and the inverses of their
                // diagonal blocks (bounded wait each); tile (k,k) -= X X^T follows it one slab behind and ends up in T0 (ct_solve)
                if (!ct_solve<NT, true, !BATCH>(ld, linv + (size_t)(tk - 1) * 4096, sver + tk - 1, err,
                                        spin_limit, ntasks, A + (size_t)(tk * 64) * ld + (tk - 1) * 64)) return;
#ifdef ALABI_CHOL_PROF
                p2 = __builtin_amdgcn_s_memrealtime();
#endif
                CT_LOG(7);
                publish_version(ver + tk * nb + (tk - 1), tk, tid);      // the solved panel tile is final: updates of column k can start
                CT_LOG(8);
#ifdef ALABI_CHOL_PROF
                p3 = __builtin_amdgcn_s_memrealtime();
#endif
            } else {
                tile_load_sc1<NT>(T0, D, ld, tid);
            }
            __syncthreads();
#ifdef ALABI_CHOL_PROF
            p4 = __builtin_amdgcn_s_memrealtime();
#endif
            CT_LOG(9);
            const double rinv = ct_potrf_publish(tk, info, D, ld, dinv, sver + tk, linv + (size_t)tk * 4096, err);
#ifdef ALABI_CHOL_PROF
            const long long p5 = __builtin_amdgcn_s_memrealtime();
#endif
            if (w == 0) __hip_atomic_store(ct_g64(dinv + tk * 64 + l),
                                           (unsigned long long)__double_as_longlong(rinv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tile_store_sc1<NT>(D, ld, T0, tid, true);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                __hip_atomic_store(ct_g32(sver + tk), 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(ct_g32(ver + tk * nb + tk), tk + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            CT_LOG(15);
#ifdef ALABI_CHOL_PROF
            if (tid == 0 && tk > 0) {   // 10-ns units: [0] loads [1] trsm [2] store+publish panel [3] mfma+park [4] potrf [5] store+publish diag [6] count [7] wait for deps
                const long long p6 = __builtin_amdgcn_s_memrealtime();
                prof[0] += p1 - p0; prof[1] += p2 - p1; prof[2] += p3 - p2; prof[3] += p4 - p3; prof[4] += p5 - p4; prof[5] += p6 - p5; prof[6] += 1;
            }
#endif
        }
    }
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
chol_tasks_kernel(double* __restrict__ A, int ld, int nb, const CholTask* __restrict__ tasks, int ntasks, int* __restrict__ ctl,
                  int* __restrict__ info, double* __restrict__ dinv, int spin_limit) {
    chol_tasks_body<256, false>(A, ld, nb, tasks, ntasks, ctl, info, dinv, spin_limit, nullptr, nullptr, 1);
}
__global__ void __launch_bounds__(512)
chol_tasks8_kernel(double* __restrict__ A, int ld, int nb, const CholTask* __restrict__ tasks, int ntasks, int* __restrict__ ctl,
                   int* __restrict__ info, double* __restrict__ dinv, int spin_limit) {
    chol_tasks_body<512, false>(A, ld, nb, tasks, ntasks, ctl, info, dinv, spin_limit, nullptr, nullptr, 1);
}
__global__ void __launch_bounds__(512)
chol_tasks8_batch_kernel(const CholMat* __restrict__ mats, const CholTask* __restrict__ tasks, int ntasks, const int* __restrict__ list_off,
                         int nlists, int* __restrict__ ctl, int spin_limit) {
    chol_tasks_body<512, true>(nullptr, 64, 1, tasks, ntasks, ctl, nullptr, nullptr, spin_limit, mats, list_off, nlists);
}

}  // namespace alabi
