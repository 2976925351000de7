// On-GPU affine-invariant ensemble sampler (red-blue stretch move) for gfx950.
//
// Replaces emcee.EnsembleSampler(W, d, sm.lnprob).run_mcmc(p0, nsteps) as driven by the
// reference at alabi/core.py:2319-2325, with the log-probability of alabi/core.py:2073-2100:
// surrogate GP mean (core.py:1486 / :85) + uniform box prior (utility.py:218-275).
// Semantics restated from emcee 3 moves/red_blue.py + moves/stretch.py (see
// oracle/stretch_oracle.py, which is the CPU statement these kernels are tested against):
//   per step: random balanced 0/1 labelling; for split in {0,1}: for every walker k of the
//   active set S: z = ((a-1)u+1)^2/a, partner r = randint(|C|), q = C[r] - (C[r]-S_k) z,
//   accept iff (d-1) ln z + lnp(q) - lnp(S_k) > ln u'.
//
// Moves (emcee's moves=, alabi_ens_set_moves): one move per step and ensemble out of a table of stretch and differential-
// evolution moves (emcee 3 moves/de.py: q = S_k + gamma (C[j2] - C[j1]), j1 != j2, gamma = gamma0 (1 + sigma n), log factor 0).
// A DE record uses the stretch record's slots plus one second-partner id (write_de_record); the half-step, multi-proposal and
// propose kernels have a second instantiation that reads it (tests/de_move_numpy.py is the CPU statement).
// The snooker update (ter Braak & Vrugt 2008, eq. 4; tests/snooker_numpy.py is the CPU statement) moves S_k along the line through
// itself and z = C[j1] by gammas times the difference of the projections of z1 = C[j2] and z2 = C[j3] on that line (snooker_coord);
// its log factor (d - 1) (ln|q - z| - ln|S_k - z|) depends on the rows, so it is formed where the proposal is: the half-step and
// the propose kernel have a third instantiation that reads the third partner (write_snooker_record) and still takes stretch and
// DE records, since the step's move is chosen on the device.  The multi-proposal kernel has no such instantiation: a set with a
// snooker move runs one proposal per workgroup.
//
// The walk move (Goodman & Weare 2010; emcee 3 moves/walk.py) and the KDE move (emcee 3 moves/kde.py) use the WHOLE complementary
// half (tests/walk_kde_numpy.py is the CPU statement): walk q = S_k + sum_{j in J} z_j (C[j] - mean_J) / sqrt(s0 - 1) over a subset J
// of s0 rows (all of them by default), log factor 0; KDE q = C[r] + L z with L the Cholesky factor of f^2 cov(C), log factor
// kde.logpdf(S_k) - kde.logpdf(q) as two log-sum-exps over the whitened rows.  Their records name no partner: the half-step and the
// propose kernel have a fourth instantiation (wk_proposal) that takes the step's kind from MoveBuffers::kind, draws the subset, r
// and the normals where they are used (Philox streams 6-8) and still takes stretch, DE and snooker records.  ens_kde_prepass_kernel,
// one workgroup per ensemble in front of a half step, leaves mean, L and the whitened rows of the half in KdeBuffers, or the flag
// of a factorisation that broke down (every proposal of that half step is then rejected and the half step counted).
//
// E independent ensembles of W walkers ("independent chains") can share every launch: walker
// ids are global (e*W + i), lists are per-ensemble segments, blockIdx.y is the ensemble.
//
// Kernels
//   ens_draw_kernel   one workgroup per (step, ensemble): Philox4x32-10 keys -> rank -> label ->
//                     the two ordered walker lists, then per list position one proposal record
//                     (walker id, partner walker id, z, (d-1) ln z, ln u').  Draws depend only on
//                     (seed, step, global walker id): every rank of a multi-GPU run and the CPU
//                     oracle generate identical values.
//   ens_prep_kernel   the same record construction from caller-supplied draws (test entry).
//   ens_half_kernel   one workgroup per proposal of a half step.  The record is ONE dependent
//                     load away from blockIdx (no list -> partner -> list chasing); the first d
//                     lanes build the proposal and the box test; all lanes evaluate the GP mean
//                     with coalesced SoA loads of the training set and a shuffle+LDS reduction;
//                     lane 0 does the accept test; the walker's state (and its chain row) is
//                     written in place.  Walkers of S write, walkers of C are only read, so a
//                     half step needs no intra-kernel synchronisation; the two half steps are
//                     ordered by the stream (a kernel boundary is cheaper than a grid barrier
//                     on this chip).
// The persistent kernels, which run whole chunks of steps in one launch, are in ens_stream.hip (shared code: ens_stream.hpp),
// ens_pair.hip and ens_group.hip; this file keeps the draws, the records and one launch per half step.
// The per-step work at the headline size (W=256, N=2000, d=10) is 2 x 128 workgroups x
// 2000 kernel evaluations: latency bound, not HBM bound (X and alpha, 176 KB, stay in L2).
#include <cstdlib>
#include <vector>
#include "ens_device.hpp"

namespace alabi {

// One proposal record, in the arrays the launch-per-half-step kernels read and in one 32-byte line for the persistent kernel.
__device__ inline void store_record(const DrawBuffers& b, size_t pos, int wid, int cw, double zz, double lnfac, double lnu) {
    b.order[pos] = wid;
    b.cw[pos] = cw;
    b.zz[pos] = zz;
    b.lnfac[pos] = lnfac;
    b.lnu[pos] = lnu;
    unsigned long long* pk = b.packed + 4 * pos;
    pk[0] = (unsigned long long)(unsigned)wid | ((unsigned long long)(unsigned)cw << 32);
    pk[1] = (unsigned long long)__double_as_longlong(zz);
    pk[2] = (unsigned long long)__double_as_longlong(lnfac);
    pk[3] = (unsigned long long)__double_as_longlong(lnu);
}

// Proposal record of list position `pos` (walker id wid = order[pos]) from raw draws keyed by
// walker id.  z = ((a-1) u + 1)^2 / a in NumPy's operation order (no contraction).
__device__ inline void write_record(const DrawBuffers& b, size_t pos, int wid, int cw, double u_z, double u_acc,
                                    double a, int d) {
    const double t1 = (a - 1.0) * u_z + 1.0;
    const double zz = (t1 * t1) / a;
    store_record(b, pos, wid, cw, zz, ((double)d - 1.0) * log(zz), log(u_acc));
}

// Differential-evolution record (emcee 3 moves/de.py: q = s + gamma (C[j2] - C[j1]), log factor 0) in the slots of a stretch
// record: cw = C[j1], zz = gamma, lnfac = 0.0 -- the accept test lnfac + lp_new - lp_old > ln u' needs no second form -- and the
// second partner beside it.  A stretch record is marked by cw2 = -1.
__device__ inline void write_de_record(const DrawBuffers& b, const MoveBuffers& mv, size_t pos, int wid, int cw, int cw2, int j2,
                                       double gamma, double u_acc) {
    store_record(b, pos, wid, cw, gamma, 0.0, log(u_acc));
    if (mv.cw2) { mv.cw2[pos] = cw2; mv.partner2[pos] = j2; }
}

// Snooker record: cw = z = C[j1], cw2 = z1 = C[j2], third partner z2 = C[j3], zz = gammas; lnfac is a placeholder, the kernel
// that forms the proposal computes the factor from the rows.  Stretch and DE records carry -1 in the third-partner slots.
__device__ inline void write_snooker_record(const DrawBuffers& b, const MoveBuffers& mv, size_t pos, int wid, int cw, int cw2, int j2,
                                            int cw3, int j3, double gammas, double u_acc) {
    store_record(b, pos, wid, cw, gammas, 0.0, log(u_acc));
    if (mv.cw2) { mv.cw2[pos] = cw2; mv.partner2[pos] = j2; }
    if (mv.cw3) { mv.cw3[pos] = cw3; mv.partner3[pos] = j3; }
}

// grid = (steps of the chunk, ensembles); dynamic LDS = Wp * 12 + 1024 bytes, Wp = W rounded up to a power of two.
// The rank of a walker's key among the step's keys (ties by walker id) decides its label: a bitonic sort of (key, id) pairs in
// LDS -- O(W log^2 W) compare-exchanges instead of the W^2 comparisons of the first version (0.21 ms per 1024-step chunk at
// 1024 walkers, 0.62 ms at 2048: 4 % of the C4 run) -- then the two ordered lists by a prefix count over the labels.
__global__ void __launch_bounds__(256)
ens_draw_kernel(unsigned long long seed, const long long* __restrict__ run_state, long long step_off, int W, int Wp, int d, MoveTable mt,
                DrawBuffers b, MoveBuffers mv) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);                       // [Wp]; after the sort: label[W], olist[W]
    uint32_t* ids = reinterpret_cast<uint32_t*>(smem + (size_t)Wp * 8);       // [Wp]
    int* scan = reinterpret_cast<int*>(smem + (size_t)Wp * 12);               // [256]
    const int E = gridDim.y, e = blockIdx.y, tid = threadIdx.x;
    // first step of the chunk: read from run_state, or (run_state == nullptr) given by value so that the launch depends on no earlier kernel
    const long long step = (run_state ? run_state[0] : 0) + step_off + blockIdx.x;
    const uint32_t s_lo = (uint32_t)step, s_hi = (uint32_t)((unsigned long long)step >> 32);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const size_t base = ((size_t)blockIdx.x * E + e) * W;
    const uint32_t g0 = (uint32_t)e * (uint32_t)W;  // global id of this ensemble's walker 0
    uint32_t r[4];
    for (int i = tid; i < Wp; i += 256) {
        uint64_t key = ~0ull;                                                 // padding sorts behind every walker (ties by id)
        if (i < W) {
            philox4x32_10(s_lo, s_hi, g0 + (uint32_t)i, 0u, k0, k1, r);
            key = ((uint64_t)r[0] << 32) | r[1];
        }
        keys[i] = key; ids[i] = (uint32_t)i;
    }
    __syncthreads();
    for (int k = 2; k <= Wp; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < Wp; t += 256) {
                const int x = t ^ j;
                if (x > t) {
                    const uint64_t ka = keys[t], kb = keys[x];
                    const uint32_t ia = ids[t], ib = ids[x];
                    const bool gt = (ka > kb) || (ka == kb && ia > ib);
                    if (gt == ((t & k) == 0)) { keys[t] = kb; keys[x] = ka; ids[t] = ib; ids[x] = ia; }
                }
            }
            __syncthreads();
        }
    // rank of walker ids[t] is t: label = rank & 1 (`label` and `olist` reuse the keys' memory: the sort's last barrier is behind us)
    int* label = reinterpret_cast<int*>(smem);
    int* olist = label + W;   // local ids in list order (set 0 then set 1)
    for (int t = tid; t < Wp; t += 256) {
        const uint32_t i = ids[t];
        if (i < (uint32_t)W) label[i] = t & 1;
    }
    __syncthreads();
    // position of walker i inside its list = number of walkers j < i with the same label: every thread owns a run of
    // consecutive walkers, the runs' label-0 counts are scanned by one wave
    const int n0 = (W + 1) / 2;
    const int per = (W + 255) / 256, i0 = tid * per, i1 = (i0 + per < W) ? i0 + per : W;
    int zeros = 0;
    for (int i = i0; i < i1; ++i) zeros += (label[i] == 0);
    scan[tid] = zeros;
    __syncthreads();
    if (tid < 64) {
        int v[4], tot = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { v[q] = scan[4 * tid + q]; tot += v[q]; }
        int inc = tot;                                                        // inclusive scan over the 64 lanes
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(inc, off, 64); if (tid >= off) inc += o; }
        int run = inc - tot;
#pragma unroll
        for (int q = 0; q < 4; ++q) { scan[4 * tid + q] = run; run += v[q]; }
    }
    __syncthreads();
    {
        int z = scan[tid], o = i0 - z;                                        // label-0 / label-1 walkers before i0
        for (int i = i0; i < i1; ++i) {
            const int li = label[i];
            const int pos = li ? o++ : z++;
            olist[(li ? n0 : 0) + pos] = i;
        }
    }
    __syncthreads();
    // The step's move, one per step and ensemble as in emcee: stream 3 at the ensemble's walker 0, index = #{k: cum[k] <= u}
    // (what np.searchsorted(cum, u, side="right") returns), clipped.  The table is read with constant indices only: it lives in
    // the kernel arguments, and a variable index would copy it to scratch memory.
    int mi = 0;
    if (mt.n > 1) {
        philox4x32_10(s_lo, s_hi, g0, 3u, k0, k1, r);
        const double um = u53(r[0], r[1]);
#pragma unroll
        for (int k = 0; k < ALABI_MAX_MOVES; ++k) mi += (k < mt.n && mt.cum[k] <= um) ? 1 : 0;
        if (mi > mt.n - 1) mi = mt.n - 1;
    }
    int kind = mt.kind[0];
    double mp0 = mt.p0[0], mp1 = mt.p1[0];
#pragma unroll
    for (int k = 1; k < ALABI_MAX_MOVES; ++k)
        if (k == mi) { kind = mt.kind[k]; mp0 = mt.p0[k]; mp1 = mt.p1[k]; }
    if (tid == 0 && mv.move) mv.move[(size_t)blockIdx.x * E + e] = mi;
    if (tid == 0 && mv.kind) {
        mv.kind[(size_t)blockIdx.x * E + e] = kind;
        mv.par[2 * ((size_t)blockIdx.x * E + e)] = mp0;
        mv.par[2 * ((size_t)blockIdx.x * E + e) + 1] = mp1;
    }
    for (int pos = tid; pos < W; pos += 256) {
        const int i = olist[pos];
        const int li = pos >= n0;
        philox4x32_10(s_lo, s_hi, g0 + (uint32_t)i, 1u, k0, k1, r);
        const double uz = u53(r[0], r[1]);
        const uint64_t nc = li ? (uint64_t)n0 : (uint64_t)(W - n0);
        const int pr = (int)(((uint64_t)r[2] * nc) >> 32);
        const int cw = nc ? olist[(li ? 0 : n0) + pr] : i;   // one walker (a Metropolis set): no complementary half, the record names itself
        const uint32_t r3 = r[3];
        philox4x32_10(s_lo, s_hi, g0 + (uint32_t)i, 2u, k0, k1, r);
        const double ua = u53(r[0], r[1]);
        // streams 0-2 and what is exported of them do not depend on the move
        b.partner[base + pos] = pr;
        b.u_z[base + pos] = uz;
        b.u_acc[base + pos] = ua;
        b.pos_of[base + i] = pos;
        if (kind >= 3) {
            // walk, KDE: the proposal reads the whole complementary half and draws where it is formed (streams 6-8); the record
            // carries the walker and ln u' (the stretch partner fills its slot, nobody reads it)
            store_record(b, base + pos, (int)g0 + i, (int)g0 + cw, 0.0, 0.0, log(ua));
            if (mv.cw2) { mv.cw2[base + pos] = -1; mv.partner2[base + pos] = -1; }
            if (mv.cw3) { mv.cw3[base + pos] = -1; mv.partner3[base + pos] = -1; }
            continue;
        }
        if (kind == 0) {
            write_record(b, base + pos, (int)g0 + i, (int)g0 + cw, uz, ua, mp0, d);
            if (mv.cw2) { mv.cw2[base + pos] = -1; mv.partner2[base + pos] = -1; }
            if (mv.cw3) { mv.cw3[base + pos] = -1; mv.partner3[base + pos] = -1; }
        } else {
            // j1 = pr and j2 != j1 from the fourth word: uniform over the nc (nc - 1) ordered pairs (emcee's _get_nondiagonal_pairs);
            // nc >= 2 is checked where the moves are set
            const int j2p = (int)(((uint64_t)r3 * (nc - 1)) >> 32);
            const int j2 = j2p + (j2p >= pr ? 1 : 0);
            const int cw2 = olist[(li ? 0 : n0) + j2];
            if (kind == 2) {
                // snooker: a third walker from stream 5, bumped past the smaller and then the larger of j1, j2 -- uniform over the
                // nc (nc - 1) (nc - 2) ordered triples; nc >= 3 is checked where the moves are set
                philox4x32_10(s_lo, s_hi, g0 + (uint32_t)i, 5u, k0, k1, r);
                const int jlo = pr < j2 ? pr : j2, jhi = pr < j2 ? j2 : pr;
                int j3 = (int)(((uint64_t)r[0] * (nc - 2)) >> 32);
                j3 += (j3 >= jlo ? 1 : 0);
                j3 += (j3 >= jhi ? 1 : 0);
                const int cw3 = olist[(li ? 0 : n0) + j3];
                write_snooker_record(b, mv, base + pos, (int)g0 + i, (int)g0 + cw, (int)g0 + cw2, j2, (int)g0 + cw3, j3, mp0, ua);
                continue;
            }
            // gamma = g0 (1 + sigma n), n standard normal by Box-Muller from stream 4
            philox4x32_10(s_lo, s_hi, g0 + (uint32_t)i, 4u, k0, k1, r);
            const double u1 = u53(r[0], r[1]), u2 = u53(r[2], r[3]);
            const double nrm = sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2);
            const double gamma = mp0 * (1.0 + mp1 * nrm);
            write_de_record(b, mv, base + pos, (int)g0 + i, (int)g0 + cw, (int)g0 + cw2, j2, gamma, ua);
            if (mv.cw3) { mv.cw3[base + pos] = -1; mv.partner3[base + pos] = -1; }
        }
    }
}

// Records from caller-supplied draws (E = 1): order[W] lists set 0 then set 1, u_z / partner / u_acc are
// keyed by WALKER id, partner indexes the complementary list.  Bad indices yield an inert record (w = -1).
__global__ void __launch_bounds__(256)
ens_prep_kernel(const int* __restrict__ order, int n0, int W, const double* __restrict__ u_z,
                const int* __restrict__ partner, const double* __restrict__ u_acc, double a, int d,
                DrawBuffers b) {
    const int pos = blockIdx.x * 256 + threadIdx.x;
    if (pos >= W) return;
    const int w = order[pos];
    const int li = pos >= n0;
    const int nC = li ? n0 : W - n0;
    int cw = -1;
    double uz = 0.5, ua = 0.5;
    int wid = -1;
    if ((unsigned)w < (unsigned)W) {
        const int pr = partner[w];
        if ((unsigned)pr < (unsigned)nC) {
            const int c = order[(li ? 0 : n0) + pr];
            if ((unsigned)c < (unsigned)W) { wid = w; cw = c; uz = u_z[w]; ua = u_acc[w]; }
        }
    }
    write_record(b, pos, wid, cw, uz, ua, a, d);
}

// The same for differential-evolution records: j1 / j2 index the complementary list (j1 != j2), gamma is the step size.
__global__ void __launch_bounds__(256)
ens_prep_de_kernel(const int* __restrict__ order, int n0, int W, const int* __restrict__ j1, const int* __restrict__ j2,
                   const double* __restrict__ gamma, const double* __restrict__ u_acc, DrawBuffers b, MoveBuffers mv) {
    const int pos = blockIdx.x * 256 + threadIdx.x;
    if (pos >= W) return;
    const int w = order[pos];
    const int li = pos >= n0;
    const int nC = li ? n0 : W - n0;
    int wid = -1, cw = -1, cw2 = -1, jj = -1;
    double g = 0.0, ua = 0.5;
    if ((unsigned)w < (unsigned)W) {
        const int a1 = j1[w], a2 = j2[w];
        if ((unsigned)a1 < (unsigned)nC && (unsigned)a2 < (unsigned)nC && a1 != a2) {
            const int c1 = order[(li ? 0 : n0) + a1], c2 = order[(li ? 0 : n0) + a2];
            if ((unsigned)c1 < (unsigned)W && (unsigned)c2 < (unsigned)W) { wid = w; cw = c1; cw2 = c2; jj = a2; g = gamma[w]; ua = u_acc[w]; }
        }
    }
    write_de_record(b, mv, pos, wid, cw, cw2, jj, g, ua);
}

// The same for snooker records: j1 / j2 / j3 index the complementary list, pairwise distinct; gamma is the fixed step gammas.
__global__ void __launch_bounds__(256)
ens_prep_snooker_kernel(const int* __restrict__ order, int n0, int W, const int* __restrict__ j1, const int* __restrict__ j2,
                        const int* __restrict__ j3, double gamma, const double* __restrict__ u_acc, DrawBuffers b, MoveBuffers mv) {
    const int pos = blockIdx.x * 256 + threadIdx.x;
    if (pos >= W) return;
    const int w = order[pos];
    const int li = pos >= n0;
    const int nC = li ? n0 : W - n0;
    int wid = -1, cw = -1, cw2 = -1, cw3 = -1, jj2 = -1, jj3 = -1;
    double ua = 0.5;
    if ((unsigned)w < (unsigned)W) {
        const int a1 = j1[w], a2 = j2[w], a3 = j3[w];
        if ((unsigned)a1 < (unsigned)nC && (unsigned)a2 < (unsigned)nC && (unsigned)a3 < (unsigned)nC && a1 != a2 && a1 != a3 && a2 != a3) {
            const int off = li ? 0 : n0;
            const int c1 = order[off + a1], c2 = order[off + a2], c3 = order[off + a3];
            if ((unsigned)c1 < (unsigned)W && (unsigned)c2 < (unsigned)W && (unsigned)c3 < (unsigned)W) {
                wid = w; cw = c1; cw2 = c2; cw3 = c3; jj2 = a2; jj3 = a3; ua = u_acc[w];
            }
        }
    }
    write_snooker_record(b, mv, pos, wid, cw, cw2, jj2, cw3, jj3, gamma, ua);
}

// Records of the walk and KDE test entries: the walker and ln u' (bad walker ids yield an inert record, w = -1).
__global__ void __launch_bounds__(256)
ens_prep_wk_kernel(const int* __restrict__ order, int W, const double* __restrict__ u_acc, DrawBuffers b, MoveBuffers mv) {
    const int pos = blockIdx.x * 256 + threadIdx.x;
    if (pos >= W) return;
    const int w = order[pos];
    const bool good = (unsigned)w < (unsigned)W;
    store_record(b, pos, good ? w : -1, -1, 0.0, 0.0, log(good ? u_acc[w] : 0.5));
    mv.cw2[pos] = -1; mv.partner2[pos] = -1;
    mv.cw3[pos] = -1; mv.partner3[pos] = -1;
}

// kind and parameters of step 0's move (E = 1), for the test entries
__global__ void ens_set_step_move_kernel(MoveBuffers mv, int kind, double p0, double p1) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { mv.kind[0] = kind; mv.par[0] = p0; mv.par[1] = p1; }
}

// h and the centred inputs of the squared-exponential half-step kernels (alabi_gp::Xc, ::ens_h)
__global__ void __launch_bounds__(256)
ens_se_prepare_kernel(const double* __restrict__ Xt, const double* __restrict__ centre, const double* __restrict__ alpha, int N, int Npad,
                      int d, int rows, double* __restrict__ Xc, double* __restrict__ h) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= Npad) return;
    // a point that contributes nothing (padding, alpha exactly 0 or NaN) gets h = ALABI_SE_PAD AND a zero row: with its real
    // coordinates the exponent q.x - |q|^2/2 - 1000 of se_pair_terms could still be large for a point tens of length scales from
    // the centre (round-3 advisor), with a zero row it is -|q|^2/2 - 1000 and the term underflows to exactly 0
    const double a = n < N ? alpha[n] : 0.0;
    const bool live = a != 0.0 && a == a;
    double hh = 0.0;
    for (int k = 0; k < rows; ++k) {
        const double v = (k < d && live) ? Xt[(size_t)k * Npad + n] - centre[k] : 0.0;
        Xc[(size_t)k * Npad + n] = v;
        hh = fma(v, v, hh);
    }
    double out = ALABI_SE_PAD;
    if (live) {
        long long bits = __double_as_longlong(0.5 * hh - log(fabs(a)));
        bits = (bits & ~1LL) | (a < 0.0 ? 1LL : 0LL);
        out = __longlong_as_double(bits);
    }
    h[n] = out;
}

// The Gaussian move's draws of drawn step 0 (alabi_ens_export_gauss_draws): f per ensemble, the coordinate and the d normals per
// walker, from the kind and parameters the draw kernel left for the step (f = 1, coordinate -1 where its move is another).
__global__ void __launch_bounds__(256)
ens_gauss_export_kernel(unsigned long long seed, const long long* __restrict__ run_state, int W, int E, int d, MoveBuffers mv,
                        double* __restrict__ f_out, int* __restrict__ coord_out, double* __restrict__ z_out) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= W * E) return;
    const int e = gid / W;
    const long long step = run_state[0];
    const uint32_t s_lo = (uint32_t)step, s_hi = (uint32_t)((unsigned long long)step >> 32);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    double f = 1.0;
    int c = -1;
    if (mv.kind[e] == 5) gauss_step_draws(s_lo, s_hi, (uint32_t)(e * W), (uint32_t)gid, k0, k1, step, mv.par[2 * e], (int)mv.par[2 * e + 1], d, f, c);
    if (gid == e * W) f_out[e] = f;
    coord_out[gid] = c;
    for (int k = 0; k < d; ++k) z_out[(size_t)gid * d + k] = philox_normal(s_lo, s_hi, (uint32_t)gid, 10u + 16u * (uint32_t)k, k0, k1);
}

// The proposal of a record from the rows it names, in NumPy's operation order (the library is built without contraction):
// stretch q = c - (c - s) z; differential evolution q = s + gamma (c2 - c), c = C[j1], c2 = C[j2] (diff = np.diff(c[pairs])).
__device__ inline double propose_coord(bool de, double sv, double cv, double c2v, double zz) {
    return de ? sv + zz * (c2v - cv) : cv - (cv - sv) * zz;
}

// Sum over k = 0 .. d-1 of the value lane k of the wave holds, accumulated in that order from 0 (what tests/snooker_numpy.py
// states as _seq_sum); every lane returns it.  readlane takes the value whether or not the caller's branch has the lane active.
template <int D>
__device__ __forceinline__ double lane_seq_sum(double v, int d) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double t = lane_bcast(v, k);
        if (k < d) s += t;
    }
    return s;
}

// Snooker proposal (ter Braak & Vrugt 2008, eq. 4), coordinate `lane` of it.  Called by lanes 0 .. D-1 of wave 0 together; lanes
// >= d pass zeros and their result means nothing.  sv, zv, z1v, z2v: the coordinate of s, z = C[j1], z1 = C[j2], z2 = C[j3].
//   delta = s - z, n = |delta|, e = delta / n, p = e.z1 - e.z2, q = s + (gamma p) e, lnfac = (d - 1) (ln|q - z| - ln n)
// in the operation order of tests/snooker_numpy.py (products rounded, then added in coordinate order: no contraction); sqrt and /
// are correctly rounded, so q has the model's bits.  n == 0 makes q NaN (out of the box), |q - z| == 0 makes lnfac -inf or, for
// d == 1, NaN: the accept test is false in each case.
template <int D>
__device__ __forceinline__ double snooker_coord(int d, double sv, double zv, double z1v, double z2v, double gamma, double& lnfac) {
    const double delta = sv - zv;
    const double n = sqrt(lane_seq_sum<D>(delta * delta, d));
    const double ev = delta / n;
    const double pz1 = lane_seq_sum<D>(ev * z1v, d);
    const double pz2 = lane_seq_sum<D>(ev * z2v, d);
    const double gp = gamma * (pz1 - pz2);
    const double qv = sv + gp * ev;
    const double dq = qv - zv;
    const double nq = sqrt(lane_seq_sum<D>(dq * dq, d));
    lnfac = ((double)d - 1.0) * (log(nq) - log(n));
    return qv;
}

// ---- walk and KDE moves: proposals from the whole complementary half ----------------------------------------------------------
// Draws (tests/walk_kde_numpy.py states the same layout): Philox counter (step, global walker id, stream word), stream word =
// S + 16 b with
//   S = 6, b = j >> 1:  64-bit key of row j of the complementary list, words (0, 1) for even j, (2, 3) for odd j; row j belongs to the
//                       subset J iff the rank of its key among the Nc keys (ties by j) is < s0 -- no key is drawn when s0 = Nc;
//   S = 7, b = j:       z_j, the normal of row j (Box-Muller as stream 4: sqrt(-2 ln(1 - u53(r0, r1))) cos(2 pi u53(r2, r3)));
//   S = 8, b = 0:       r = (r0 Nc) >> 32, the KDE move's row;  b = 1 + k: the normal z_k of coordinate k.
// Streams 0-5 are S + 16 b with b = 0 and S < 6: nothing here meets them.  S = 9 and 10 belong to the Gaussian move (ens_device.hpp).
#define ALABI_WK_MAX_NC 2048     // rows of a complementary half the walk move's lists hold in LDS
#define ALABI_WK_TILE 2048       // doubles of the tile through which its rows are read

// log(exp(m1) s1 + exp(m2) s2) as (max, scaled sum): the running-maximum form of kde.hip
__device__ inline void lse_merge(double& m, double& s, double m2, double s2) {
    const double mm = m > m2 ? m : m2;
    if (mm == -INFINITY) { m = mm; s = 0.0; return; }
    s = s * exp(m - mm) + s2 * exp(m2 - mm);
    m = mm;
}

// The proposal of a walk (kind 3) or KDE (kind 4) step for walker w (global id), called by EVERY thread of the workgroup (it has
// barriers).  sv: coordinate tid of the walker in lanes tid < d, 0 elsewhere.  Leaves coordinate tid of the proposal in qc (lanes
// tid < d), the log factor in lnfac (every thread) and reject = 1 where the half step's factorisation broke down.  Returns 0 for
// a proposal that is a no-op (a test entry's subset or row out of range or repeated).  Operation order: tests/walk_kde_numpy.py.
template <int D>
__device__ __forceinline__ int wk_proposal(const HalfArgs& p, int kind, int e, int w, double sv, double& qc, double& lnfac, int& reject) {
    __shared__ __attribute__((aligned(16))) unsigned char wk_lds[48 * 1024];
    __shared__ double wk_red[2][16][2];
    const int tid = threadIdx.x, T = blockDim.x, d = p.d;
    const int Nc = p.split ? p.n0 : p.W - p.n0;
    const int* clist = p.rec.order + (size_t)e * p.W + (p.split ? 0 : p.n0);
    const long long step = p.run_state[0] + p.local_t;
    const uint32_t s_lo = (uint32_t)step, s_hi = (uint32_t)((unsigned long long)step >> 32);
    const uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32);
    const bool in = tid < d;
    qc = 0.0; lnfac = 0.0; reject = 0;
    if (kind == 5) {
        // Gaussian Metropolis move (ens_device.hpp: gauss_step_draws, gauss_coord): reads nothing but the walker itself
        double* Cs = reinterpret_cast<double*>(wk_lds);                        // [d, d] (32 KB at d = 64)
        const int mi = p.gauss_k >= 0 ? p.gauss_k : p.mvidx[e];
        if (!p.gauss_C || (unsigned)mi >= (unsigned)ALABI_MAX_MOVES) return 0;  // checked where the moves are set
        const int diagonal = (p.gauss_diag >> mi) & 1;
        double f;
        int c;
        if (p.inj.z) { f = p.gauss_f; c = p.inj.idx[w]; }
        else gauss_step_draws(s_lo, s_hi, (uint32_t)(e * p.W), (uint32_t)w, k0, k1, step, p.mvpar[2 * e], (int)p.mvpar[2 * e + 1], d, f, c);
        if (c < -1 || c >= d) return 0;                                        // a test entry's coordinate out of range; workgroup-uniform
        for (int idx = tid; idx < d * d; idx += T) Cs[idx] = p.gauss_C[(size_t)mi * d * d + idx];
        __syncthreads();
        if (tid < 64) {
            double z = 0.0;
            if (in) z = p.inj.z ? p.inj.z[(size_t)w * d + tid] : philox_normal(s_lo, s_hi, (uint32_t)w, 10u + 16u * (uint32_t)tid, k0, k1);
            qc = gauss_coord(Cs, diagonal, d, tid, sv, z, f, c);
        }
        return 1;
    }
    if (kind == 3) {
        uint64_t* keys = reinterpret_cast<uint64_t*>(wk_lds);                  // [Nc]; after the ranks: zl
        double* zl = reinterpret_cast<double*>(wk_lds);                        // [s0] normals in sum order
        int* rank = reinterpret_cast<int*>(wk_lds + 16 * 1024);                // [Nc]
        int* J = reinterpret_cast<int*>(wk_lds + 24 * 1024);                   // [s0] global walker ids in sum order
        double* tile = reinterpret_cast<double*>(wk_lds + 32 * 1024);          // [ALABI_WK_TILE]
        const double p0 = p.mvpar[2 * e];
        const int s0 = p0 == 0.0 ? Nc : (int)p0;
        if (s0 < 2 || s0 > Nc || Nc > ALABI_WK_MAX_NC) return 0;               // checked where the moves are set
        if (p.inj.idx) {
            int bad = 0;
            for (int m = tid; m < s0; m += T) {
                const int j = p.inj.idx[(size_t)w * s0 + m];
                int c = -1;
                if ((unsigned)j < (unsigned)Nc) c = clist[j];
                if (c < 0) bad = 1;
                for (int m2 = 0; m2 < m; ++m2) bad |= (p.inj.idx[(size_t)w * s0 + m2] == j);
                J[m] = c;
                zl[m] = p.inj.z[(size_t)w * s0 + m];
            }
            if (__syncthreads_or(bad)) return 0;
        } else if (s0 == Nc) {
            for (int j = tid; j < Nc; j += T) {
                J[j] = clist[j];
                zl[j] = philox_normal(s_lo, s_hi, (uint32_t)w, 7u + 16u * (uint32_t)j, k0, k1);
            }
            __syncthreads();
        } else {
            uint32_t r[4];
            for (int j = tid; j < Nc; j += T) {
                philox4x32_10(s_lo, s_hi, (uint32_t)w, 6u + 16u * (uint32_t)(j >> 1), k0, k1, r);
                keys[j] = (j & 1) ? (((uint64_t)r[2] << 32) | r[3]) : (((uint64_t)r[0] << 32) | r[1]);
            }
            __syncthreads();
            for (int j = tid; j < Nc; j += T) {
                const uint64_t kj = keys[j];
                int rk = 0;
                for (int i = 0; i < Nc; ++i) { const uint64_t ki = keys[i]; rk += (ki < kj || (ki == kj && i < j)) ? 1 : 0; }
                rank[j] = rk;
            }
            __syncthreads();                                                   // the keys are dead: zl takes their place
            for (int j = tid; j < Nc; j += T) {
                if (rank[j] >= s0) continue;
                int pos = 0;
                for (int i = 0; i < j; ++i) pos += rank[i] < s0 ? 1 : 0;
                J[pos] = clist[j];
                zl[pos] = philox_normal(s_lo, s_hi, (uint32_t)w, 7u + 16u * (uint32_t)j, k0, k1);
            }
            __syncthreads();
        }
        // rows of J through an LDS tile (loaded by all threads), summed by lane k in the order m = 0 .. s0-1: mean, then the walk sum
        const int rows = ALABI_WK_TILE / d;
        double mean = 0.0, acc = 0.0;
        for (int pass = 0; pass < 2; ++pass) {
            for (int m0 = 0; m0 < s0; m0 += rows) {
                const int nr = s0 - m0 < rows ? s0 - m0 : rows;
                for (int idx = tid; idx < nr * d; idx += T) tile[idx] = p.coords[(size_t)J[m0 + idx / d] * d + idx % d];
                __syncthreads();
                if (in) {
                    if (pass == 0) for (int m = 0; m < nr; ++m) mean += tile[m * d + tid];
                    else for (int m = 0; m < nr; ++m) acc += zl[m0 + m] * (tile[m * d + tid] - mean);
                }
                __syncthreads();
            }
            if (pass == 0) mean = mean / (double)s0;
        }
        const double scale = 1.0 / sqrt((double)s0 - 1.0);
        qc = sv + scale * acc;
        return 1;
    }
    // ---- KDE
    if (p.kde.flag[e]) { reject = 1; qc = sv; return 1; }                      // workgroup-uniform
    double* Ls = reinterpret_cast<double*>(wk_lds);                            // [d, d] (32 KB at d = 64)
    double* yx = reinterpret_cast<double*>(wk_lds + 32 * 1024);                // [d] whitened walker
    double* yq = yx + ALABI_MAX_DIM;                                           // [d] whitened proposal
    int ri;
    if (p.inj.idx) ri = p.inj.idx[w];
    else {
        uint32_t r[4];
        philox4x32_10(s_lo, s_hi, (uint32_t)w, 8u, k0, k1, r);
        ri = (int)(((uint64_t)r[0] * (uint64_t)Nc) >> 32);
    }
    if ((unsigned)ri >= (unsigned)Nc) return 0;                                // workgroup-uniform
    const int cr = clist[ri];
    if (cr < 0) return 0;                                                      // a test entry's list with a bad walker id
    for (int idx = tid; idx < d * d; idx += T) Ls[idx] = p.kde.L[(size_t)e * d * d + idx];
    __syncthreads();
    if (tid < 64) {                                                            // wave 0; lanes >= d carry zeros
        double z = 0.0, crk = 0.0, mk = 0.0;
        if (in) {
            z = p.inj.z ? p.inj.z[(size_t)w * d + tid] : philox_normal(s_lo, s_hi, (uint32_t)w, 8u + 16u * (uint32_t)(1 + tid), k0, k1);
            crk = p.coords[(size_t)cr * d + tid];
            mk = p.kde.mean[(size_t)e * d + tid];
        }
        double acc = 0.0;                                                      // (L z)_k = sum_{m <= k} L[k][m] z_m, m ascending
        for (int m = 0; m < d; ++m) {
            const double zm = lane_bcast(z, m);
            if (in && m <= tid) acc += Ls[tid * d + m] * zm;
        }
        qc = crk + acc;
        // y = L^-1 (v - mean) for v = walker, proposal: column-oriented forward substitution, lane k keeps row k's residual
        double bx = sv - mk, bq = qc - mk;
        for (int i = 0; i < d; ++i) {
            if (tid == i) { const double lii = Ls[i * d + i]; bx = bx / lii; bq = bq / lii; }
            const double yxi = lane_bcast(bx, i), yqi = lane_bcast(bq, i);
            if (in && tid > i) { const double lki = Ls[tid * d + i]; bx -= lki * yxi; bq -= lki * yqi; }
        }
        if (in) { yx[tid] = bx; yq[tid] = bq; }
    }
    __syncthreads();
    // the two log-sum-exps over the whitened rows, every thread a strided share, merged in a fixed tree
    double mx = -INFINITY, sx = 0.0, mq = -INFINITY, sq = 0.0;
    const double* white = p.kde.white + (size_t)e * p.n0 * d;                  // n0 = the larger half
    for (int j = tid; j < Nc; j += T) {
        const double* row = white + (size_t)j * d;
        double ax = 0.0, aq = 0.0;
        for (int k = 0; k < d; ++k) {
            const double y = row[k];
            const double dx = yx[k] - y, dq = yq[k] - y;
            ax = fma(dx, dx, ax);
            aq = fma(dq, dq, aq);
        }
        lse_merge(mx, sx, -0.5 * ax, 1.0);
        lse_merge(mq, sq, -0.5 * aq, 1.0);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lse_merge(mx, sx, __shfl_xor(mx, off, 64), __shfl_xor(sx, off, 64));
        lse_merge(mq, sq, __shfl_xor(mq, off, 64), __shfl_xor(sq, off, 64));
    }
    if ((tid & 63) == 0) { wk_red[0][tid >> 6][0] = mx; wk_red[0][tid >> 6][1] = sx; wk_red[1][tid >> 6][0] = mq; wk_red[1][tid >> 6][1] = sq; }
    __syncthreads();
    mx = wk_red[0][0][0]; sx = wk_red[0][0][1]; mq = wk_red[1][0][0]; sq = wk_red[1][0][1];
    for (int k = 1; k < (T >> 6); ++k) {
        lse_merge(mx, sx, wk_red[0][k][0], wk_red[0][k][1]);
        lse_merge(mq, sq, wk_red[1][k][0], wk_red[1][k][1]);
    }
    lnfac = (mx + log(sx)) - (mq + log(sq));
    if (tid == 0 && p.inj.lnfac_out) p.inj.lnfac_out[w] = lnfac;
    return 1;
}

// Pre-pass of a KDE half step: one workgroup per ensemble.  Not a KDE step (the move is chosen on the device): exits at once.
// mean_k = (sum_j c_jk) / Nc, cov_ab = (sum_j (c_ja - mean_a)(c_jb - mean_b)) / (Nc - 1), every sum over j ascending from 0.0 with
// rounded products, H = (f f) cov, left-looking Cholesky (t = H_ij - sum_{k<j} L_ik L_jk, k ascending; L_jj = sqrt(t_jj),
// L_ij = t_ij / L_jj), rows whitened by forward substitution -- the order tests/walk_kde_numpy.py states.
__global__ void __launch_bounds__(256)
ens_kde_prepass_kernel(HalfArgs p) {
    __shared__ double Ls[ALABI_MAX_DIM * ALABI_MAX_DIM];
    __shared__ double tile[ALABI_WK_TILE];                                     // rows of the half, loaded by all threads, read in order
    __shared__ double mean_s[ALABI_MAX_DIM];
    const int e = blockIdx.x, tid = threadIdx.x, d = p.d;
    if (p.mvkind[e] != 4) return;
    const int Nc = p.split ? p.n0 : p.W - p.n0;
    const int* clist = p.rec.order + (size_t)e * p.W + (p.split ? 0 : p.n0);
    const double f = p.mvpar[2 * e + (p.split ? 1 : 0)];
    const int rows = ALABI_WK_TILE / d;
    int bad = 0;
    for (int j = tid; j < Nc; j += 256) bad |= ((unsigned)clist[j] >= (unsigned)(p.W * gridDim.x)) ? 1 : 0;   // a test entry's list
    bad = __syncthreads_or(bad);
    if (!bad) {
        double m = 0.0;
        for (int j0 = 0; j0 < Nc; j0 += rows) {
            const int nr = Nc - j0 < rows ? Nc - j0 : rows;
            for (int idx = tid; idx < nr * d; idx += 256) tile[idx] = p.coords[(size_t)clist[j0 + idx / d] * d + idx % d];
            __syncthreads();
            if (tid < d) for (int r = 0; r < nr; ++r) m += tile[r * d + tid];
            __syncthreads();
        }
        if (tid < d) {
            m = m / (double)Nc;
            mean_s[tid] = m;
            p.kde.mean[(size_t)e * d + tid] = m;
        }
        __syncthreads();
        // covariance: entry idx = a (a + 1) / 2 + b, b <= a; a thread owns entries tid, tid + 256, ... (at most 9 at d = 64)
        constexpr int NQ = (ALABI_MAX_DIM * (ALABI_MAX_DIM + 1) / 2 + 255) / 256;
        const int ne = d * (d + 1) / 2;
        int ea[NQ], eb[NQ];
        double sum[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            int a = 0, rem = tid + 256 * q;
            if (rem < ne) while (rem > a) { rem -= a + 1; ++a; }
            ea[q] = a; eb[q] = rem < ne ? rem : 0; sum[q] = 0.0;
        }
        for (int j0 = 0; j0 < Nc; j0 += rows) {
            const int nr = Nc - j0 < rows ? Nc - j0 : rows;
            for (int idx = tid; idx < nr * d; idx += 256)
                tile[idx] = p.coords[(size_t)clist[j0 + idx / d] * d + idx % d] - mean_s[idx % d];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (tid + 256 * q < ne)
                    for (int r = 0; r < nr; ++r) sum[q] += tile[r * d + ea[q]] * tile[r * d + eb[q]];
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (tid + 256 * q < ne) Ls[ea[q] * d + eb[q]] = (f * f) * (sum[q] / ((double)Nc - 1.0));
        __syncthreads();
        for (int j = 0; j < d && !bad; ++j) {
            double t = 0.0;
            const int i = j + tid;                                             // row of column j this thread forms (d <= 64 < 256)
            if (i < d) {
                t = Ls[i * d + j];
                for (int k = 0; k < j; ++k) t -= Ls[i * d + k] * Ls[j * d + k];
                if (i == j) Ls[j * d + j] = t;
            }
            __syncthreads();
            const double piv = Ls[j * d + j];
            bad = !(piv > 0.0) || !(piv < INFINITY);
            __syncthreads();
            if (!bad && i < d) { const double ljj = sqrt(piv); Ls[i * d + j] = (i == j) ? ljj : t / ljj; }
            __syncthreads();
        }
    }
    if (tid == 0) {
        p.kde.flag[e] = bad;
        if (bad) atomicAdd(p.kde.singular, 1ull);
    }
    if (bad) return;
    for (int idx = tid; idx < d * d; idx += 256) p.kde.L[(size_t)e * d * d + idx] = (idx % d <= idx / d) ? Ls[idx] : 0.0;
    // whitened rows: a tile of centred rows, one thread per row substitutes forward in place, the tile goes out as it lies
    double* white = p.kde.white + (size_t)e * p.n0 * d;
    for (int j0 = 0; j0 < Nc; j0 += rows) {
        const int nr = Nc - j0 < rows ? Nc - j0 : rows;
        for (int idx = tid; idx < nr * d; idx += 256)
            tile[idx] = p.coords[(size_t)clist[j0 + idx / d] * d + idx % d] - mean_s[idx % d];
        __syncthreads();
        for (int r = tid; r < nr; r += 256) {
            double* row = tile + r * d;
            for (int i = 0; i < d; ++i) {
                double t = row[i];
                for (int k = 0; k < i; ++k) t -= Ls[i * d + k] * row[k];
                row[i] = t / Ls[i * d + i];
            }
        }
        __syncthreads();
        for (int idx = tid; idx < nr * d; idx += 256) white[(size_t)j0 * d + idx] = tile[idx];
        __syncthreads();
    }
}

// DE: the instantiation that reads the records' second partner (HalfArgs::cw2) and branches, workgroup-uniformly, on the
// record's kind; without it the code is the stretch move's alone.  SNK (with DE): the one that reads the third partner as well
// (HalfArgs::cw3) and forms a snooker record's proposal and log factor; stretch and DE records take the branches they take in the
// DE instantiation.  WK (with SNK): the one that also forms the proposals of walk and KDE steps (wk_proposal), on a workgroup-uniform
// branch on the step's kind; every other record takes the branch it takes in the snooker instantiation.
template <int D, bool GENERIC, bool DE, bool SNK = false, bool WK = false>
__device__ __forceinline__ void ens_half_body(const HalfArgs& p) {
    static_assert(DE || !SNK, "the three-partner instantiation reads the second partner too");
    static_assert(SNK || !WK, "the whole-half instantiation takes snooker records too");
    __shared__ double q_s[ALABI_MAX_DIM], qs_s[ALABI_MAX_DIM], old_s[ALABI_MAX_DIM];
    __shared__ double scratch[16];
    const int tid = threadIdx.x, T = blockDim.x;
    const int e = blockIdx.y;
    const size_t pos = (size_t)e * p.W + (p.split ? p.n0 : 0) + p.part_begin + blockIdx.x;
    // (1) Issue this thread's first training-point loads right away (16 B per lane: points 2*tid and
    //     2*tid+1 of every coordinate row): they do not depend on the proposal, so their latency -- every
    //     kernel starts with a cold L2 on this chip, and a CU ingests only ~64 B/clk -- overlaps the
    //     record -> coords chain below.
    const int half = p.Npad >> 1;                 // Npad is a multiple of 64
    const bool vA = tid < half;
    const double* Xsrc = GENERIC ? p.Xt : p.Xc;        // squared exponential: centred inputs and h instead of alpha (se_pair_terms)
    const double* Asrc = GENERIC ? p.alpha : p.ens_h;
    f64x2 xa[D];
#pragma unroll
    for (int k = 0; k < D; ++k)
        xa[k] = vA ? reinterpret_cast<const f64x2*>(Xsrc + (size_t)k * p.Npad)[tid] : f64x2{0.0, 0.0};
    const f64x2 aa = vA ? reinterpret_cast<const f64x2*>(Asrc)[tid] : (GENERIC ? f64x2{0.0, 0.0} : f64x2{ALABI_SE_PAD, ALABI_SE_PAD});
    // (2) proposal record: one dependent load away from blockIdx
    const int w = p.rec.order[pos];
    if (w < 0) return;  // inert record (range-checked test input); workgroup-uniform
    const int cw = p.rec.cw[pos];
    const double zz = p.rec.zz[pos];
    const int cw2 = DE ? p.cw2[pos] : -1;         // second partner of a differential-evolution record, -1: a stretch record
    const int cw3 = SNK ? p.cw3[pos] : -1;        // third partner of a snooker record, -1: a stretch or DE record
    const bool snk = SNK && cw3 >= 0;
    const bool de = DE && cw2 >= 0 && !snk;
    // where the two rows live: in place (coords / logp), or -- sharded ensemble -- in the history of published rows
    const double* own_c = p.coords + (size_t)w * p.d;
    const double* own_lp = p.logp + w;
    const double* par_c = p.coords + (size_t)cw * p.d;
    const double* par2_c = p.coords + (size_t)(de || snk ? cw2 : cw) * p.d;
    if (p.shist) {
        const unsigned long long lw = p.rec.link[2 * pos];
        const int so = (int)(unsigned)(lw & 0xffffffffull), sp = (int)(unsigned)(lw >> 32);
        if (so >= 0) { own_c = p.shist + so; own_lp = own_c + p.d; }
        if (sp >= 0) par_c = p.shist + sp;
    }
    double lp_old = 0.0, lnfac = 0.0, lnu = 0.0;
    if (tid < 64) { lp_old = *own_lp; lnfac = p.rec.lnfac[pos]; lnu = p.rec.lnu[pos]; }  // wave 0 decides
    const double* inv_len = p.consts;
    const double* lo = p.consts + ALABI_MAX_DIM;
    const double* hi = p.consts + 2 * ALABI_MAX_DIM;
    int ok = 1;
    const int wkind = WK ? p.mvkind[e] : 0;                // kind of the step's move; workgroup-uniform
    if (WK && wkind >= 3) {
        const bool in = tid < p.d;
        const double sv = in ? own_c[tid] : 0.0;
        double qc, lf;
        int rej;
        if (!wk_proposal<D>(p, wkind, e, w, sv, qc, lf, rej)) return;   // a test entry's bad subset: the walker stays as it is
        lnfac = lf;
        if (rej) ok = 0;                                   // the KDE of this half step has no factor: rejected like a proposal outside the box
        if (tid < D) {
            double qv = 0.0;
            if (in) {
                ok = ok && (qc > lo[tid]) && (qc < hi[tid]);
                q_s[tid] = qc; old_s[tid] = sv;
                qv = qc * inv_len[tid];
                if (!GENERIC) qv -= p.centre[tid];
            }
            qs_s[tid] = qv;
        }
    } else if (tid < D) {
        double qv = 0.0;
        if (SNK && snk) {                                  // workgroup-uniform; lanes d .. D-1 take part in the sums with zeros
            const bool in = tid < p.d;
            const double* par3_c = p.coords + (size_t)cw3 * p.d;
            const double sv = in ? own_c[tid] : 0.0, zv = in ? par_c[tid] : 0.0;
            const double z1v = in ? par2_c[tid] : 0.0, z2v = in ? par3_c[tid] : 0.0;
            double lf;
            const double qc = snooker_coord<D>(p.d, sv, zv, z1v, z2v, zz, lf);
            if (in) {
                lnfac = lf;                                // in the lanes that use the accept flag: 0 .. d-1
                ok = (qc > lo[tid]) && (qc < hi[tid]);
                q_s[tid] = qc; old_s[tid] = sv;
                qv = qc * inv_len[tid];
                if (!GENERIC) qv -= p.centre[tid];
            }
        } else if (tid < p.d) {
            const double cv = par_c[tid];
            const double sv = own_c[tid];
            qv = DE ? propose_coord(de, sv, cv, par2_c[tid], zz) : cv - (cv - sv) * zz;
            ok = (qv > lo[tid]) && (qv < hi[tid]);
            q_s[tid] = qv; old_s[tid] = sv;
            qv *= inv_len[tid];
            if (!GENERIC) qv -= p.centre[tid];
        }
        qs_s[tid] = qv;
    }
    const int inb = __syncthreads_and(ok);
    double lp_new = -INFINITY;
    if (inb) {  // workgroup-uniform
        double q[D];
#pragma unroll
        for (int k = 0; k < D; ++k) q[k] = qs_s[k];
        const double acc = half_lane_sum<D, GENERIC>(xa, aa, q, Xsrc, Asrc, p.Npad, tid, T, p.kf);
        // (3) wave totals by DPP, one LDS word per wave, ONE barrier; only wave 0 goes on
        const double wsum = wave_sum_dpp(acc);
        if ((tid & 63) == 63) scratch[tid >> 6] = wsum;
        __syncthreads();
        if (tid >= 64) return;
        const int nw = T >> 6;
        double part = (tid < nw) ? scratch[tid] : 0.0;
        part = wave_sum_dpp(part);   // fixed order: bit-reproducible
        const double s = lane_bcast(part, 63);
        lp_new = fma(p.amp, s, p.mean);
        if (p.ymap) lp_new = apply_ymap(lp_new, p.ymap);
        if (p.has_prior)
            lp_new += normal_prior_sum(p.consts + 3 * ALABI_MAX_DIM, p.consts + 4 * ALABI_MAX_DIM, tid, p.d, q_s[tid]) + p.prior_const;
    } else if (tid >= 64) {
        return;
    }
    // (4) wave 0: accept test in every lane (same inputs), first d lanes write the state
    const int acc_flag = (lnfac + lp_new - lp_old > lnu) ? 1 : 0;
    if (p.sout) {                                          // sharded ensemble: the new row goes to the history, nothing else is written
        double* o = p.sout + (size_t)blockIdx.x * (p.d + 2);
        if (tid < p.d) o[tid] = acc_flag ? q_s[tid] : old_s[tid];
        if (tid == 0) { o[p.d] = acc_flag ? lp_new : lp_old; o[p.d + 1] = acc_flag ? 1.0 : 0.0; }
        return;
    }
    if (acc_flag) {
        if (tid < p.d) p.coords[(size_t)w * p.d + tid] = q_s[tid];
        if (tid == 0) {
            p.logp[w] = lp_new;
            if (p.n_accept) p.n_accept[w] += 1;
        }
    }
    if (p.chain || p.chain_logp) {
        const long long done = p.run_state[1] + p.local_t + 1;
        if (done % p.thin_by == 0) {
            const size_t slot = (size_t)(done / p.thin_by - 1);
            const size_t WT = (size_t)p.W * gridDim.y;
            if (p.chain && tid < p.d)
                __builtin_nontemporal_store(acc_flag ? q_s[tid] : old_s[tid], &p.chain[(slot * WT + w) * p.d + tid]);
            if (p.chain_logp && tid == 0)
                __builtin_nontemporal_store(acc_flag ? lp_new : lp_old, &p.chain_logp[slot * WT + w]);
        }
    }
}

template <int D, bool GENERIC>
__global__ void __launch_bounds__(1024)
ens_half_kernel(HalfArgs p) { ens_half_body<D, GENERIC, false>(p); }

template <int D, bool GENERIC>
__global__ void __launch_bounds__(1024)
ens_half_de_kernel(HalfArgs p) { ens_half_body<D, GENERIC, true>(p); }

template <int D, bool GENERIC>
__global__ void __launch_bounds__(1024)
ens_half_snooker_kernel(HalfArgs p) { ens_half_body<D, GENERIC, true, true>(p); }

template <int D, bool GENERIC>
__global__ void __launch_bounds__(1024)
ens_half_wk_kernel(HalfArgs p) { ens_half_body<D, GENERIC, true, true, true>(p); }

// NP proposals of the same half step per workgroup: the training set is streamed ONCE per workgroup and used for all of them.
// With more proposals than CUs (W/2 > 256, or E ensembles) ens_half_kernel is bound by L2 -> CU bandwidth: every workgroup
// pulls the whole X (440 KB at N = 5000, d = 10) for one proposal.  Per proposal the arithmetic, the lane -> point map and the
// reduction order are those of ens_half_kernel with the same block size, so the two kernels agree bit for bit.
template <int D, bool GENERIC, int NP, bool DE>
__device__ __forceinline__ void ens_half_multi_body(const HalfArgs& p) {
    __shared__ double q_s[NP][ALABI_MAX_DIM], qs_s[NP][ALABI_MAX_DIM], old_s[NP][ALABI_MAX_DIM];
    __shared__ double scratch[NP][16];
    __shared__ int ok_s[NP], w_s[NP];
    __shared__ double lpold_s[NP], lnfac_s[NP], lnu_s[NP];
    const int tid = threadIdx.x, T = blockDim.x;
    const int e = blockIdx.y;
    const int first = blockIdx.x * NP;
    const double* inv_len = p.consts;
    const double* lo = p.consts + ALABI_MAX_DIM;
    const double* hi = p.consts + 2 * ALABI_MAX_DIM;
    if (tid < NP) ok_s[tid] = 1;
    __syncthreads();
    // (1) the NP proposals: thread (pp, k) forms coordinate k of proposal pp
    for (int idx = tid; idx < NP * D; idx += T) {
        const int pp = idx / D, k = idx % D;
        int w = -1;
        if (first + pp < p.count) {
            const size_t pos = (size_t)e * p.W + (p.split ? p.n0 : 0) + p.part_begin + first + pp;
            w = p.rec.order[pos];
            if (w >= 0) {
                double qv = 0.0;
                if (k < p.d) {
                    const int cw = p.rec.cw[pos];
                    const double zz = p.rec.zz[pos];
                    const double cv = p.coords[(size_t)cw * p.d + k];
                    const double sv = p.coords[(size_t)w * p.d + k];
                    if (DE) {
                        const int cw2 = p.cw2[pos];
                        qv = propose_coord(cw2 >= 0, sv, cv, p.coords[(size_t)(cw2 >= 0 ? cw2 : cw) * p.d + k], zz);
                    } else qv = cv - (cv - sv) * zz;
                    if (!((qv > lo[k]) && (qv < hi[k]))) ok_s[pp] = 0;
                    q_s[pp][k] = qv; old_s[pp][k] = sv;
                    qv *= inv_len[k];
                    if (!GENERIC) qv -= p.centre[k];
                }
                qs_s[pp][k] = qv;
                if (k == 0) { lpold_s[pp] = p.logp[w]; lnfac_s[pp] = p.rec.lnfac[pos]; lnu_s[pp] = p.rec.lnu[pos]; }
            }
        }
        if (k == 0) w_s[pp] = w;
    }
    __syncthreads();
    // (2) kernel sums: X pairs streamed once, NP accumulators
    double q[NP][D];
    bool live[NP];
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) {
        live[pp] = w_s[pp] >= 0 && ok_s[pp];
#pragma unroll
        for (int k = 0; k < D; ++k) q[pp][k] = qs_s[pp][k];
    }
    double acc[NP];
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) acc[pp] = 0.0;
    const int half = p.Npad >> 1;
    bool first_pair = true;
    const double* Xsrc = GENERIC ? p.Xt : p.Xc;
    const double* Asrc = GENERIC ? p.alpha : p.ens_h;
    double nhq[NP];
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) nhq[pp] = GENERIC ? 0.0 : se_neg_half_norm<D>(q[pp]);
    for (int j = tid; j < half; j += T) {
        f64x2 x[D];
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] = reinterpret_cast<const f64x2*>(Xsrc + (size_t)k * p.Npad)[j];
        const f64x2 al = reinterpret_cast<const f64x2*>(Asrc)[j];
#pragma unroll
        for (int pp = 0; pp < NP; ++pp) {
            if (!GENERIC) {                                   // (se_pair_terms: the order of ens_half_kernel, acc += term_a; acc += term_b)
                double fa, fb;
                se_pair_terms<D>(x, al, q[pp], nhq[pp], fa, fb);
                acc[pp] += fa; acc[pp] += fb;
                continue;
            }
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double d0 = x[k].x - q[pp][k], d1 = x[k].y - q[pp][k];
                s0 = fma(d0, d0, s0);
                s1 = fma(d1, d1, s1);
            }
            // ens_half_kernel's order: the lane's first pair enters by a multiply, every later term by an fma
            acc[pp] = first_pair ? al.x * radial<GENERIC>(s0, p.kf) : fma(al.x, radial<GENERIC>(s0, p.kf), acc[pp]);
            acc[pp] = fma(al.y, radial<GENERIC>(s1, p.kf), acc[pp]);
        }
        first_pair = false;
    }
    // a lane without any pair (tid >= half) contributes aa = 0: 0 * f + 0 * f = 0 exactly, as in ens_half_kernel
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) {
        const double wsum = wave_sum_dpp(acc[pp]);
        if ((tid & 63) == 63) scratch[pp][tid >> 6] = wsum;
    }
    __syncthreads();
    if (tid >= 64) return;
    // (3) wave 0: accept tests and state updates, one proposal after the other
    const int nw = T >> 6;
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) {
        const int w = w_s[pp];
        if (w < 0) continue;                              // beyond the launch's proposals, or an inert record
        double lp_new = -INFINITY;
        if (ok_s[pp]) {
            double part = (tid < nw) ? scratch[pp][tid] : 0.0;
            part = wave_sum_dpp(part);
            lp_new = fma(p.amp, lane_bcast(part, 63), p.mean);
            if (p.ymap) lp_new = apply_ymap(lp_new, p.ymap);
            if (p.has_prior)
                lp_new += normal_prior_sum(p.consts + 3 * ALABI_MAX_DIM, p.consts + 4 * ALABI_MAX_DIM, tid, p.d, q_s[pp][tid]) +
                          p.prior_const;
        }
        const double lp_old = lpold_s[pp];
        const int acc_flag = (lnfac_s[pp] + lp_new - lp_old > lnu_s[pp]) ? 1 : 0;
        if (acc_flag) {
            if (tid < p.d) p.coords[(size_t)w * p.d + tid] = q_s[pp][tid];
            if (tid == 0) {
                p.logp[w] = lp_new;
                if (p.n_accept) p.n_accept[w] += 1;
            }
        }
        if (p.chain || p.chain_logp) {
            const long long done = p.run_state[1] + p.local_t + 1;
            if (done % p.thin_by == 0) {
                const size_t slot = (size_t)(done / p.thin_by - 1);
                const size_t WT = (size_t)p.W * gridDim.y;
                if (p.chain && tid < p.d)
                    __builtin_nontemporal_store(acc_flag ? q_s[pp][tid] : old_s[pp][tid], &p.chain[(slot * WT + w) * p.d + tid]);
                if (p.chain_logp && tid == 0)
                    __builtin_nontemporal_store(acc_flag ? lp_new : lp_old, &p.chain_logp[slot * WT + w]);
            }
        }
    }
}

template <int D, bool GENERIC, int NP>
__global__ void __launch_bounds__(512)
ens_half_multi_kernel(HalfArgs p) { ens_half_multi_body<D, GENERIC, NP, false>(p); }

template <int D, bool GENERIC, int NP>
__global__ void __launch_bounds__(512)
ens_half_multi_de_kernel(HalfArgs p) { ens_half_multi_body<D, GENERIC, NP, true>(p); }

template <int D>
__global__ void __launch_bounds__(1024)
ens_lnprob_kernel(const double* __restrict__ coords, int d, const double* __restrict__ Xt,
                  const double* __restrict__ alpha, int Npad, double amp, double mean, KernelFn kf,
                  const double* __restrict__ consts, int has_prior, double prior_const, int ymap, int gate_box,
                  double* __restrict__ logp) {
    __shared__ double qs_s[ALABI_MAX_DIM];
    __shared__ double scratch[16];
    __shared__ double prior_s;
    const int tid = threadIdx.x, w = blockIdx.x;
    int ok = 1;
    double qraw = 0.0;
    if (tid < D) {
        double qv = 0.0;
        if (tid < d) {
            qv = coords[(size_t)w * d + tid];
            qraw = qv;
            ok = (qv > consts[ALABI_MAX_DIM + tid]) && (qv < consts[2 * ALABI_MAX_DIM + tid]);
            qv *= consts[tid];
        }
        qs_s[tid] = qv;
    }
    if (tid < 64) {
        const double pr = has_prior ? normal_prior_sum(consts + 3 * ALABI_MAX_DIM, consts + 4 * ALABI_MAX_DIM, tid, d, qraw) + prior_const
                                    : 0.0;
        if (tid == 0) prior_s = pr;
    }
    const int inb = __syncthreads_and(ok) || !gate_box;
    double lp = -INFINITY;
    if (inb) lp = apply_ymap(fma(amp, gp_kernel_dot_block<D>(Xt, alpha, Npad, qs_s, scratch, kf), mean), ymap) + prior_s;
    if (tid == 0) logp[w] = lp;
}

// ---------------------------------------------------------------------------------------------------
// Generic log-probability path: the reference's lnprob is like_fn(theta) + prior_fn(theta) with ARBITRARY Python
// callables (alabi/core.py:2073-2100, :2253-2280).  A half step is then split in two launches around the host call:
//   ens_propose_kernel  one workgroup per proposal of the half: forms q (same arithmetic as ens_half_kernel), writes it
//                       in list order, and -- when `like` is given -- the surrogate part y_scaler^-1(GP mean) at q
//                       (box-gated to -inf only if gate_box, i.e. when the prior is the uniform box itself);
//   (host)              lp_new = like + prior_fn(q)   [or like_fn(q) + prior_fn(q)]
//   ens_accept_kernel   one thread per proposal: accept test with the record's (d-1) ln z and ln u', state update.
// The ensemble, the draws and the accept decisions stay on the device; only the proposals of a half step travel.
template <int D, bool GENERIC, bool DE, bool SNK = false, bool WK = false>
__device__ __forceinline__ void ens_propose_body(const HalfArgs& p, int gate_box, double* __restrict__ q_out, double* __restrict__ like_out) {
    __shared__ double qs_s[ALABI_MAX_DIM];
    __shared__ double scratch[16];
    const int tid = threadIdx.x;
    const size_t pos = (size_t)(p.split ? p.n0 : 0) + p.part_begin + blockIdx.x;
    const int w = p.rec.order[pos];
    if (w < 0) {                                       // inert record: a NaN proposal is rejected by the accept kernel
        if (tid < p.d) q_out[(size_t)blockIdx.x * p.d + tid] = __longlong_as_double(0x7FF8000000000000ll);
        if (tid == 0 && like_out) like_out[blockIdx.x] = -INFINITY;
        return;
    }
    const int cw = p.rec.cw[pos];
    const double zz = p.rec.zz[pos];
    const int cw2 = DE ? p.cw2[pos] : -1;
    const int cw3 = SNK ? p.cw3[pos] : -1;
    const bool snk = SNK && cw3 >= 0;
    const bool de = DE && cw2 >= 0 && !snk;
    int ok = 1;
    const int wkind = WK ? p.mvkind[0] : 0;
    if (WK && wkind >= 3) {                                // as in ens_half_body; a half step without a factor: q = the walker, factor -inf
        const bool in = tid < p.d;
        const double sv = in ? p.coords[(size_t)w * p.d + tid] : 0.0;
        double qc, lf;
        int rej;
        const int live = wk_proposal<D>(p, wkind, 0, w, sv, qc, lf, rej);
        if (tid == 0) p.rec.lnfac[pos] = (live && !rej) ? lf : -INFINITY;
        if (!live) qc = sv;
        if (tid < D) {
            double qv = 0.0;
            if (in) {
                ok = (qc > p.consts[ALABI_MAX_DIM + tid]) && (qc < p.consts[2 * ALABI_MAX_DIM + tid]);
                q_out[(size_t)blockIdx.x * p.d + tid] = qc;
                qv = qc * p.consts[tid];
            }
            qs_s[tid] = qv;
        }
    } else if (tid < D) {
        double qv = 0.0;
        if (SNK && snk) {                                  // as in ens_half_body; the log factor goes where ens_accept_kernel reads it
            const bool in = tid < p.d;
            const double sv = in ? p.coords[(size_t)w * p.d + tid] : 0.0, zv = in ? p.coords[(size_t)cw * p.d + tid] : 0.0;
            const double z1v = in ? p.coords[(size_t)cw2 * p.d + tid] : 0.0, z2v = in ? p.coords[(size_t)cw3 * p.d + tid] : 0.0;
            double lf;
            const double qc = snooker_coord<D>(p.d, sv, zv, z1v, z2v, zz, lf);
            if (tid == 0) p.rec.lnfac[pos] = lf;
            if (in) {
                ok = (qc > p.consts[ALABI_MAX_DIM + tid]) && (qc < p.consts[2 * ALABI_MAX_DIM + tid]);
                q_out[(size_t)blockIdx.x * p.d + tid] = qc;
                qv = qc * p.consts[tid];
            }
        } else if (tid < p.d) {
            const double cv = p.coords[(size_t)cw * p.d + tid];
            const double sv = p.coords[(size_t)w * p.d + tid];
            qv = DE ? propose_coord(de, sv, cv, p.coords[(size_t)(de ? cw2 : cw) * p.d + tid], zz) : cv - (cv - sv) * zz;
            ok = (qv > p.consts[ALABI_MAX_DIM + tid]) && (qv < p.consts[2 * ALABI_MAX_DIM + tid]);
            q_out[(size_t)blockIdx.x * p.d + tid] = qv;
            qv *= p.consts[tid];
        }
        qs_s[tid] = qv;
    }
    const int inb = __syncthreads_and(ok) || !gate_box;
    if (!like_out) return;
    double lp = -INFINITY;
    if (inb) lp = apply_ymap(fma(p.amp, gp_kernel_dot_block<D, GENERIC>(p.Xt, p.alpha, p.Npad, qs_s, scratch, p.kf), p.mean), p.ymap);
    if (tid == 0) like_out[blockIdx.x] = lp;
}

template <int D, bool GENERIC>
__global__ void __launch_bounds__(1024)
ens_propose_kernel(HalfArgs p, int gate_box, double* __restrict__ q_out, double* __restrict__ like_out) {
    ens_propose_body<D, GENERIC, false>(p, gate_box, q_out, like_out);
}

template <int D, bool GENERIC>
__global__ void __launch_bounds__(1024)
ens_propose_de_kernel(HalfArgs p, int gate_box, double* __restrict__ q_out, double* __restrict__ like_out) {
    ens_propose_body<D, GENERIC, true>(p, gate_box, q_out, like_out);
}

template <int D, bool GENERIC>
__global__ void __launch_bounds__(1024)
ens_propose_snooker_kernel(HalfArgs p, int gate_box, double* __restrict__ q_out, double* __restrict__ like_out) {
    ens_propose_body<D, GENERIC, true, true>(p, gate_box, q_out, like_out);
}

template <int D, bool GENERIC>
__global__ void __launch_bounds__(1024)
ens_propose_wk_kernel(HalfArgs p, int gate_box, double* __restrict__ q_out, double* __restrict__ like_out) {
    ens_propose_body<D, GENERIC, true, true, true>(p, gate_box, q_out, like_out);
}

__global__ void __launch_bounds__(256)
ens_accept_kernel(HalfArgs p, int count, const double* __restrict__ q, const double* __restrict__ lp_new) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const size_t pos = (size_t)(p.split ? p.n0 : 0) + p.part_begin + i;
    const int w = p.rec.order[pos];
    if (w < 0) return;
    const double lpn = lp_new[i], lpo = p.logp[w];
    if (p.rec.lnfac[pos] + lpn - lpo > p.rec.lnu[pos]) {      // false for NaN
        for (int k = 0; k < p.d; ++k) p.coords[(size_t)w * p.d + k] = q[(size_t)i * p.d + k];
        p.logp[w] = lpn;
        if (p.n_accept) p.n_accept[w] += 1;
    }
}

__global__ void ens_advance_kernel(long long* run_state, long long n) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { run_state[0] += n; run_state[1] += n; }
}

int ens_se_prepare(alabi_gp* gp, hipStream_t s) {
    if (gp->ens_h_gen == gp->gen && gp->Xc && gp->ens_h) return ALABI_OK;
    int st = ensure_xa(gp, s);                         // the centre of the scaled training inputs (per factor)
    if (st != ALABI_OK) return st;
    const int rows = dim_bucket(gp->d);
    if (!gp->Xc) ALABI_HIP_CHECK(hipMalloc(&gp->Xc, (size_t)ALABI_MAX_DIM * gp->n_cap * sizeof(double)));
    if (!gp->ens_h) ALABI_HIP_CHECK(hipMalloc(&gp->ens_h, (size_t)gp->n_cap * sizeof(double)));
    hipLaunchKernelGGL(ens_se_prepare_kernel, dim3((gp->Npad + 255) / 256), dim3(256), 0, s, gp->Xt, gp->xa_centre, gp->alpha, gp->N,
                       gp->Npad, gp->d, rows, gp->Xc, gp->ens_h);
    ALABI_LAUNCH_CHECK();
    gp->ens_h_gen = gp->gen;
    return ALABI_OK;
}

int launch_ens_draw(alabi_ens* e, int nsteps, double a, hipStream_t s) { return launch_ens_draw_at(e, e->draws, nsteps, a, true, 0, s); }

// from_state: the first global step of the chunk is run_state[0]; otherwise it is step0, by value
int launch_ens_draw_at(alabi_ens* e, const DrawBuffers& into, int nsteps, double a, bool from_state, long long step0, hipStream_t s) {
    int Wp = 1;
    while (Wp < e->W) Wp <<= 1;
    const size_t lds = (size_t)Wp * 12 + 1024;
    static bool attr_set = false;
    if (!attr_set && lds > 64 * 1024) {
        ALABI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(ens_draw_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    // the default move set is one stretch move with the call's `a`; the second-partner arrays belong to the first buffer set
    MoveTable mt = e->moves;
    if (mt.n == 0) { mt = MoveTable{}; mt.n = 1; mt.kind[0] = 0; mt.cum[0] = 1.0; mt.p0[0] = a; }
    const MoveBuffers mv = (into.order == e->draws.order) ? e->mv : MoveBuffers{};
    hipLaunchKernelGGL(ens_draw_kernel, dim3(nsteps, e->E), dim3(256), lds, s, e->seed, from_state ? e->run_state : nullptr,
                       from_state ? 0LL : step0, e->W, Wp, e->d, mt, into, mv);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_prep(alabi_ens* e, const int* order, int n0, const double* u_z, const int* partner,
                    const double* u_acc, double a, hipStream_t s) {
    hipLaunchKernelGGL(ens_prep_kernel, dim3((e->W + 255) / 256), dim3(256), 0, s, order, n0, e->W, u_z, partner, u_acc,
                       a, e->d, e->draws);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_prep_de(alabi_ens* e, const int* order, int n0, const int* j1, const int* j2, const double* gamma,
                       const double* u_acc, hipStream_t s) {
    hipLaunchKernelGGL(ens_prep_de_kernel, dim3((e->W + 255) / 256), dim3(256), 0, s, order, n0, e->W, j1, j2, gamma, u_acc,
                       e->draws, e->mv);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_prep_snooker(alabi_ens* e, const int* order, int n0, const int* j1, const int* j2, const int* j3, double gamma,
                            const double* u_acc, hipStream_t s) {
    hipLaunchKernelGGL(ens_prep_snooker_kernel, dim3((e->W + 255) / 256), dim3(256), 0, s, order, n0, e->W, j1, j2, j3, gamma, u_acc,
                       e->draws, e->mv);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_prep_wk(alabi_ens* e, const int* order, const double* u_acc, hipStream_t s) {
    hipLaunchKernelGGL(ens_prep_wk_kernel, dim3((e->W + 255) / 256), dim3(256), 0, s, order, e->W, u_acc, e->draws, e->mv);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_set_step_move(alabi_ens* e, int kind, double p0, double p1, hipStream_t s) {
    hipLaunchKernelGGL(ens_set_step_move_kernel, dim3(1), dim3(64), 0, s, e->mv, kind, p0, p1);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_gauss_export(alabi_ens* e, double* f, int* coord, double* z, hipStream_t s) {
    hipLaunchKernelGGL(ens_gauss_export_kernel, dim3((e->W * e->E + 255) / 256), dim3(256), 0, s, e->seed, e->run_state, e->W, e->E, e->d,
                       e->mv, f, coord, z);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

// in front of a half step of a set with a KDE move: one workgroup per ensemble, which leaves at once where the step's move is another
int launch_ens_kde_prepass(alabi_ens* e, const HalfArgs& args, hipStream_t s) {
    if (!args.mvkind || !args.mvpar || !args.kde.white || args.shist) return ALABI_BAD_ARGUMENT;
    hipLaunchKernelGGL(ens_kde_prepass_kernel, dim3(e->E), dim3(256), 0, s, args);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_half_args(alabi_ens* e, const HalfArgs& args_in, int nblocks, const EnsSwitches& sw, hipStream_t s) {
    if (nblocks <= 0) return ALABI_OK;
    const int db = dim_bucket(e->d);
    const int threads = e->threads;
    HalfArgs args = args_in;
    args.count = nblocks;
    // more proposals than CUs: NP per workgroup share one pass over the training set (same block size: same bits)
    const int np = ens_half_np(threads, e->d, (long long)nblocks * e->E, args.shist != nullptr, e->n_cu, sw);
    if (args.mvkind) {                                // a set with a walk or KDE move: one proposal per workgroup
        if (args.shist || !args.cw2 || !args.cw3 || !args.mvpar) return ALABI_BAD_ARGUMENT;
        ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, hipLaunchKernelGGL((ens_half_wk_kernel<D, GENERIC>), dim3(nblocks, e->E), dim3(threads), 0, s, args)));
    } else if (args.cw3) {                            // records with a third partner: one proposal per workgroup
        if (args.shist || !args.cw2) return ALABI_BAD_ARGUMENT;
        ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, hipLaunchKernelGGL((ens_half_snooker_kernel<D, GENERIC>), dim3(nblocks, e->E), dim3(threads), 0, s, args)));
    } else if (args.cw2) {                            // records with a second partner: the two-partner instantiations
        if (args.shist) return ALABI_BAD_ARGUMENT;    // the sharded history links one partner row
        if (np == 4) {
            ALABI_DISPATCH_DIM16(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, hipLaunchKernelGGL((ens_half_multi_de_kernel<D, GENERIC, 4>),
                dim3((nblocks + 3) / 4, e->E), dim3(threads), 0, s, args)));
        } else if (np == 2) {
            ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, hipLaunchKernelGGL((ens_half_multi_de_kernel<D, GENERIC, 2>),
                dim3((nblocks + 1) / 2, e->E), dim3(threads), 0, s, args)));
        } else {
            ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, hipLaunchKernelGGL((ens_half_de_kernel<D, GENERIC>), dim3(nblocks, e->E), dim3(threads), 0, s, args)));
        }
    } else if (np == 4) {
        ALABI_DISPATCH_DIM16(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, hipLaunchKernelGGL((ens_half_multi_kernel<D, GENERIC, 4>),
            dim3((nblocks + 3) / 4, e->E), dim3(threads), 0, s, args)));
    } else if (np == 2) {
        ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, hipLaunchKernelGGL((ens_half_multi_kernel<D, GENERIC, 2>),
            dim3((nblocks + 1) / 2, e->E), dim3(threads), 0, s, args)));
    } else {
        ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, hipLaunchKernelGGL((ens_half_kernel<D, GENERIC>), dim3(nblocks, e->E), dim3(threads), 0, s, args)));
    }
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_lnprob(alabi_ens* e, const double* coords, int nwalkers, double* logp, int gate_box, hipStream_t s) {
    const int db = dim_bucket(e->d);
    alabi_gp* gp = e->gp;
    ALABI_DISPATCH_DIM(db, hipLaunchKernelGGL(ens_lnprob_kernel<D>, dim3(nwalkers), dim3(e->threads), 0, s, coords, e->d,
                                              gp->Xt, gp->alpha, gp->Npad, e->lp_scale * exp(gp->log_amp),
                                              fma(e->lp_scale, gp->mean, e->lp_shift), gp->kf, e->consts, e->has_prior,
                                              e->prior_const, e->ymap, gate_box, logp));
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_propose(alabi_ens* e, const HalfArgs& args, int nblocks, int gate_box, double* q, double* like, hipStream_t s) {
    if (nblocks <= 0) return ALABI_OK;
    const int db = dim_bucket(e->d);
    if (args.mvkind) {
        if (!args.cw2 || !args.cw3 || !args.mvpar) return ALABI_BAD_ARGUMENT;
        ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, hipLaunchKernelGGL((ens_propose_wk_kernel<D, GENERIC>), dim3(nblocks),
                                                                                        dim3(e->threads), 0, s, args, gate_box, q, like)));
    } else if (args.cw3) {
        if (!args.cw2) return ALABI_BAD_ARGUMENT;
        ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, hipLaunchKernelGGL((ens_propose_snooker_kernel<D, GENERIC>), dim3(nblocks),
                                                                                        dim3(e->threads), 0, s, args, gate_box, q, like)));
    } else if (args.cw2) {
        ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, hipLaunchKernelGGL((ens_propose_de_kernel<D, GENERIC>), dim3(nblocks),
                                                                                        dim3(e->threads), 0, s, args, gate_box, q, like)));
    } else {
        ALABI_DISPATCH_DIM(db, ALABI_DISPATCH_KERNEL(e->gp->kf.type, hipLaunchKernelGGL((ens_propose_kernel<D, GENERIC>), dim3(nblocks),
                                                                                        dim3(e->threads), 0, s, args, gate_box, q, like)));
    }
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_accept(alabi_ens* e, const HalfArgs& args, int count, const double* q, const double* lp_new, hipStream_t s) {
    if (count <= 0) return ALABI_OK;
    hipLaunchKernelGGL(ens_accept_kernel, dim3((count + 255) / 256), dim3(256), 0, s, args, count, q, lp_new);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_ens_advance(alabi_ens* e, long long n, hipStream_t s) {
    hipLaunchKernelGGL(ens_advance_kernel, dim3(1), dim3(64), 0, s, e->run_state, n);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // namespace alabi
