// How an ensemble handle is laid out and which way alabi_ens_run takes: the environment switches of the ensemble sampler (read in
// ONE place, ens_plan.hip) and pure functions of (shape of the handle, n_cu, switches).  ens_api.hip, ens_run.hip and the launchers
// of ensemble.hip / ens_*.hip do what they return.  Plain C++: no HIP header, so ens_plan.hip compiles with any host compiler and
// runs under a host sanitizer.
#pragma once
#include <cstddef>
#include "ens_shared.hpp"

namespace alabi {

// ---- the environment switches.  ens_switches() reads them afresh on every call (tests flip them inside one process) and is the
// only function of the ensemble sampler that reads the environment.  A flag is kept as read: ENS_UNSET when the variable is not
// set, otherwise the first character of its value ('\0' for an empty one); a number is what atoi / atoll make of the value (0 when
// unset: no rule below acts on 0).  The predicates say which characters mean what.
//
// When a switch takes effect:
//   handle creation (alabi_ens_create*)           THREADS, CHUNK, STREAM
//   every alabi_ens_run                           GROUP, GROUP_G16, GRAPH, GRAPH_STEPS, MH, MH_CHUNK, HMC_CHUNK, NUTS_CHUNK, SPIN_LIMIT, MULTI
//   every other entry that launches a half step   MULTI (alabi_ens_half_step*, alabi_ens_step_with_randoms*, the sharded run)
//   once per handle, latched                      PAIR, PLACE: at the first run that considers the pair kernel / the placement,
//                                                 from the switches of that call (alabi_ens::pair_state, ::place_state)
//   every sharded run                             SHARD_GRAPH
// An entry point reads the switches once and hands them down to the launchers, so within one call a switch cannot change
// between two launches.
constexpr int ENS_UNSET = -1;
struct EnsSwitches {
    int stream = ENS_UNSET;       // ALABI_ENS_STREAM: '0' no persistent-kernel buffers on new handles
    int group = ENS_UNSET;        // ALABI_ENS_GROUP: '0' never ens_group_kernel, '1' wherever its blocking is feasible
    int group_g16 = ENS_UNSET;    // ALABI_ENS_GROUP_G16: '1' the 16-member blocking where 8 members would be chosen (tests)
    int graph = ENS_UNSET;        // ALABI_ENS_GRAPH: '0' no graph replay on the launch-per-half-step path
    int mh = ENS_UNSET;           // ALABI_ENS_MH: '0' an all-Gaussian table does not run on ens_mh_kernel
    int multi = ENS_UNSET;        // ALABI_ENS_MULTI: '0' / '1' one proposal per workgroup, '2' / '4' that many
    int pair = ENS_UNSET;         // ALABI_ENS_PAIR: '0' no ens_pair_kernel
    int place = ENS_UNSET;        // ALABI_ENS_PLACE: '0' no placement of the pair kernel's items
    int shard_graph = ENS_UNSET;  // ALABI_ENS_SHARD_GRAPH: '1' graph replay of a full chunk of the sharded run
    int threads = 0;              // ALABI_ENS_THREADS: 64 / 128 / 256 / 512 / 1024 lanes of the half-step workgroup
    int graph_steps = 0;          // ALABI_ENS_GRAPH_STEPS: steps per captured graph, 1 ... chunk_cap
    int spin_limit = 0;           // ALABI_ENS_SPIN_LIMIT > 0: the raw number v (tests: force a time-out).  ens_stream_kernel and
                                  // ens_pair_kernel give up after v polls, ens_group_kernel after v - 1 (1: the first miss)
    long long chunk = 0;          // ALABI_ENS_CHUNK: a shorter chunk, 2 ... (tests of the chunk boundary at few steps)
    long long mh_chunk = 0;       // ALABI_ENS_MH_CHUNK: a shorter ens_mh_kernel launch, 1 ...
    long long hmc_chunk = 0;      // ALABI_ENS_HMC_CHUNK: a shorter ens_hmc_kernel launch, 1 ...
    long long nuts_chunk = 0;     // ALABI_ENS_NUTS_CHUNK: a shorter ens_nuts_kernel launch, 1 ...
};
EnsSwitches ens_switches();

inline bool ens_stream_buffers_off(const EnsSwitches& sw) { return sw.stream == '0'; }
inline bool ens_group_off(const EnsSwitches& sw) { return sw.group == '0'; }
inline bool ens_group_preferred(const EnsSwitches& sw) { return sw.group == '1'; }
inline bool ens_group_force_g16(const EnsSwitches& sw) { return sw.group_g16 == '1'; }
inline bool ens_graph_off(const EnsSwitches& sw) { return sw.graph == '0'; }
inline bool ens_mh_off(const EnsSwitches& sw) { return sw.mh == '0'; }
inline bool ens_pair_off(const EnsSwitches& sw) { return sw.pair == '0'; }
inline bool ens_place_off(const EnsSwitches& sw) { return sw.place == '0'; }
inline bool ens_shard_graph_on(const EnsSwitches& sw) { return sw.shard_graph == '1'; }
// polls of a hand-off word before a persistent kernel gives up and sets the time-out flag
inline int ens_spin_limit_stream(const EnsSwitches& sw) { return sw.spin_limit > 0 ? sw.spin_limit : 1 << 20; }      // ens_stream_kernel, ens_pair_kernel
inline int ens_spin_limit_group(const EnsSwitches& sw) { return sw.spin_limit > 0 ? sw.spin_limit - 1 : 1 << 20; }   // ens_group_kernel (1: the first miss)

// ---- the shape of a handle: everything of alabi_ens the rules below read, projected by ens_shape() (common.hpp)
struct EnsShape {
    int W = 0, E = 1, d = 0, Npad = 0;
    int generic = 0;        // kernel family: 0 squared exponential, 1 the others (the GENERIC instantiations)
    int ymap = 0;           // inverse y scaler inside the kernels (0: none)
    int threads = 0, chunk_cap = 0, stream_grid = 0;     // what ens_create_plan gave the handle
    int has_hist = 0;       // the version history and the time-out flag exist
    int stream_ok = 0, mh_ok = 0;                        // alabi_ens_set_stream
    int has_de = 0;         // the table holds a move that reads more than one partner row, or the whole half
    int all_gauss = 0, all_hmc = 0;
    int factors = 0;        // scale factors of the Gaussian / HMC moves are on the device
    int n_moves = 0;
    int lmax = 1;           // largest leapfrog count of the table (HMC)
    int mh_lds = 0, hmc_lds = 0;                         // dynamic LDS bytes of ens_mh_kernel / ens_hmc_kernel for this table
    int has_stream = 0;     // the call was given a stream (the null stream cannot capture, and is kept off the persistent kernels)
    int all_nuts = 0;       // every move of the table is a NUTS move (kind 7); lmax is then the table's largest max_depth
    int nuts_lds = 0;       // dynamic LDS bytes of ens_nuts_kernel for this table
};
inline int ens_mh_lds_bytes(int n_moves, int d) { return n_moves * d * d * (int)sizeof(double); }
inline size_t ens_hmc_lds_bytes(int n_moves, int d, int Npad) { return ((size_t)n_moves * d * (d | 1) + (size_t)Npad) * sizeof(double); }
// ens_nuts_kernel: the same plus the U-turn checkpoints of a subtree, [2][ALABI_NUTS_MAX_DEPTH][64] doubles
inline size_t ens_nuts_lds_bytes(int n_moves, int d, int Npad) {
    return ens_hmc_lds_bytes(n_moves, d, Npad) + (size_t)2 * ALABI_NUTS_MAX_DEPTH * 64 * sizeof(double);
}

// ---- creation: workgroup size of the half-step kernels, steps the draw buffers hold, workgroups per ensemble of the persistent
// kernel (0: no persistent-kernel buffers -- more ensembles than CUs, or ALABI_ENS_STREAM=0)
struct EnsCreatePlan {
    int threads, chunk_cap, stream_grid;
};
EnsCreatePlan ens_create_plan(int W, int E, int Npad, int n_cu, const EnsSwitches& sw);

// Point pairs per compute lane of the persistent kernels for this handle, 0: they do not fit (ens_stream_max_db).
int ens_stream_ppt(const EnsShape& sh);

// ---- group kernel: the blocking for an ensemble
struct GroupPlan {
    int ok, KS, Q, QP, G, NG, RT, tpm, ltw;
    size_t lds_bytes;
};
GroupPlan ens_group_plan(const EnsShape& sh, int n_cu, const EnsSwitches& sw);

// Steps per launch of ens_mh_kernel / ens_hmc_kernel / ens_nuts_kernel, 0: the table does not run on that kernel
int ens_mh_chunk(const EnsShape& sh, int n_cu, const EnsSwitches& sw);
int ens_hmc_chunk(const EnsShape& sh, int n_cu, const EnsSwitches& sw);
int ens_nuts_chunk(const EnsShape& sh, int n_cu, const EnsSwitches& sw);

// Proposals per workgroup (1, 2, 4) of a half-step launch of `total` proposals over all ensembles; hist_mode: the sharded
// run's history mode, always 1
int ens_half_np(int threads, int d, long long total, bool hist_mode, int n_cu, const EnsSwitches& sw);

// ---- the route of alabi_ens_run
//   path 0  one launch per half step (graph: replay of a captured chunk of graph_steps steps where the call has at least two)
//        1  persistent kernel: ens_stream_kernel, or ens_pair_kernel where `pair` holds and the launcher could allocate
//        3  ens_group_kernel
//        4  ens_mh_kernel, `chunk` steps per launch        5  ens_hmc_kernel, `chunk` steps per launch
//        6  ens_nuts_kernel, `chunk` transitions per launch
//       -1  refused (ALABI_BAD_ARGUMENT): an HMC or NUTS table that does not fit, or a red-blue table on one walker
// The plan says what is wanted; a launcher that allocates says whether it could be had.  The group kernel's hand-off buffers
// (ens_group_buffers): when they cannot be had the caller asks again with group_allowed = false.  The pair kernel's proposals
// (ens_pair_ready) and the placement counters (ens_place_ready): `pair` and `place` are the rules alone, each latched by its
// launcher at the first call that asks, so a later call's switches no longer move them.  The second draw-buffer set and the
// side stream (ens_draw_ahead_ready) are no route: the persistent run draws ahead where they exist.
struct EnsRoute {
    int path;
    int chunk;          // paths 4, 5, 6
    bool pair, place;   // path 1
    bool graph;         // path 0
    int graph_steps;
};
EnsRoute ens_route(const EnsShape& sh, int n_cu, const EnsSwitches& sw, bool group_allowed = true);

}  // namespace alabi
