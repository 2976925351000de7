// What the host and the device side of the task-queue Cholesky share: the task record, the per-matrix record of the batched queue,
// the size thresholds, and the environment switches of the whole factorisation (read in ONE place, chol_tasklist.hip).
// Plain C++: no HIP header, so the host-only combinatorics (chol_tasklist.hip) compile with any host compiler.
#pragma once
#include <vector>

namespace alabi {

// One task of the queue (chol_queue.hpp has the protocol, chol_tasklist.hip the order).
// type & 255: 0 CHAIN(k), 1 TRSM(i,k), 2 UPDATE(i,j,k..k+cnt-1) with cnt = type >> 8 consecutive block columns (chol_build_tasks),
//             4 UPDATE2 = UPDATE(i,j,..) and UPDATE(i+1,j,..) in one task (eight-wave kernel), 5 UPDATE4 = the 2 x 2 block of tiles
//             (i,j), (i+1,j), (i,j+1), (i+1,j+1), i >= j + 1
// Batched queue (chol_tasks8_batch_kernel): bits 16.. of `type` say which matrix of the batch the task belongs to; the matrices are
// independent, each with its own tile versions, slab counters, status word and reciprocal diagonal.
struct CholTask { int type, i, j, k; };
struct CholMat { double* A; double* dinv; double* linv; int* ver; int* sver; int* info; int ld, nb; };
#define ALABI_CHOL_TASKS_MAX_NB 256   // default upper end of the one-launch task queue (N <= 16384); beyond: panels of 8 block columns
#define ALABI_CHOL_W8_MIN_NB 3    // block columns from which the queue runs eight waves per workgroup (chol_tasks8_kernel): every size it takes
#define ALABI_CHOL_UPDATE4_MIN_NB 100 // block columns from which the far updates take 2 x 2 tiles per task (UPDATE4; below: UPDATE2)
#define ALABI_CHOL_PLAIN_MIN 4   // block columns per UPDATE from which its operands are read with ordinary loads behind one acquire

// ---- the environment switches of the factorisation.  chol_switches() reads them afresh on every call (tests flip them inside one
// process) and is the only function of the Cholesky that reads the environment.
// A flag is kept as read: CHOL_UNSET when the variable is not set, otherwise the first character of its value ('\0' for an empty
// one); the predicates below say which characters mean what.  A number is kept when it lies in its accepted range; otherwise the
// field holds the default, or 0 / CHOL_UNSET where the default depends on the size of the matrix.
constexpr int CHOL_UNSET = -1;

// The switches that shape a task list.  A cached list is valid for exactly the CholListShape it was built with: compare with ==.
struct CholListShape {
    int gk = 0;                     // ALABI_CHOL_GK 1..64: block columns per far update (0: by size, chol_task_shape)
    int near = 0;                   // ALABI_CHOL_NEAR 1..16: width of the near band (0: by size)
    int w8 = CHOL_UNSET;            // ALABI_CHOL_W8: '1' eight waves per workgroup, anything else four; unset: by size
    int update2 = CHOL_UNSET;       // ALABI_CHOL_UPDATE2: '0' no two-tile tasks
    int update4 = CHOL_UNSET;       // ALABI_CHOL_UPDATE4: read differently by the two lists (chol_four_single, chol_four_batch)
    int batch_gk = 10;              // ALABI_BATCH_GK 1..255: block columns per group of a batched matrix's list
    int batch_left = CHOL_UNSET;    // ALABI_BATCH_LEFT: '0' the single-matrix list inside a batch
    int batch_phases = CHOL_UNSET;  // ALABI_BATCH_PHASES: '0' matrix by matrix, '3' without the split of the updates
    bool operator==(const CholListShape& o) const {
        return gk == o.gk && near == o.near && w8 == o.w8 && update2 == o.update2 && update4 == o.update4 && batch_gk == o.batch_gk &&
               batch_left == o.batch_left && batch_phases == o.batch_phases;
    }
};
struct CholSwitches {
    CholListShape list;
    int tasks = CHOL_UNSET;         // ALABI_CHOL_TASKS: '1' forces the queue, '0' forces it off
    int spin_limit = 1 << 18;       // ALABI_CHOL_SPIN_LIMIT > 0: polls before a wait of the queue gives up (tests: force a time-out)
    int panel = CHOL_UNSET;         // ALABI_CHOL_PANEL 0 / 2 / 4 / 6 / 8: block columns per panel of the launch-per-step path (unset: by size)
    int lookahead = CHOL_UNSET;     // ALABI_CHOL_LOOKAHEAD: '0' no second stream behind a panel
    bool log_print = false;         // ALABI_CHOL_LOG_PRINT set: an ALABI_CHOL_LOG build prints the chain's event log
    int batch_lists = 8;            // ALABI_BATCH_LISTS 1..8
    int batch_window = 8;           // ALABI_BATCH_WINDOW 0..4096
};
CholSwitches chol_switches();

inline bool chol_queue_forced_on(const CholSwitches& sw) { return sw.tasks == '1'; }
inline bool chol_queue_forced_off(const CholSwitches& sw) { return sw.tasks == '0'; }
inline bool chol_lookahead(const CholSwitches& sw) { return sw.lookahead != '0'; }
inline bool chol_batch_left(const CholListShape& sh) { return sh.batch_left != '0'; }
// ALABI_CHOL_UPDATE4, the single matrix's list: '1' = on, anything else set = off, unset = from ALABI_CHOL_UPDATE4_MIN_NB block columns on
inline bool chol_four_single(const CholListShape& sh, int nb) { return sh.update4 == CHOL_UNSET ? nb >= ALABI_CHOL_UPDATE4_MIN_NB : sh.update4 == '1'; }
// ... and a batched matrix's list: on unless '0'
inline bool chol_four_batch(const CholListShape& sh) { return sh.update4 != '0'; }

// ---- chol_tasklist.hip: the lists (pure host combinatorics)
bool chol_tasks_w8(int nb, const CholListShape& sh);                                  // eight waves per workgroup (chol_tasks8_kernel)?
void chol_single_tasks(int nb, const CholListShape& sh, std::vector<CholTask>& t);    // the list of one matrix on its own
int chol_batch_build(const std::vector<int>& nbs, int nlists, int window, const CholListShape& sh, std::vector<CholTask>& out,
                     std::vector<int>& list_off);                                     // the interleaved lists of a batch

}  // namespace alabi
