// dag_task.hpp -- the records and constants of a task list: what the host planner (dag_plan.hpp) writes and the persistent
// kernel (dag_kernel.hpp) reads.  Plain C++17, no HIP header.
#pragma once

// The following scheme (scheme 2: strip solves that follow the factorisation step by step, dag_pss / dag_special) is part
// of the build unless -DPSOAP_NO_FOLLOW is given (the build's fallback rung and the variant matrix of DESIGN.md 3.4 use
// the older structure, in which the fused diagonal task is the only out-of-line routine).
#if !defined(PSOAP_NO_FOLLOW) && !defined(PSOAP_FOLLOW)
#define PSOAP_FOLLOW 1
#endif

namespace psoap {

constexpr int DAG_QUEUES = 8;   // one ticket queue per XCD (MI355X: 8 XCDs, each with its own 4 MiB L2)

// queue g holds tasks[first[g] .. first[g+1]) in ticket order (kernel argument, by value)
struct DagQueues {
    unsigned int first[DAG_QUEUES + 1];
    unsigned int follow_first;      // scheme 2: the first block row whose strip solves follow (0, or 2: PSOAP_FOLLOW_ROW0=0)
};

// Scheme 0 (the kernels without the latency paths, LAT = false; round 4): updates wait for the TILES they read -- the
// per-column progress words MatFlags::rvrow -- instead of whole block rows (dag_update).  Compile-time: a run-time switch
// around a one-lane poll is the code shape on which hipcc parks values under the poll's exec mask (the
// build's assembly scan caught exactly that in the first version), so the choice is the kernel form's: LAT = false.

// One entry of the host-built task list (dag_build_tasks); the ticket is the index.
//   PART : partial left-looking update of tile (q, j) over finished block rows [pa, pb); the
//          128 x 128 partial sum goes to workspace slot `slot`, then arrive[ctr] += 1.
//   DIAG / OFF : the final part [pa, pb) of the update, plus the S-1 partials of slots
//          slot .. slot+S-2 (added in slot order once arrive[ctr] == S-1), then the tile's
//          factorisation (DIAG) or strip solve (OFF).
// Splitting along K serves two purposes: the diagonal tile of block row q+1 is pre-accumulated
// over rows < q while block row q is still in flight (its final part is one panel long, so the
// critical chain per block row is 128-row update -> in-block Cholesky), and the last block rows,
// which have too few tiles to occupy the persistent grid, are cut into up to 8 parts per tile.
// Latency scheme only -- the row-to-row critical path potrf(q) -> strip solve of (q, q+1) -> update of
// (q+1, q+1) -> potrf(q+1) is kept inside the DIAG tasks, one cross-workgroup hand-off per block row:
//   DAG_FUSED    (DIAG)  after the in-block Cholesky the same workgroup solves tile (q, q+1) and publishes
//                        next_done = q + 1;
//   DAG_WAITNEXT (DIAG)  the final part [q-1, q) waits for next_done >= q instead of the whole block row;
//   DAG_NOSOLVE  (OFF)   tile (q, q+1): update only, publishes off1_ready = q + 1 (the DIAG task solves it).
//   DAG_SCHUR    (predict) final of a tile of the Schur complement  A - W^T W  = Sigma: rows AND columns lie in the
//                        appended range (q, j >= P), update over all P block rows, then the tile -- with the prior
//                        covariance A evaluated on the fly like K -- is stored into DagAug::S and mirrored; no solve.
enum : unsigned char { DAG_PART = 0, DAG_DIAG = 1, DAG_OFF = 2, DAG_SCHUR = 3, DAG_TYPE_MASK = 0x0F, DAG_CHAIN = 0x10,
                       DAG_NOSOLVE = 0x20, DAG_WAITNEXT = 0x40, DAG_FUSED = 0x80 };
struct DagTask {
    unsigned char type, q, j, S;
    unsigned short b;
    unsigned char pa, pb;
    unsigned int slot;
    unsigned int ctr;
};
static_assert(sizeof(DagTask) == 16, "DagTask is 16 bytes");
constexpr unsigned int DAG_CTR_MASK = 0x00ffffffu;   // DagTask::ctr of a final: bits 24.. belong to the skyline (dag_build_tasks)

constexpr unsigned short STREAM_BURST_END = 0x8000;   // DagTask::b of a lane's task list (the matrix index is the lane):
                                                      // the last ticket of a burst -- the next one starts a block row
constexpr int STREAM_MAX_LANES = 64;       // lanes of a stream, at most (StreamDev, dag_kernel.hpp)
constexpr int STREAM_NOMINAL_LANES = 32;   // the lane count every lane plan's split factors are cut for (dag_build_lane_plan)

}  // namespace psoap
