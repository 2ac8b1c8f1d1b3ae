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
// Ready-only hand-out of the PART tasks (round 5, the review's item 4, asked for since round 3) -- BUILT, MEASURED, NOT
// SHIPPED: compiled in with -DPSOAP_POOL only (tools/build_variant.py pool -DPSOAP_POOL).  The premise was round 3's reading of
// tools/wg_occupancy.py: "80-130 of the 256 workgroups of a single N = 6000 evaluation hold PARTs that wait".  That column
// counts a part from its start to the stamp behind its LAST panel's wait -- the look-ahead K-loop over its older panels
// included.  The stamps that add up the waits themselves (tools/part_wait_share.py, profiles/r5_pool_*.txt) say: in list
// order the parts spend 6.9 % of the time they hold a workgroup waiting for block rows and 5.6 % for their predecessor's
// tile at N = 6000 (2.7 / 2.1 % at N = 8192, 2.9 / 2.4 % for eight matrices) -- at most 8 % of the launch's capacity, on
// a launch whose length is the row-to-row chain's.  Handed out ready-only (three iterations: compare-exchange per final,
// chains overlapping again, fetch-add with held tickets; windows of 128 ... 4096 parts; just-in-time leads 0 ... 16) the
// waits for rows drop to 1.2 % and the finals pay for it: they are drawn later, hold their workgroups for 186 ms in all
// instead of 121 (eight matrices: 4.92 s instead of 3.37) and the row-to-row period grows from 55 to 70 us -- a single
// N = 6000 evaluation takes 3.25 ms against 2.57, eight take 15.0 against 10.9, N = 8192 5.85 against 4.82, predict 11.7
// against 10.5.  The list order with its just-in-time parts IS the better scheduler here; what bounds the single evaluation
// is the chain.
// How it works, for the record.  With ONE in-order ticket list a workgroup that draws a PART whose panels or predecessor are
// not there yet holds it and waits, while ready PARTs further down the list wait for a workgroup.  The list is handed out
// in two parts per queue:
//   main  the finals (DIAG / OFF / SCHUR), in the list's order, from a ticket counter as before -- but a final with a chain
//         is only handed out once the chain's LAST part has been taken (so whoever holds a final waits for running work only);
//   pool  the PARTs, in the list's order, each with a `taken` bit: a workgroup that finds no final to take scans a window
//         of the pool from its first untaken entry and takes a part that is READY -- its panels' block rows complete
//         (rows_done >= pb) and its predecessor in the chain TAKEN (it adds the predecessor's running sum at the end of
//         its own update, so the parts of a chain overlap as they do in list order).
// Every wait still targets a task somebody is running: finals wait for finals with smaller main tickets (all handed out)
// and for their chain (all taken); parts wait for nothing.  And something can always be taken: when nothing runs, either
// the head final's chain is taken (it can be handed out) or the pool's first untaken part is ready (its predecessors are
// done, the rows it reads belong to finals ahead of the head) -- tests/test_dag_plan.py plays it through.
// order[first[g] .. first[g+1]) of queue g: n_main[g] task ids of finals, then the ids of its PARTs; dep[] (main entries):
// position in order[] of the last part of the final's chain, DAG_POOL_NONE without one.
constexpr unsigned int DAG_POOL_NONE = 0xffffffffu;
struct DagPool {
    const unsigned int* order;      // nullptr: the launch hands its tasks out in list order (schemes 0, streams)
    const unsigned int* dep;
    unsigned int* taken;            // one BIT per entry of order[] (bit p & 31 of word p >> 5), zeroed per launch
    unsigned int n_main[DAG_QUEUES];
};

// Scheme 0 (the kernels without the latency paths, LAT = false; round 4): updates wait for the TILES they read -- the
// per-column progress words MatFlags::rvrow -- instead of whole block rows (dag_update).  Compile-time: a run-time switch
// around a one-lane poll is the code shape on which hipcc parks values under the poll's exec mask (the
// build's assembly scan caught exactly that in the first version).  -DPSOAP_NO_TILE_DEPS: whole rows as in rounds 1-3 (A/B).
#ifdef PSOAP_NO_TILE_DEPS
constexpr bool DAG_TILE_DEPS = false;
#else
constexpr bool DAG_TILE_DEPS = true;
#endif

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
