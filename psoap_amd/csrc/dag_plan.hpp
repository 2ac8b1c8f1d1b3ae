// dag_plan.hpp -- the host scheduler of the persistent Cholesky kernel (k_chol_dag, dag_kernel.hpp): the task lists,
// the scheme and worker rules, and the plan rule of a likelihood launch.  Plain C++17 over std::vector: no
// HIP type, so it is compiled, run and sanitized by a host compiler alone (tests/host/plan_host_check.cpp).
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "tile_consts.hpp"
#include "dag_task.hpp"

namespace psoap {

// ---------------------------------------------------------------------------------------------
// Host: build the task lists (one queue per XCD, matrix b in queue b mod 8) for a batch of B
// matrices of P block rows on `workers` persistent workgroups.  Ticket order inside a queue
// (every wait targets a smaller ticket of the same queue):
//   for each block row q:  DIAG finals of row q (the queue's matrices)
//                          PARTs that pre-accumulate the diagonal tile of row q+1 over rows < q
//                          PARTs + OFF finals of row q (b-major, then j; inside a skyline j-major, then b: below)
// ---------------------------------------------------------------------------------------------
struct DagPlan {
    std::vector<DagTask> tasks;
    DagQueues queues{};
    unsigned int n_slots = 0;
    unsigned int n_ctrs = 0;
    int scheme = 0;            // 0 throughput, 1 latency: selects the kernel instantiation (k_chol_dag<.., LAT>)
};

inline int dag_split_factor(int tasks_in_row, int q, int workers, int scheme, bool augmented = false)
{
    // cut tiles of sparse block rows until the row offers about `workers` tasks (at most 8 parts).
    // Throughput scheme: full occupancy, parts at least two panels long.  Latency scheme: half the workers,
    // parts at least four panels long -- every part costs a round trip of its 128 KB partial tile through the
    // workspace and a dependency hand-off, and the workers that are not on a matrix's critical path have
    // slack (measured, tools/split_sweep.sh: N = 2000, B = 32: 3.0 -> 2.5 ms; N = 6000, B = 4: 7.7 -> 7.1 ms;
    // single evaluations unchanged; a quarter of the workers is too few from N = 6000, B = 8 on).
    // PSOAP_DAG_SPLIT_PCT / PSOAP_DAG_SPLIT_MIN override both numbers (experiments).
    static const int env_pct = getenv("PSOAP_DAG_SPLIT_PCT") ? atoi(getenv("PSOAP_DAG_SPLIT_PCT")) : 0;
    static const int env_min = getenv("PSOAP_DAG_SPLIT_MIN") ? atoi(getenv("PSOAP_DAG_SPLIT_MIN")) : 0;
    // (scheme 2: 35 % -- with the PARTs handed out just in time the chains run ahead of the finals anyway, and every part
    // less is a partial-tile hand-over less; measured over N = 4096 .. 8192, B = 1 .. 8: 25 / 35 / 50 / 70 %)
    // (predict -- appended columns: the launch is bound by throughput, not by its chain: 494 of 512 workgroups busy, 88 % of
    // their time in PART tasks (tools/predict_timeline.py), and every part less is a 128 KB partial tile that does not
    // travel: 25 % measured 9.85-10.0 ms against 10.25-10.3 at 35 %, profiles/r5_experiments.txt)
    const int pct = env_pct > 0 ? env_pct : (scheme == 2 ? (augmented ? 25 : 35) : (scheme >= 1 ? 50 : 100));
    const int minp = env_min > 0 ? env_min : (scheme >= 1 ? 4 : 2);
    int S = 1;
    while (S < 8 && tasks_in_row * S * 100 < workers * pct && minp * S <= q) S *= 2;
    return S;
}

// Tasks of one tile whose update over panels [pa_first, pb_last) is cut into pieces.
//   scheme 0 (throughput): nsplit equal ranges; the first nsplit-1 are PARTs, the final takes the last
//     range and GATHERS the nsplit-1 partial tiles.  Least work per tile; right when other matrices of
//     the queue hide the wait for the block row above.
//   scheme 1 (latency): nsplit PARTs over equal ranges of [pa_first, pb_last - 1) plus a final that
//     covers the LAST panel only -- the one piece that has to wait for the block row above, kept as
//     short as the dependency allows (the PARTs wait for older rows and run ahead).  The partial sums
//     are CHAINED: PART s adds the tile PART s-1 left in the previous slot to its own, so every task
//     reads one partial tile.  Right when a queue holds one matrix and the row-to-row chain is the
//     critical path.
// Encoding: PART.S = index in the chain (0 when gathered), PART.slot = its output (gathered:
// consecutive slots; chained: an even/odd pair used alternately); final.S = number of pieces,
// final.slot = first slot to read (gather: the first PART's, chain: the last PART's).  nsplit == 1: one final over the whole range.
inline int dag_final_panels()
{
    const char* e = getenv("PSOAP_FINAL_PANELS");      // experiments
    return e ? atoi(e) : 2;
}
inline int dag_jit_rows()
{
    const char* e = getenv("PSOAP_DAG_JIT");      // experiments; 0: readiness order
    return e ? atoi(e) : 6;
}
inline int dag_follow_first_row()
{
    const char* e = getenv("PSOAP_FOLLOW_ROW0");      // experiments; 0: rows 0 and 1 keep the forms of scheme 1
    return (e && e[0] == '0') ? 2 : 0;
}
inline bool dag_xfollow_enabled()
{
    const char* e = getenv("PSOAP_XFOLLOW");
    return !(e && e[0] == '0');
}
// final_panels: how many of the last panels a chain's final takes itself (1: only the one that depends on the block row
// above; 2 -- following strip solves: the chain's last PART then needs the row before that only and is folded in a whole
// row period before the final gets its last operands -- the hand-over of a partial tile costs 30-40 us)
inline void dag_emit(DagPlan& plan, int type, int b, int q, int j, int pa_first, int pb_last, int nsplit, int scheme,
                     unsigned char final_flags = 0, int final_panels = 1)
{
    if (final_panels > 1) {
        const int left = pb_last - final_panels - pa_first;         // panels for the PARTs
        if (left <= 0) nsplit = 1;
        else if (nsplit > left) nsplit = left;
        if (scheme < 1 || nsplit <= 1) final_panels = 1;            // (only a chain's final has a fixed range)
    }
    const bool chain = (scheme >= 1) && nsplit > 1;
    const int nparts = chain ? nsplit : nsplit - 1;                 // PART tasks
    const unsigned int ctr = (nparts > 0) ? plan.n_ctrs++ : 0u;
    if (chain) plan.n_slots += plan.n_slots & 1u;                   // a chain ping-pongs between an even/odd slot pair
    const unsigned int slot0 = plan.n_slots;
    const int pb_parts = chain ? pb_last - final_panels : pb_last;
    const int span = pb_parts - pa_first;
    const unsigned char flag = chain ? DAG_CHAIN : 0;
    for (int sidx = 0; sidx < nparts; ++sidx) {
        DagTask t{};
        t.type = DAG_PART | flag;
        t.b = (unsigned short)b;
        t.q = (unsigned char)q;
        t.j = (unsigned char)j;
        t.S = (unsigned char)(chain ? sidx : 0);
        t.pa = (unsigned char)(pa_first + (long long)span * sidx / nsplit);
        t.pb = (unsigned char)(pa_first + (long long)span * (sidx + 1) / nsplit);
        // gathered: one slot per PART; chained: PART s reads slot0 + ((s - 1) & 1) and writes slot0 + (s & 1)
        // (its predecessor's reader -- itself -- is the only one, so two slots per tile are enough)
        t.slot = chain ? slot0 + (unsigned int)(sidx & 1) : plan.n_slots++;
        t.ctr = ctr;
        plan.tasks.push_back(t);
    }
    if (chain) plan.n_slots = slot0 + 2;
    DagTask t{};
    t.type = (unsigned char)type | flag | final_flags;
    t.b = (unsigned short)b;
    t.q = (unsigned char)q;
    t.j = (unsigned char)j;
    t.S = (unsigned char)(nparts + 1);
    t.pa = (unsigned char)(chain ? pb_last - final_panels : pa_first + (long long)span * (nsplit - 1) / nsplit);
    t.pb = (unsigned char)pb_last;
    t.slot = (nparts > 0) ? (chain ? slot0 + (unsigned int)((nparts - 1) & 1) : slot0) : 0u;
    t.ctr = ctr;
    plan.tasks.push_back(t);
}

// task list of ONE queue: the matrices in `mats`, served by about `workers` workgroups
// `Bq_nominal` (the largest queue's matrix count) decides the split factors, so every matrix of the
// batch gets the same task structure and identical proposals give identical bits in any batch slot
// Tasks of the Schur complement of the appended columns (predict: Sigma = A - W^T W), Ms x Ms tiles, upper triangle:
// tile (P + i, P + j) is a left-looking update over ALL P block rows with nothing to solve afterwards -- work that
// needs no critical path, cut into chained parts of `len` panels whose boundaries are staggered from tile to tile, so
// that about the same number of parts becomes ready with every finished block row and the workgroups that wait on the
// factorisation's row-to-row chain always find one.  The final covers the last panel and stores into DagAug::S.
inline void dag_emit_schur(DagPlan& plan, int b, int P, int Ms, int len = 8)
{
    static const int env_len = getenv("PSOAP_SCHUR_LEN") ? atoi(getenv("PSOAP_SCHUR_LEN")) : 0;   // experiments
    if (env_len > 0) len = env_len;
    int tile = 0;
    for (int i = 0; i < Ms; ++i)
        for (int j = i; j < Ms; ++j, ++tile) {
            std::vector<int> cuts;                           // part boundaries in [0, P - 1]
            cuts.push_back(0);
            for (int c = 1 + tile % len; c < P - 1; c += len) cuts.push_back(c);
            if (P - 1 > cuts.back()) cuts.push_back(P - 1);
            const int nparts = (int)cuts.size() - 1;         // PARTs cover [0, P - 1); may be 0 when P == 1
            const unsigned int ctr = plan.n_ctrs++;
            plan.n_slots += plan.n_slots & 1u;
            const unsigned int slot0 = plan.n_slots;
            for (int sidx = 0; sidx < nparts; ++sidx) {
                DagTask t{};
                t.type = DAG_PART | DAG_CHAIN;
                t.b = (unsigned short)b;
                t.q = (unsigned char)(P + i);
                t.j = (unsigned char)(P + j);
                t.S = (unsigned char)sidx;
                t.pa = (unsigned char)cuts[sidx];
                t.pb = (unsigned char)cuts[sidx + 1];
                t.slot = slot0 + (unsigned int)(sidx & 1);
                t.ctr = ctr;
                plan.tasks.push_back(t);
            }
            plan.n_slots = slot0 + (nparts > 1 ? 2 : (nparts > 0 ? 1 : 0));
            DagTask fin{};
            fin.type = DAG_SCHUR | DAG_CHAIN;
            fin.b = (unsigned short)b;
            fin.q = (unsigned char)(P + i);
            fin.j = (unsigned char)(P + j);
            fin.S = (unsigned char)(nparts + 1);
            fin.pa = (unsigned char)(P - 1);
            fin.pb = (unsigned char)P;
            fin.slot = nparts > 0 ? slot0 + (unsigned int)((nparts - 1) & 1) : 0u;
            fin.ctr = ctr;
            plan.tasks.push_back(fin);
        }
}

// PSOAP_FIXED_PLAN=1 (round 4): every matrix gets the task structure of a stream lane (dag_build_lane_plan: scheme 0, the
// split factors of ONE matrix on the nominal share of the workgroups) whatever the batch -- so the order of summation
// inside a matrix, and with it every bit of its lnprob, is the same for every batch size, for every number of chunks in
// a launch, for every number of GPUs, and equal to what a stream returns.  What it costs: small batches lose the
// latency schemes (a single N = 6000 evaluation: 11 ms instead of 2.6).  For runs that have to be reproducible across
// world sizes (an MH chain decided in the last bits: the reference's np.sum over chunks is deterministic,
// psoap/sample_parallel.py:387).
inline bool dag_fixed_plan()
{
    const char* e = getenv("PSOAP_FIXED_PLAN");
    return e && e[0] == '1';
}
inline int dag_nominal_share(int workers_total) { const int s = workers_total / STREAM_NOMINAL_LANES / 2; return s > 0 ? s : 1; }

// ---- skyline-aware list rules (scheme 0 inside a skyline; profiles/sky_sched.md, profiles/sky_split_ab.md) ----------------
// The split and order rules above were measured on dense lists, where a block row offers P - q tiles of q panels each.
// Inside a skyline a row is a band of tiles whose updates run over q - first[j] panels, and the rules look at that work:
//   order    the tiles of a block row column by column over the queue's matrices (j-major), not matrix after matrix: tile
//            (q, q+1), whose strip solve continues into the diagonal task of block q+1, comes up first for EVERY matrix
//            of the queue and not behind all tiles of the matrices in front of it; within a matrix the order stays j
//            ascending, which inside a skyline is longest update first (first is non-decreasing);
//   history  the pre-accumulation of diagonal tile q+1 is cut by its clipped span q - first[q+1] into parts of at
//            least DAG_SKY_PRE_LEN panels (at most 8 parts), not by "a quarter of the workers".
// The off-diagonal tiles keep the dense split rule (dag_split_factor on the row's tile count): cutting them by the row's
// work in panels instead was tried and stayed inside the run-to-run spread (profiles/sky_split_ab.md).
// The list stays a function of (B, P, scheme, first).  PSOAP_SKY_SPLIT=0 (read at handle creation, and by
// psoap_dag_plan_sky when it is called): the dense rules inside the skyline, the list as it was.
inline bool dag_sky_split_env()
{
    const char* e = getenv("PSOAP_SKY_SPLIT");
    return !(e && e[0] == '0');
}
constexpr int DAG_SKY_PRE_LEN = 6;
// PARTs of a pre-accumulation over `span` panels: pieces of at least DAG_SKY_PRE_LEN, at most 8
inline int dag_sky_pre_parts(int span)
{
    const int n = span / DAG_SKY_PRE_LEN;
    return n < 1 ? 1 : (n > 8 ? 8 : n);
}

// tiles of block row q inside the skyline `first` of a matrix of P block rows (the diagonal tile included)
inline int dag_sky_row_tiles(const int* first, int P, int q)
{
    int n = 0;
    for (int j = q; j < P && first[j] <= q; ++j) ++n;
    return n;
}
// `first` (scheme 0, uniform batches without appended columns; nullptr: dense): the skyline -- tile (q, j) exists iff
// q >= first[j], first non-decreasing with first[j] <= max(j - 1, 0); the update of an existing tile runs over the block rows
// [first[j], q) and is cut into equal ranges of that.  All zero: the dense list, byte for byte.
inline void dag_build_queue(DagPlan& plan, const std::vector<int>& mats, const std::vector<int>& Ps, int workers,
                            int Bq_nominal, int scheme, int Mt = 0, int Ms = 0, int fixed_share = 0, const int* first = nullptr,
                            bool sky_split = false)
{
    // Ps[b]: block rows of matrix b.  A heterogeneous batch (matrices of several chunks) walks the block
    // rows of all its matrices together; a matrix simply drops out once its rows are used up.
    if (mats.empty()) return;
    int P = 0;
    bool uniform = true;
    for (int b : mats) {
        P = Ps[b] > P ? Ps[b] : P;
        uniform = uniform && Ps[b] == Ps[mats[0]];
    }
    std::vector<std::vector<DagTask>> early_final(P);   // DIAG finals whose PARTs were emitted a row early
    // scheme 0 (round 4): the final of DIAG(q+1) sits right BEHIND the final of tile (q, q+1) and is run by the workgroup
    // that ran that one (DAG_FUSED on the OFF final: "continue with the next record"; DAG_NOSOLVE on the DIAG final:
    // "owned", skipped by whoever draws its ticket) -- see k_chol_dag
    const bool cont0 = (scheme == 0);
    std::vector<DagTask> owned_final(Ps.size());          // per matrix: the DIAG(q+1) final to emit behind tile (q, q+1)
    std::vector<char> has_owned(Ps.size(), 0);
    auto fj = [first](int j) { return first ? first[j] : 0; };
    // (the skyline-aware rules, above)
    const bool sky = first && sky_split;
    for (int q = 0; q < P; ++q) {
        // tiles of this block row in the queue; uniform batches use the nominal matrix count so that the
        // split factors do not depend on the slot a matrix sits in
        long long row_tiles = 0;
        int live = 0;
        for (int b : mats)
            if (q < Ps[b]) {
                row_tiles += Ps[b] + Mt - q;
                ++live;
            }
        if (uniform) {
            row_tiles = (long long)Bq_nominal * (P + Mt - q);
            live = Bq_nominal;
        }
        if (first) row_tiles = (long long)Bq_nominal * dag_sky_row_tiles(first, P, q);
        const int Bq = live;
        // (fixed_share > 0: per matrix, from its own size only)
        // (span: the block rows the tile's update runs over -- q, or q - first[j] inside a skyline)
        auto s_off = [&](int b, int span) {
            return fixed_share > 0 ? dag_split_factor(Ps[b] + Mt - q, q, fixed_share, scheme)
                                   : dag_split_factor((int)row_tiles, span, workers, scheme, Mt > 0);
        };
        // latency scheme: DIAG(q) also solves the tile right of the diagonal (DAG_FUSED) whenever a next
        // diagonal tile exists, and DIAG(q >= 1) waits only for that tile of the row above (DAG_WAITNEXT)
        // scheme 2 ("following"): from block row 2 on -- where the diagonal task is the fused fast one, which publishes its
        // block rows step by step -- the strip solves FOLLOW the factorisation (dag_pss: DAG_WAITNEXT on an OFF task),
        // the diagonal task solves nothing itself, and the strip solve of tile (q, q+1) publishes next_done (DAG_NOSOLVE
        // on a following OFF task).  Rows 0 and 1 keep the forms of scheme 1.
        // (dag_follow_first_row(): 0 -- the first block rows follow as well: their diagonal tasks then need a running sum to
        // start from, which a PART with an empty range provides, it "carries K"; 2: rows 0 and 1 in the forms of scheme 1)
        const int q_f = dag_follow_first_row();
        const bool following = (scheme == 2) && q >= q_f;
        // (block row r: its solved tiles are delivered row block by row block (DAG_FUSED on a following OFF task) to the
        // tasks of block row r+1 that read them -- the diagonal task of block r+1 (DAG_NOSOLVE on a DIAG task) and the
        // last panel of the strip solves' updates; PSOAP_XFOLLOW=0 keeps the first level only -- A/B measurements)
        auto xlink = [&](int r) { return scheme == 2 && r >= q_f && dag_xfollow_enabled(); };
        auto fused = [&](int b) { return scheme >= 1 && !following && q + 1 < Ps[b]; };
        // 1. DIAG finals of this row
        if (q <= 1 && following) {
            // the fused fast diagonal task (the one that publishes its steps) for the first block rows too: a chain of
            // one PART over no panels -- the covariance tile -- and the final over [0, q)
            for (int b : mats) {
                if (q >= Ps[b]) continue;
                const unsigned int ctr = plan.n_ctrs++;
                plan.n_slots += plan.n_slots & 1u;
                const unsigned int slot0 = plan.n_slots;
                plan.n_slots = slot0 + 1;
                DagTask t{};
                t.type = DAG_PART | DAG_CHAIN;
                t.b = (unsigned short)b;
                t.q = t.j = (unsigned char)q;
                t.S = 0;
                t.pa = t.pb = 0;
                t.slot = slot0;
                t.ctr = ctr;
                plan.tasks.push_back(t);
                DagTask fin{};
                fin.type = DAG_DIAG | DAG_CHAIN | DAG_WAITNEXT | ((q == 1 && xlink(0)) ? DAG_NOSOLVE : 0);
                fin.b = (unsigned short)b;
                fin.q = fin.j = (unsigned char)q;
                fin.S = 2;
                fin.pa = 0;
                fin.pb = (unsigned char)q;
                fin.slot = slot0;
                fin.ctr = ctr;
                plan.tasks.push_back(fin);
            }
        } else if (q <= 1) {
            for (int b : mats)
                if (q < Ps[b]) {
                    if (cont0 && q == 1) {
                        // DIAG(1): one final over [0, 1), emitted behind tile (0, 1) -- row 0 has come by already: here
                        // only for a matrix whose row 0 had no such tile (never: q < Ps[b] means P >= 2)
                        continue;
                    }
                    dag_emit(plan, DAG_DIAG, b, q, q, 0, q, 1, scheme,
                             (unsigned char)((fused(b) ? DAG_FUSED : 0) | (scheme >= 1 && q == 1 ? DAG_WAITNEXT : 0)));
                }
        } else {
            for (const DagTask& t : early_final[q]) plan.tasks.push_back(t);
        }
        // 2. pre-accumulate the diagonal tile of row q+1 over rows [0, q): PARTs now, final (panel q) later.
        // Latency scheme: the PART that needs the block row just above (panel q-1, available only when ALL
        // of row q-1 is finished) is one panel long; the long ones cover [0, q-1) and run a row earlier.
        if (q + 1 < P && q >= 1) {
            const int f_pre = fj(q + 1), span_pre = q - f_pre;      // (skyline: the diagonal tile's history starts at first[q+1])
            const int S_pre = sky
                                  ? dag_sky_pre_parts(span_pre)
                              : fixed_share > 0
                                  ? dag_split_factor(1, q, fixed_share / 4 > 0 ? fixed_share / 4 : 1, scheme)
                                  : dag_split_factor(Bq, span_pre, workers / 4 > 0 ? workers / 4 : 1, scheme);
            for (int b : mats) {
                if (q + 1 >= Ps[b]) continue;
                const unsigned int ctr = plan.n_ctrs++;
                const bool chain = (scheme >= 1);
                if (chain) plan.n_slots += plan.n_slots & 1u;
                const unsigned int slot0 = plan.n_slots;
                const unsigned char flag = chain ? DAG_CHAIN : 0;
                // ranges of the PARTs
                std::vector<std::pair<int, int>> ranges;
                // (second level of following, two-panel finals: the diagonal task itself applies panel q-1 -- with a PART
                // for it, the hand-over of the partial tile sat on the row-to-row path)
                const bool two = xlink(q) && dag_final_panels() == 2;
                if (chain && q >= 2) {
                    int S_long = S_pre;
                    while (S_long > 1 && (q - 1) / S_long < 1) S_long /= 2;
                    for (int sidx = 0; sidx < S_long; ++sidx)
                        ranges.emplace_back((int)((long long)(q - 1) * sidx / S_long),
                                            (int)((long long)(q - 1) * (sidx + 1) / S_long));
                    if (!two) ranges.emplace_back(q - 1, q);
                } else if (span_pre > 0) {      // (nothing to pre-accumulate when the history starts at row q: the final alone)
                    for (int sidx = 0; sidx < S_pre; ++sidx)
                        ranges.emplace_back(f_pre + (int)((long long)span_pre * sidx / S_pre),
                                            f_pre + (int)((long long)span_pre * (sidx + 1) / S_pre));
                }
                const int n_parts = (int)ranges.size();
                for (int sidx = 0; sidx < n_parts; ++sidx) {
                    DagTask t{};
                    t.type = DAG_PART | flag;
                    t.b = (unsigned short)b;
                    t.q = (unsigned char)(q + 1);
                    t.j = (unsigned char)(q + 1);
                    t.S = (unsigned char)(chain ? sidx : 0);
                    t.pa = (unsigned char)ranges[sidx].first;
                    t.pb = (unsigned char)ranges[sidx].second;
                    t.slot = chain ? slot0 + (unsigned int)(sidx & 1) : plan.n_slots++;
                    t.ctr = ctr;
                    plan.tasks.push_back(t);
                }
                if (chain) plan.n_slots = slot0 + (n_parts > 1 ? 2 : 1);
                DagTask fin{};
                fin.type = DAG_DIAG | flag;
                if (chain) fin.type |= DAG_WAITNEXT;
                if (chain && q + 2 < Ps[b] && !(scheme == 2 && q + 1 >= q_f)) fin.type |= DAG_FUSED;
                // second level of following: the strip solve of tile (q, q+1) follows the factorisation of block q
                // (q >= 2) and this task follows IT -- DAG_NOSOLVE here, DAG_FUSED on that strip solve (step 3 below)
                if (xlink(q)) fin.type |= DAG_NOSOLVE;
                fin.b = (unsigned short)b;
                fin.q = fin.j = (unsigned char)(q + 1);
                fin.S = (unsigned char)(n_parts + 1);
                fin.pa = (unsigned char)(two && chain && q >= 2 ? q - 1 : q);
                fin.pb = (unsigned char)(q + 1);
                fin.slot = n_parts == 0 ? 0u : chain ? slot0 + (unsigned int)((n_parts - 1) & 1) : slot0;
                fin.ctr = ctr;
                if (cont0) {
                    fin.type |= DAG_NOSOLVE;          // owned by the strip solve of tile (q, q+1): step 3
                    owned_final[b] = fin;
                    has_owned[b] = 1;
                } else {
                    early_final[q + 1].push_back(fin);
                }
            }
        }
        // 3. off-diagonal tiles of this row
        auto emit_off = [&](int b, int j) {
            const bool owner = cont0 && j == q + 1 && q + 1 < Ps[b];     // its workgroup goes on with DIAG(q+1)
            dag_emit(plan, DAG_OFF, b, q, j, fj(j), q, s_off(b, q - fj(j)), scheme,
                     following ? (unsigned char)(DAG_WAITNEXT | (xlink(q) ? DAG_FUSED : 0) |
                                                 ((j == q + 1 && q + 1 < Ps[b]) ? DAG_NOSOLVE : 0))
                               : (unsigned char)(((j == q + 1 && fused(b)) ? DAG_NOSOLVE : 0) | (owner ? DAG_FUSED : 0)),
                     following ? dag_final_panels() : 1);
            if (owner) {
                if (q == 0) {
                    dag_emit(plan, DAG_DIAG, b, 1, 1, 0, 1, 1, scheme, DAG_NOSOLVE);   // DIAG(1): one final over [0, 1)
                } else {
                    plan.tasks.push_back(owned_final[b]);
                    has_owned[b] = 0;
                }
            }
        };
        if (sky) {
            // (a skyline batch is uniform: every matrix has P block rows)
            for (int j = q + 1; j < P && first[j] <= q; ++j)
                for (int b : mats) emit_off(b, j);
        } else {
            for (int b : mats)
                for (int j = q + 1; j < Ps[b] + Mt && q < Ps[b]; ++j) {
                    if (fj(j) > q) break;      // outside the skyline (first is non-decreasing: so is the rest of the row)
                    emit_off(b, j);
                }
        }
    }
    if (Ms > 0)
        for (int b : mats) dag_emit_schur(plan, b, Ps[b], Ms);
}

// scheme: 0 throughput, 1 latency (dag_emit), -1 automatic: latency while the row-to-row dependency chain,
// not the MFMA work, bounds the run time -- i.e. while a queue has too few block rows in flight to hide the
// wait for the row above.  Measured on MI355X (tools/scheme_table.py; N = 2000 .. 8192, B = 1 .. 32, round 2,
// with the critical path fused into the diagonal tasks): the latency scheme wins or ties while the block
// rows of the matrices of the fullest queue add up to at most ~150 (N = 6000: B = 1: 12.7 -> 4.8 ms,
// B = 8: 17.6 -> 12.9 ms, B = 24: 31.1 -> 30.8 ms; N = 2000, B = 32: 3.9 -> 3.1 ms), or when no queue holds
// more than one matrix; throughput beyond (N = 6000, B = 32: 39.2 vs 39.9 ms; N = 8192, B = 32: 95.0 vs 96.1).
// (Readiness ordering was also tried for the throughput scheme: 800 -> 776 evals/s, not adopted.)
// (Round 6, after the round-5 kernel work: tools/latency_quick.py under PSOAP_DAG_SCHEME=0 / 1, ms per batch, scheme 1 / 0 --
//   N = 6000: 10 matrices 13.03 / 13.50, 12: 15.31 / 15.48, 16: 19.94 / 19.47, 24: 29.14 / 28.37; N = 8192: 12: 36.21 / 35.81, 16:
//   47.86 / 46.81; N = 4096: 20: 8.49 / 8.67, 24: 9.91 / 9.94, 28: 11.41 / 11.35, 32: 12.98 / 12.61; N = 2000: 32: 2.44 / 2.78
// -- the throughput scheme is ahead from about 740 block rows in the launch on (was 1200): 92 per queue.)
constexpr int DAG_LATENCY_QUEUE_ROWS = 92;
// How many of the 8 ticket queues a batch uses (matrix b goes to queue b mod that number; the workgroups of an XCD whose own
// queue is empty spread evenly over the queues in use -- k_chol_dag's steal0).  A queue's matrices share its workgroups, so a
// batch is through when its FULLEST queue is: 12 matrices on 8 queues are 2 + 1 per queue and cost what 16 do, 9 cost
// what 16 do.  Round 4 (tools/queue_sweep.py, profiles/r4_queue_sweep.txt; N = 6000, ms per batch with 8 / 4 / 2 / 1 queues):
//    9 matrices 17.9 / 14.2 / 13.1 / 12.6     12: 20.1 / 16.0 / 16.0 / --      13: 20.3 / 19.4 / 17.7 / 17.4
//   17 matrices 26.8 / 24.0 / 22.2 / 21.8     25: 33.4 / 33.4 / 32.2 / 31.3    16, 24, 32: the same within 0.5 % (8 ahead)
// i.e. time ~ ceil(B / n) x n, with all XCDs drawing from ONE in-order list costing about 1 % (every matrix in front of
// all eight L2s).  The rule: the n in {8, 4, 2, 1} with the smallest ceil(B / n) x n, the larger n on a tie.  Up to 8
// matrices keep a queue each (the XCDs without one steal; one shared queue measures the same).
inline int dag_queue_count(int B)
{
    if (const char* e = getenv("PSOAP_DAG_QUEUES"))      // experiments
        if (atoi(e) > 0) return atoi(e) < DAG_QUEUES ? atoi(e) : DAG_QUEUES;
    if (B <= DAG_QUEUES) return DAG_QUEUES;
    int best = DAG_QUEUES, best_cost = (B + DAG_QUEUES - 1) / DAG_QUEUES * DAG_QUEUES;
    for (int n = DAG_QUEUES / 2; n >= 1; n /= 2) {
        const int cost = (B + n - 1) / n * n;
        if (cost < best_cost) {
            best = n;
            best_cost = cost;
        }
    }
    return best;
}
constexpr int DAG_FOLLOW_MAX_MATS = 8;
constexpr int DAG_FOLLOW_SMALL_ROWS = 20;
inline int dag_auto_scheme(const std::vector<int>& Ps)
{
    long long rows[DAG_QUEUES] = {};
    int count[DAG_QUEUES] = {};
    const int nq = dag_queue_count((int)Ps.size());
    for (size_t b = 0; b < Ps.size(); ++b) {
        rows[b % nq] += Ps[b];
        ++count[b % nq];
    }
    long long max_rows = 0;
    int max_count = 0;
    for (int g = 0; g < DAG_QUEUES; ++g) {
        max_rows = rows[g] > max_rows ? rows[g] : max_rows;
        max_count = count[g] > max_count ? count[g] : max_count;
    }
    // (block rows per XCD: a queue shared by 8 / nq XCDs works its rows off that much faster)
    const int latency = (max_rows * nq <= (long long)DAG_LATENCY_QUEUE_ROWS * DAG_QUEUES || max_count <= 1) ? 1 : 0;
#ifdef PSOAP_FOLLOW
    // following strip solves (scheme 2) where they were measured to win (profiles/r3_follow_table.txt: N = 2000 .. 8192, B =
    // 1 .. 32, against scheme 1 with its PARTs just in time): up to eight matrices everywhere -- single evaluations 12-37 %
    // faster, eight matrices 1-21 % -- and up to 24 small ones (at most 20 block rows: N = 2000, 12 / 16 / 24 matrices 12 /
    // 10 / 3 % faster; from N = 4096 on scheme 1 is 1-2 % ahead at 12 and 16)
    int Pmax = 0;
    for (int P : Ps) Pmax = P > Pmax ? P : Pmax;
    if (latency == 1 && (Ps.size() <= (size_t)DAG_FOLLOW_MAX_MATS || (Ps.size() <= 24 && Pmax <= DAG_FOLLOW_SMALL_ROWS))) return 2;
#endif
    return latency;
}
// fixed_share > 0: the fixed plan (dag_fixed_plan) -- scheme 0, every matrix cut as ONE matrix on `fixed_share` workgroups
// first: the skyline of a uniform likelihood batch (dag_build_queue) -- scheme 0 then, whatever `scheme` says.  A final's
// DagTask::ctr carries in bits 24.. how many tiles its block row is SHORT of the dense P - q (the kernel counts a row's
// finished tasks against it); zero everywhere in a dense list.
inline DagPlan dag_build_tasks(const std::vector<int>& Ps, int workers, int scheme = -1, int Mt = 0, int Ms = 0,
                               int fixed_share = 0, const int* first = nullptr, bool sky_split = false)
{
    DagPlan plan;
    const int B = (int)Ps.size();
    if (fixed_share > 0 || first) scheme = 0;
    if (scheme < 0) scheme = dag_auto_scheme(Ps);
#ifndef PSOAP_FOLLOW
    if (scheme == 2) scheme = 1;       // the following scheme needs the kernels built with -DPSOAP_FOLLOW
#endif
    plan.scheme = scheme;
    // workgroups of XCDs whose own queue is empty steal, so the workers are shared by the queues in use
    const int nq = dag_queue_count(B);
    const int used = B < nq ? (B > 0 ? B : 1) : nq;
    const int per_queue = workers / used > 0 ? workers / used : 1;
    for (int g = 0; g < DAG_QUEUES; ++g) {
        plan.queues.first[g] = (unsigned int)plan.tasks.size();
        std::vector<int> mats;
        if (g < nq)
            for (int b = g; b < B; b += nq) mats.push_back(b);
        dag_build_queue(plan, mats, Ps, per_queue, (B + nq - 1) / nq, scheme, Mt, Ms, fixed_share, first, sky_split);
        if (scheme >= 1) {
            // Latency scheme: hand the tasks out in order of READINESS instead of block row by block row.
            // A task over panels [pa, pb) can run once block row pb-1 is finished ("stage" pb); within a
            // stage the diagonal final (the in-block Cholesky everybody waits for) comes first, then the
            // row's other finals, then the PARTs that just became ready, nearest block row first.  PARTs of
            // far-away rows thus run as soon as their panels exist instead of arriving in a burst when
            // their row comes up, and a worker rarely takes a ticket it then has to spin on.  Every wait
            // still targets a smaller ticket: a chain's PARTs have increasing pb, its final the largest.
            // (the update-only task of tile (q, q+1), which DIAG(q) waits for after its factorisation, goes in
            // front of it: every wait still targets a smaller ticket)
            auto cls = [](const DagTask& t) {
                const int ty = t.type & DAG_TYPE_MASK;
                if (ty == DAG_OFF && (t.type & DAG_NOSOLVE) && !(t.type & DAG_WAITNEXT)) return -1;   // update-only: in front of its DIAG
                if (ty == DAG_PART && t.pb == 0 && t.q == t.j && t.q <= 1) return -2;  // the running sum DIAG(0) / DIAG(1) start from
                return ty == DAG_DIAG ? 0 : (ty == DAG_OFF ? 1 : 2);      // PART and DAG_SCHUR: whatever is left of a stage
            };
            // (scheme 2, PSOAP_DAG_EARLY=1: a final that covers two panels -- a following strip solve or the diagonal task that
            // follows one, from block row 4 on -- starts with the older panel, i.e. could be picked up a stage early.  That
            // paid while the PARTs were in readiness order (the finals queued behind a whole round of them, 110 us at
            // N = 6000, q = 8); with the PARTs handed out just in time -- below -- it only makes the finals hold their
            // workgroups longer: N = 6000: 2.68 -> 2.59 ms for one evaluation, 6.46 -> 6.17 for four WITHOUT it.  Off.)
            // (latency schemes, PARTs: not before block row q - jit is the current one.  In pure readiness order the early stages
            // hold every far row's first PARTs -- ~300 tasks per stage at N = 6000 against ~50 at the end -- and the
            // finals of the next rows queue up behind them: 90 us per block row over the first third of the matrix
            // instead of 45.  Just in time, every stage holds about one block row's worth of PARTs.)
            // (scheme 1 as well -- it is what 17 .. 32 matrices of N <= 4096 and 17 .. 24 of N = 6000 get: 1-5 % there;
            // PSOAP_DAG_JIT1=0 keeps its PARTs in readiness order)
            static const bool jit1 = !(getenv("PSOAP_DAG_JIT1") && getenv("PSOAP_DAG_JIT1")[0] == '0');
            const int jit = (scheme == 2 || (scheme == 1 && jit1)) ? dag_jit_rows() : 0;
            // (the PARTs of the Schur tiles of predict, rows q >= P, keep their place: they are the filler work)
            auto jit_part = [jit, &Ps](const DagTask& t) {
                return jit > 0 && (t.type & DAG_TYPE_MASK) == DAG_PART && (t.type & DAG_CHAIN) && (int)t.q < Ps[t.b];
            };
            // (measured: 6 block rows ahead; 4 .. 12 within 2 %, a lead that grows with the row index 5-8 % worse)
            // (... and a chain's parts one after the other over the stages of that lead, not all in its first one: a part
            // waits for its predecessor, and a workgroup that holds a waiting part works on nothing else)
            std::vector<int> chain_parts(plan.n_ctrs + 1, 1);
            if (jit > 0)
                for (size_t i = plan.queues.first[g]; i < plan.tasks.size(); ++i) {
                    const DagTask& t = plan.tasks[i];
                    if ((t.type & DAG_TYPE_MASK) != DAG_PART && (t.type & DAG_CHAIN) && t.S > 1) chain_parts[t.ctr] = t.S - 1;
                }
            auto stage = [jit, &jit_part, &chain_parts](const DagTask& t) {
                const int ty = t.type & DAG_TYPE_MASK;
                if (jit_part(t)) {
                    const int spread = jit > 2 ? (int)t.S * (jit - 2) / chain_parts[t.ctr] : 0;
                    return std::max((int)t.pb, (int)t.q - jit + spread);
                }
                const bool follows = (ty == DAG_OFF && (t.type & DAG_WAITNEXT)) || (ty == DAG_DIAG && (t.type & DAG_NOSOLVE));
                static const bool early = getenv("PSOAP_DAG_EARLY") && getenv("PSOAP_DAG_EARLY")[0] == '1';   // experiments
                return (early && follows && t.q >= 4 && t.pb - t.pa >= 2) ? t.pb - 1 : (int)t.pb;   // (q >= 4: what it follows is a stage early too)
            };
            // (the finals of a stage row by row -- only scheme 2 has finals of two rows in one stage, and those of the
            // lower row follow those of the upper one)
            std::stable_sort(plan.tasks.begin() + plan.queues.first[g], plan.tasks.end(),
                             [&](const DagTask& a, const DagTask& b) {
                                 if (stage(a) != stage(b)) return stage(a) < stage(b);
                                 const int ca = cls(a), cb = cls(b);
                                 if ((ca == 2) != (cb == 2)) return cb == 2;     // (finals behind the PARTs of their stage: 3-6 % slower)
                                 // (tried: within a stage the PARTs that wait for nothing ahead of the ones that need the row
                                 // just finishing -- 3-5 % slower: those are the chains of the nearest rows)
                                 if (a.q != b.q) return a.q < b.q;
                                 if (ca != cb) return ca < cb;
                                 // (just in time: the chains of a row's tiles side by side -- first parts, second parts, ...
                                 // -- not tile after tile: a part waits for its predecessor)
                                 if (jit_part(a) && jit_part(b) && a.S != b.S) return a.S < b.S;
                                 return false;
                             });
        }
    }
    plan.queues.first[DAG_QUEUES] = (unsigned int)plan.tasks.size();
    if (first)
        for (DagTask& t : plan.tasks)
            if ((t.type & DAG_TYPE_MASK) != DAG_PART)
                t.ctr |= (unsigned int)(Ps[t.b] - t.q - dag_sky_row_tiles(first, Ps[t.b], t.q)) << 24;
    plan.queues.follow_first = (unsigned int)dag_follow_first_row();
    return plan;
}

// How many persistent workgroups a batch gets: all the device admits (two per compute unit), or ONE per compute
// unit when the batch is bound by the row-to-row chains of its matrices and not by MFMA throughput.  The
// in-block factorisation on a chain is VALU / LDS work in dependent steps; an MFMA-streaming workgroup on the
// same compute unit owns the double-precision pipe for 64 cycles per instruction and slows it up to 2x
// (priorities only decide who issues next).  With one workgroup per compute unit the chain runs undisturbed:
// N = 6000: 4.1 -> 3.5 ms for one evaluation, N = 2000, B = 8: 1.40 -> 1.27 ms -- but the device then
// delivers roughly half the throughput, so the switch is by work: measured over N = 2000 .. 8192, B = 1 .. 32
// (tools/latency_quick.py under PSOAP_DAG_WORKERS), one per compute unit wins while
//     algorithmic flops of the batch  <=  3.3e9 x block rows of its largest matrix
// (chain time ~ 75 us per block row against ~35 TFLOP/s of the half-populated device), i.e. B N^2 <~ 7.7e7.
// Round 3 (following scheme): several matrices -- 2.0e9 instead of 3.3e9: their strip solves hold workgroups while they
// follow the factorisation, which a second workgroup per compute unit makes up for earlier (N = 6000, B = 2: 4.29 -> 3.99
// ms; N = 4096, B = 4: 2.87 -> 2.70 ms; N = 4096, B = 2 stays with one: 1.92 against 2.15 ms).
// Round 4: one workgroup per compute unit now means the kernels compiled for one wave per SIMD (512 registers per lane,
// nothing of the chain phases in scratch memory: 3-7 % faster), which moves the crossover for several matrices back to
// 3.3e9: N = 4096, 3 / 4 matrices 2.39 -> 2.16 / 2.74 -> 2.62 ms, N = 6000, 2 matrices 3.94 -> 3.83 ms; beyond (N = 4096:
// 6, N = 6000: 3, N = 8192: 2 matrices) two per compute unit stay 5-12 % ahead.
inline int dag_pick_workers(double flops, int Pmax, int compute_units, int max_workers, int n_mats = 1)
{
    if (const char* e = getenv("PSOAP_DAG_WORKERS"))      // experiments
        if (atoi(e) > 0) return atoi(e);
    if (max_workers <= compute_units) return max_workers;
    (void)n_mats;
    return flops <= 3.3e9 * (double)Pmax ? compute_units : max_workers;
}
inline double dag_batch_flops(const std::vector<int>& Ps, int Mt = 0)
{
    double f = 0.0;
    for (int P : Ps) {
        const double n = 128.0 * P, r = 128.0 * Mt;
        f += n * n * n / 3.0 + n * n * r;
    }
    return f;
}

// The task list every lane of a stream runs (one matrix), cut as if `lanes` matrices shared `workers` workgroups, with its
// bursts marked (DagTask::b, which the lanes do not need: the matrix index is the lane).  A burst is what the workgroups of
// an XCD draw from one lane before they move on to the next: one block row -- scheme 0: the tasks emitted for row q (the
// PARTs that pre-accumulate DIAG(q+1), the row's strip solves with their PARTs, the owned DIAG(q+1)); schemes 1, 2:
// whatever precedes a diagonal final.  bursts == false: every ticket ends one (the lanes ticket by ticket in turn).
// The list depends on P and the scheme ONLY -- the split factors are those of a nominal 32 lanes whatever the stream's
// lane count -- so a proposal's result is bit-identical for every lane count, batch size, submission order and world size.
// Scheme 0 splits half as eagerly as a plain launch does (a row's tiles are cut while `tiles x parts` stays below HALF the
// workgroups' share of one lane): with other matrices in other phases always in flight, sparse block
// rows need not fill the device by themselves, and every part saved is a partial tile that does not travel (measured:
// 38.5 -> 38.2 ms per 32-walker step).
inline DagPlan dag_build_lane_plan(int P, int lanes, int workers, int scheme, bool bursts = true)
{
    (void)lanes;
    // (scheme 0: dag_nominal_share -- half the workgroups' share of one of 32 lanes: the fixed plan, also what a batch
    // launch gets under PSOAP_FIXED_PLAN=1)
    const int share15 = workers / STREAM_NOMINAL_LANES > 0 ? workers / STREAM_NOMINAL_LANES : 1;
    DagPlan plan = scheme == 0 ? dag_build_tasks(std::vector<int>(1, P), share15, 0, 0, 0, dag_nominal_share(workers))
                               : dag_build_tasks(std::vector<int>(1, P), share15, scheme);
    const bool rows = plan.scheme == 0;
    // (schemes 1, 2: the list is in order of readiness already and its tasks are short -- the lanes ticket by ticket in turn
    // measured 8 % faster at N = 2000, the same at N = 4096)
    if (plan.scheme != 0) bursts = false;
    auto section = [](const DagTask& t) { return (t.q == t.j && t.q > 0) ? (int)t.q - 1 : (int)t.q; };
    for (size_t i = 0; i < plan.tasks.size(); ++i) {
        const bool last = i + 1 == plan.tasks.size();
        bool end = !bursts || last;
        if (!end) {
            const DagTask& nx = plan.tasks[i + 1];
            end = rows ? section(nx) != section(plan.tasks[i]) : (nx.type & DAG_TYPE_MASK) == DAG_DIAG;
        }
        plan.tasks[i].b = (unsigned short)(end ? STREAM_BURST_END : 0);
    }
    return plan;
}

// uniform batch: B matrices of P block rows each
inline DagPlan dag_build_tasks(int B, int P, int workers, int scheme = -1, int Mt = 0, int Ms = 0)
{
    return dag_build_tasks(std::vector<int>((size_t)(B > 0 ? B : 0), P), workers, scheme, Mt, Ms);
}

// ---- the plan rule ---------------------------------------------------------------------------------
// PSOAP_DAG_SCHEME=0|1|2 pins the split scheme (experiments); -1: automatic.  Read when a plan is built.
inline int dag_env_scheme()
{
    const char* e = getenv("PSOAP_DAG_SCHEME");
    return e ? atoi(e) : -1;
}

// workgroups of a batch (Ps[b] block rows each, Mt appended column tiles) on a device with `compute_units` CUs that admits
// `max_workers` of them
inline int dag_batch_workers(const std::vector<int>& Ps, int Mt, int compute_units, int max_workers)
{
    int Pmax = 0;
    for (int P : Ps) Pmax = P > Pmax ? P : Pmax;
    return dag_pick_workers(dag_batch_flops(Ps, Mt), Pmax, compute_units, max_workers, (int)Ps.size());
}

// The task list of a likelihood launch (a chunk's batch, a group's): the batch's workers (*workers), the scheme
// PSOAP_DAG_SCHEME pins, and under PSOAP_FIXED_PLAN=1 the task structure of a stream lane for every matrix, whatever the
// batch (dag_fixed_plan).  Predict builds its plan from the same pieces with its Mt / Ms (predict_run).
inline DagPlan dag_lnlike_plan(const std::vector<int>& Ps, int n_cus, int dag_grid, int* workers)
{
    *workers = dag_batch_workers(Ps, 0, n_cus, dag_grid);
    return dag_build_tasks(Ps, *workers, dag_env_scheme(), 0, 0, dag_fixed_plan() ? dag_nominal_share(dag_grid - 1) : 0);
}

// the scheme dag_lnlike_plan's list is built for (psoap_batch_eval asks before it builds: only scheme 0 reads a skyline)
inline int dag_lnlike_scheme(const std::vector<int>& Ps)
{
    if (dag_fixed_plan()) return 0;
    const int e = dag_env_scheme();
    int scheme = e >= 0 ? e : dag_auto_scheme(Ps);
#ifndef PSOAP_FOLLOW
    if (scheme == 2) scheme = 1;
#endif
    return scheme;
}

// The throughput list of a uniform batch inside the skyline first[0 .. P) (sky_kernels.hpp; dag_build_queue)
// (sky_split: the skyline-aware rules -- the handle's PSOAP_SKY_SPLIT, read at its creation)
inline DagPlan dag_lnlike_plan_sky(int B, int P, const int* first, int n_cus, int dag_grid, int* workers, bool sky_split)
{
    const std::vector<int> Ps((size_t)B, P);
    *workers = dag_batch_workers(Ps, 0, n_cus, dag_grid);
    return dag_build_tasks(Ps, *workers, 0, 0, 0, 0, first, sky_split);
}

// what a list executes: tiles (finals), tile-GEMM units (128-row panels of the updates), MFMA flops (updates + strip solves)
struct DagPlanWork {
    long long tiles = 0, units = 0;
    double flops = 0.0;
};
inline DagPlanWork dag_plan_work(const DagPlan& plan)
{
    DagPlanWork w;
    long long solves = 0;
    for (const DagTask& t : plan.tasks) {
        const int ty = t.type & DAG_TYPE_MASK;
        w.units += (int)t.pb - (int)t.pa;
        if (ty != DAG_PART) ++w.tiles;
        if (ty == DAG_OFF) ++solves;
    }
    w.flops = 2.0 * NB * NB * NB * (double)(w.units + solves);
    return w;
}

// the LAT kernels (and predict's, the stream's): at most two workgroups per compute unit
inline int dag_two_per_cu(int workers, int n_cus) { return workers > 2 * n_cus ? 2 * n_cus : workers; }
}  // namespace psoap
