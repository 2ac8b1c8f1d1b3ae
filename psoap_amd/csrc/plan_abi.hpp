// plan_abi.hpp -- the pure-host entry points of the C ABI (include/psoap_gp.h): the planner's task lists and the host
// twins of the skyline kernels.  No HIP call and no HIP header: psoap_gp.hip includes it into the library, and a host
// compiler builds the same text into stand-alone, sanitized programs (tests/host/plan_host_check.cpp, sky_fine_host_check.cpp).
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "abi_error.hpp"
#include "dag_plan.hpp"
#include "draw_rng.hpp"
#include "mix_plan.hpp"
#include "sky_rules.hpp"
#include "vel_fisher_plan.hpp"

using namespace psoap;

// what every plan entry point hands back: the counts, the queues' first tickets, and min(max_tasks, n_tasks) task records
static void plan_export(const DagPlan& plan, void* out, long long max_tasks, long long* n_tasks, long long* n_slots,
                        long long* n_ctrs, unsigned int* queue_first)
{
    *n_tasks = (long long)plan.tasks.size();
    if (n_slots) *n_slots = plan.n_slots;
    if (n_ctrs) *n_ctrs = plan.n_ctrs;
    if (queue_first) memcpy(queue_first, plan.queues.first, sizeof plan.queues.first);
    if (out) {
        const long long n = max_tasks < *n_tasks ? max_tasks : *n_tasks;
        memcpy(out, plan.tasks.data(), sizeof(DagTask) * n);
    }
}

// Pure host function (no HIP call): the task list the persistent kernel would run for a batch of
// B matrices with P block rows on `workers` workgroups.  Lets the scheduler be validated on a CPU.
extern "C" int psoap_dag_plan(int B, int P, int workers, void* out, long long max_tasks, long long* n_tasks,
                              long long* n_slots, long long* n_ctrs, unsigned int* queue_first)
{
    if (B < 1 || P < 1 || P > 255 || workers < 1 || !n_tasks) FAIL("psoap_dag_plan: bad arguments");
    plan_export(dag_build_tasks(B, P, workers), out, max_tasks, n_tasks, n_slots, n_ctrs, queue_first);
    return 0;
}

// Pure host function: the throughput list of the same batch inside the skyline first[0 .. P) (tile (q, j) exists iff
// q >= first[j]; non-decreasing, first[j] <= max(j - 1, 0)).  All zero: psoap_dag_plan's list, byte for byte.
extern "C" int psoap_dag_plan_sky(int B, int P, const int* first, int workers, void* out, long long max_tasks,
                                  long long* n_tasks, long long* n_slots, long long* n_ctrs, unsigned int* queue_first)
{
    if (B < 1 || P < 1 || P > 255 || workers < 1 || !n_tasks || !first) FAIL("psoap_dag_plan_sky: bad arguments");
    bool any = false;
    for (int j = 0; j < P; ++j) {
        if (first[j] < 0 || first[j] > (j > 0 ? j - 1 : 0) || (j > 0 && first[j] < first[j - 1]))
            FAIL("psoap_dag_plan_sky: first must be non-decreasing with 0 <= first[j] <= max(j - 1, 0)");
        any = any || first[j] > 0;
    }
    DagPlan plan = any ? dag_build_tasks(std::vector<int>((size_t)B, P), workers, 0, 0, 0, 0, first, dag_sky_split_env())
                       : dag_build_tasks(B, P, workers);
    plan_export(plan, out, max_tasks, n_tasks, n_slots, n_ctrs, queue_first);
    return 0;
}

// One candidate order on the host, by the routines the upload-side kernels run (sky_rules.hpp): its permutation and its
// union skyline over the batch lwl (B, c, N), gp (B, 2c); returns the envelope's cost (sky_cost).  first_b, if given: the
// per-matrix skylines (B, P) the union is the minimum of
static long long sky_host_candidate(int c, int N, int B, const double* lwl, const double* gp, int cand, std::vector<int>& perm,
                                    std::vector<int>& first, std::vector<int>* first_b = nullptr)
{
    const int P = round_up(N, NB) / NB;
    double w[3];
    sky_cand_weights(c, cand, w);
    std::vector<unsigned long long> key((size_t)N);
    for (int i = 0; i < N; ++i) {
        double v[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < c; ++k) v[k] = lwl[(size_t)k * N + i];
        key[i] = sky_key(sky_cand_key(c, w, v));
    }
    perm.resize((size_t)N);
    first.assign((size_t)P, 0);
    for (int i = 0; i < N; ++i) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&key](int a, int b) { return key[a] < key[b]; });
    std::vector<double> x((size_t)c * N), lo((size_t)c * P), hi((size_t)c * P);
    std::vector<int> fb((size_t)P);
    for (int b = 0; b < B; ++b) {
        for (int k = 0; k < c; ++k)
            for (int r = 0; r < N; ++r) x[(size_t)k * N + r] = lwl[((size_t)b * c + k) * N + perm[r]];
        for (int k = 0; k < c; ++k)
            for (int t = 0; t < P; ++t)
                sky_interval(x.data() + (size_t)k * N, t * NB, (t + 1) * NB < N ? (t + 1) * NB : N, &lo[(size_t)k * P + t],
                             &hi[(size_t)k * P + t]);
        double p2[3] = {0.0, 0.0, 0.0};
        const bool ok = sky_gp(gp + (size_t)b * 2 * c, c, p2);
        for (int j = 0; j < P; ++j) fb[j] = sky_first_raw(j, P, c, lo.data(), hi.data(), p2, ok);
        sky_first_finish(fb.data(), P);
        for (int j = 0; j < P; ++j) first[j] = (b == 0 || fb[j] < first[j]) ? fb[j] : first[j];
        if (first_b) first_b->insert(first_b->end(), fb.begin(), fb.end());
    }
    return sky_cost(first.data(), P);
}

// The first n_cand candidate orders of the batch lwl (B, c, N), gp (B, 2c): the cheapest envelope wins, ties to the lowest
// candidate.  cand_out: the winner; perm_out (N) and first_out (ceil(N / 128)): its permutation and union skyline; any
// output may be null.  Beyond SKY_MAX_N: the identity permutation and the dense skyline.
static void sky_host_order(int c, int N, int B, const double* lwl, const double* gp, int n_cand, int* first_out, int* perm_out,
                           int* cand_out)
{
    const int P = round_up(N, NB) / NB;
    std::vector<int> perm((size_t)N), first((size_t)P, 0);
    for (int i = 0; i < N; ++i) perm[i] = i;
    int best = 0;
    if (N <= SKY_MAX_N) {
        long long best_cost = sky_host_candidate(c, N, B, lwl, gp, 0, perm, first);
        std::vector<int> pk, fk;
        for (int k = 1; k < n_cand; ++k) {
            const long long cost = sky_host_candidate(c, N, B, lwl, gp, k, pk, fk);
            if (cost < best_cost) {
                best_cost = cost;
                best = k;
                perm.swap(pk);
                first.swap(fk);
            }
        }
    }
    if (perm_out) memcpy(perm_out, perm.data(), sizeof(int) * (size_t)N);
    if (first_out) memcpy(first_out, first.data(), sizeof(int) * (size_t)P);
    if (cand_out) *cand_out = best;
}

// Pure host function, the twin of the upload-side kernels pinned to candidate 0 (the order by the first walker's first
// component; what a handle created under PSOAP_SKY_ORDER=0 computes): the permutation and the union skyline of a batch
// lwl (B, c, N), gp (B, 2c).  perm_out (N), first_out (ceil(N / 128)); either may be null.
extern "C" int psoap_sky_first(int c, int N, int B, const double* lwl, const double* gp, int* first_out, int* perm_out)
{
    if (c < 1 || c > 3 || N < 1 || B < 1 || !lwl || !gp) FAIL("psoap_sky_first: bad arguments");
    sky_host_order(c, N, B, lwl, gp, 1, first_out, perm_out, nullptr);
    return 0;
}

// Pure host function, the twin of the upload-side kernels as a handle runs them: every candidate order of the batch
// (sky_n_cand(c) of them), the cheapest envelope wins, ties to the lowest candidate.  cand_out: the winner; perm_out (N)
// and first_out (ceil(N / 128)): its permutation and union skyline; any output may be null.
extern "C" int psoap_sky_order(int c, int N, int B, const double* lwl, const double* gp, int* first_out, int* perm_out,
                               int* cand_out)
{
    if (c < 1 || c > 3 || N < 1 || B < 1 || !lwl || !gp) FAIL("psoap_sky_order: bad arguments");
    sky_host_order(c, N, B, lwl, gp, sky_n_cand(c), first_out, perm_out, cand_out);
    return 0;
}

// Pure host function, the twin of what the kernel's clip reads (DagMat::first): the winning candidate of psoap_sky_order and
// its per-matrix skylines first_b_out (B, ceil(N / 128)) -- the union is their minimum over the batch -- with the tile-GEMM
// units they leave, summed over the batch, in *units_out.  Any output may be null.  Beyond SKY_MAX_N: all zero, dense.
extern "C" int psoap_sky_clip(int c, int N, int B, const double* lwl, const double* gp, int* first_b_out, long long* units_out,
                              int* cand_out)
{
    if (c < 1 || c > 3 || N < 1 || B < 1 || !lwl || !gp) FAIL("psoap_sky_clip: bad arguments");
    const int P = round_up(N, NB) / NB;
    int cand = 0;
    sky_host_order(c, N, B, lwl, gp, sky_n_cand(c), nullptr, nullptr, &cand);
    std::vector<int> perm, first, first_b;
    if (N <= SKY_MAX_N) sky_host_candidate(c, N, B, lwl, gp, cand, perm, first, &first_b);
    else first_b.assign((size_t)B * P, 0);
    long long units = 0;
    for (int b = 0; b < B; ++b) units += sky_cost(first_b.data() + (size_t)b * P, P);
    if (first_b_out) memcpy(first_b_out, first_b.data(), sizeof(int) * (size_t)B * P);
    if (units_out) *units_out = units;
    if (cand_out) *cand_out = cand;
    return 0;
}

// Pure host function, the twin of k_sky_fine: the winning candidate of psoap_sky_order and, per matrix and column tile, the
// first 16-row group that is not provably zero -- first16_b_out (B, ceil(N / 128)), what DagMat::first points at: clamped to
// 8 max(j - 1, 0), non-decreasing, at or beyond 8 times psoap_sky_clip's row (checked here) -- with the 16-row stages the
// updates of the union's list then run, summed over the batch, in *stages_out (sky_stages_col).  Any output may be null.
// Beyond SKY_MAX_N: all zero, dense.
extern "C" int psoap_sky_clip16(int c, int N, int B, const double* lwl, const double* gp, int* first16_b_out, long long* stages_out,
                                int* cand_out)
{
    if (c < 1 || c > 3 || N < 1 || B < 1 || !lwl || !gp) FAIL("psoap_sky_clip16: bad arguments");
    const int P = round_up(N, NB) / NB, G = round_up(N, SKY_G) / SKY_G;
    int cand = 0;
    sky_host_order(c, N, B, lwl, gp, sky_n_cand(c), nullptr, nullptr, &cand);
    std::vector<int> perm, first((size_t)P, 0), first_b, first16((size_t)B * P, 0);
    long long stages = 0;
    if (N <= SKY_MAX_N) {
        sky_host_candidate(c, N, B, lwl, gp, cand, perm, first, &first_b);
        std::vector<double> x((size_t)c * N), lo((size_t)c * P), hi((size_t)c * P), lo16((size_t)c * G), hi16((size_t)c * G);
        for (int b = 0; b < B; ++b) {
            for (int k = 0; k < c; ++k) {
                double* xk = x.data() + (size_t)k * N;
                for (int r = 0; r < N; ++r) xk[r] = lwl[((size_t)b * c + k) * N + perm[r]];
                for (int t = 0; t < P; ++t)
                    sky_interval(xk, t * NB, (t + 1) * NB < N ? (t + 1) * NB : N, &lo[(size_t)k * P + t], &hi[(size_t)k * P + t]);
                for (int g = 0; g < G; ++g)
                    sky_interval(xk, g * SKY_G, (g + 1) * SKY_G < N ? (g + 1) * SKY_G : N, &lo16[(size_t)k * G + g],
                                 &hi16[(size_t)k * G + g]);
            }
            double p2[3] = {0.0, 0.0, 0.0};
            const bool ok = sky_gp(gp + (size_t)b * 2 * c, c, p2);
            int* f16 = first16.data() + (size_t)b * P;
            for (int j = 0; j < P; ++j) f16[j] = sky_first16_raw(j, G, P, c, lo16.data(), hi16.data(), lo.data(), hi.data(), p2, ok);
            sky_first16_finish(f16, P);
            for (int j = 0; j < P; ++j)
                if (f16[j] < SKY_GPT * first_b[(size_t)b * P + j]) FAIL("psoap_sky_clip16: a column starts above its own first tile");
        }
    }
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < P; ++j) stages += sky_stages_col(j, first[j], first16[(size_t)b * P + j]);
    if (first16_b_out) memcpy(first16_b_out, first16.data(), sizeof(int) * (size_t)B * P);
    if (stages_out) *stages_out = stages;
    if (cand_out) *cand_out = cand;
    return 0;
}

// Pure host function: the task list every lane of a stream of `lanes` lanes runs for matrices of P block rows
// (dag_build_lane_plan); DagTask::b carries the burst marks (0x8000: the last ticket of a burst).
extern "C" int psoap_stream_plan(int P, int lanes, int workers, int scheme, void* out, long long max_tasks,
                                 long long* n_tasks, long long* n_slots, long long* n_ctrs, int* scheme_out)
{
    if (P < 1 || P > 255 || lanes < 1 || lanes > STREAM_MAX_LANES || workers < 1 || scheme < -1 || scheme > 2 || !n_tasks)
        FAIL("psoap_stream_plan: bad arguments");
    if (scheme < 0) scheme = dag_auto_scheme(std::vector<int>((size_t)lanes, P));
    DagPlan plan = dag_build_lane_plan(P, lanes, workers, scheme);
    plan_export(plan, out, max_tasks, n_tasks, n_slots, n_ctrs, nullptr);
    if (scheme_out) *scheme_out = plan.scheme;
    return 0;
}

// One matrix with Mt appended column tiles (predict) and, when Ms > 0, the Ms x Ms tiles of their Schur complement as
// tasks of the same launch (DAG_SCHUR).  scheme: -1 automatic, 0 throughput, 1 latency.
extern "C" int psoap_dag_plan_aug(int P, int Mt, int Ms, int workers, int scheme, void* out, long long max_tasks,
                                  long long* n_tasks, long long* n_slots, long long* n_ctrs, unsigned int* queue_first)
{
    if (P < 1 || Mt < 0 || Ms < 0 || Ms > Mt || P + Mt > 255 || workers < 1 || !n_tasks)
        FAIL("psoap_dag_plan_aug: bad arguments");
    plan_export(dag_build_tasks(1, P, workers, scheme, Mt, Ms), out, max_tasks, n_tasks, n_slots, n_ctrs, queue_first);
    return 0;
}

// The same for a heterogeneous batch: matrix b has Ps[b] block rows.
extern "C" int psoap_dag_plan_multi(int B, const int* Ps, int workers, void* out, long long max_tasks,
                                    long long* n_tasks, long long* n_slots, long long* n_ctrs,
                                    unsigned int* queue_first)
{
    if (B < 1 || !Ps || workers < 1 || !n_tasks) FAIL("psoap_dag_plan_multi: bad arguments");
    for (int b = 0; b < B; ++b)
        if (Ps[b] < 1 || Ps[b] > 255) FAIL("psoap_dag_plan_multi: 1 <= P <= 255");
    plan_export(dag_build_tasks(std::vector<int>(Ps, Ps + B), workers), out, max_tasks, n_tasks, n_slots, n_ctrs, queue_first);
    return 0;
}

// Pure host function: how many persistent workgroups a batch of B matrices (Ps[b] block rows each, Mt appended
// column tiles) gets on a device with `compute_units` CUs that admits `max_workers` of them (dag_pick_workers).
extern "C" int psoap_dag_pick_workers(int B, const int* Ps, int Mt, int compute_units, int max_workers, int* workers)
{
    if (B < 1 || !Ps || Mt < 0 || compute_units < 1 || max_workers < 1 || !workers) FAIL("psoap_dag_pick_workers: bad arguments");
    *workers = dag_batch_workers(std::vector<int>(Ps, Ps + B), Mt, compute_units, max_workers);
    return 0;
}

// Pure host function: the counter block (pair index c0, draw index c1) of the generator behind psoap_chunk_predict_draw and
// psoap_draw_normals (draw_rng.hpp: Philox4x32-10, key = the two words of seed, counter (c0, c1, 0, 0)).
extern "C" int psoap_draw_philox(unsigned long long seed, unsigned int c0, unsigned int c1, unsigned int out[4])
{
    if (!out) FAIL("psoap_draw_philox: bad arguments");
    const PhiloxBlock b = draw_block(seed, c0, c1);
    for (int k = 0; k < 4; ++k) out[k] = b.w[k];
    return 0;
}

// Pure host function: the plan of a mixture of R prediction rows and up to S_max samples (mix_plan.hpp) -- the padded sizes,
// the upper tiles of the rank-S product in launch order (tiles_out: min(max_tiles, n_tiles) pairs (ti, tj); may be null) and
// the bytes of all its device buffers.  Any output may be null.
extern "C" int psoap_mix_plan(int R, int S_max, int want_sigma, int* Rpad, int* Spad, int* n_tiles, int* tiles_out, int max_tiles,
                              long long* bytes)
{
    if (const char* why = mix_check_plan(R, S_max, want_sigma)) FAIL(std::string("psoap_mix_plan: ") + why);
    MixPlan g;
    mix_plan(R, S_max, want_sigma, g);
    if (Rpad) *Rpad = g.Rpad;
    if (Spad) *Spad = g.Spad;
    if (n_tiles) *n_tiles = (int)g.tiles.size();
    if (tiles_out)
        for (int t = 0; t < (int)g.tiles.size() && t < max_tiles; ++t) tiles_out[2 * t] = g.tiles[(size_t)t].ti, tiles_out[2 * t + 1] = g.tiles[(size_t)t].tj;
    if (bytes) *bytes = g.bytes;
    return 0;
}

// Pure host function: the plan of psoap_chunk_fisher_vel for a chunk of N pixels with the epoch index `epoch` (N values in
// [0, n_epochs)) and c components (vel_fisher_plan.hpp) -- the number of slots (the distinct epochs of every 128-row tile
// row), slot_of_out (N): the slot of every pixel, slot_first_out (ceil(N / 128) + 1), slot_epoch_out (min(max_slots, n_slots)),
// the numbers of tiles of the two product launches and the bytes of every device buffer beyond [K | I].  Any output may be null.
extern "C" int psoap_vel_fisher_plan(int c, int N, int n_epochs, const int32_t* epoch, int* n_slots, int* slot_of_out,
                                     int* slot_first_out, int* slot_epoch_out, int max_slots, int* n_tiles_all, int* n_tiles_upper,
                                     long long* bytes)
{
    if (const char* why = vel_fisher_check(c, N, n_epochs, epoch)) FAIL(std::string("psoap_vel_fisher_plan: ") + why);
    VelFisherPlan g;
    vel_fisher_plan(c, N, n_epochs, epoch, g);
    if (n_slots) *n_slots = g.S;
    if (slot_of_out) memcpy(slot_of_out, g.slot_of.data(), sizeof(int) * (size_t)N);
    if (slot_first_out) memcpy(slot_first_out, g.slot_first.data(), sizeof(int) * ((size_t)g.P + 1));
    if (slot_epoch_out)
        for (int a = 0; a < g.S && a < max_slots; ++a) slot_epoch_out[a] = g.slot_epoch[(size_t)a];
    if (n_tiles_all) *n_tiles_all = (int)g.tiles_all.size();
    if (n_tiles_upper) *n_tiles_upper = (int)g.tiles_upper.size();
    if (bytes) *bytes = g.bytes;
    return 0;
}
