// sky_split_host_check.cpp -- the skyline-aware split and order rules of the planner (psoap_amd/csrc/dag_plan.hpp,
// PSOAP_SKY_SPLIT) as a stand-alone host program: no HIP header, no HIP library.  tests/test_sky_split_host.py builds it with
// AddressSanitizer and UBSan and runs it; every output buffer has exactly the reported size, so an overrun is a sanitizer
// report.  For a grid of envelopes, with the rules on and off (PSOAP_SKY_SPLIT=0): the list's counts and FNV-1a hash, one line
// per case -- the test makes the same calls into libpsoap_gp.so and expects the same lines -- and, checked here, what the
// kernel relies on: slots and counters inside the reported counts, PART ranges that tile [first[j], q) ahead of their final.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <memory>
#include <tuple>

#include "../../include/psoap_gp.h"
#include "../../psoap_amd/csrc/plan_abi.hpp"

typedef unsigned long long u64;

static u64 fnv1a(const void* p, size_t bytes)
{
    const unsigned char* c = static_cast<const unsigned char*>(p);
    u64 h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ c[i]) * 0x100000001b3ull;
    return h;
}

static int g_failed = 0;
static void fail(const char* what, int B, int P, int kind, int split)
{
    fprintf(stderr, "B=%d P=%d kind=%d split=%d: %s\n", B, P, kind, split, what);
    g_failed = 1;
}

// kind 0: band of width P / 2; 1: band of width 2; 2: the tight envelope first[j] = max(j - 1, 0); 3: dense up to P / 2, then
// a band of that width (the headline's shape); 4: a step
static std::vector<int> envelope(int P, int kind)
{
    std::vector<int> f((size_t)P, 0);
    for (int j = 0; j < P; ++j) {
        const int cap = j > 0 ? j - 1 : 0;
        int v = 0;
        if (kind == 0) v = j - P / 2;
        else if (kind == 1) v = j - 2;
        else if (kind == 2) v = cap;
        else if (kind == 3) v = j - (P / 2 > 1 ? P / 2 : 1);
        else v = j < P / 2 ? 0 : P / 2 - 1;
        f[(size_t)j] = v < 0 ? 0 : (v > cap ? cap : v);
    }
    return f;
}

static void one_case(int B, int P, int kind, int workers, int split)
{
    setenv("PSOAP_SKY_SPLIT", split ? "1" : "0", 1);
    const std::vector<int> first = envelope(P, kind);
    long long n_tasks = 0, n_slots = 0, n_ctrs = 0;
    if (psoap_dag_plan_sky(B, P, first.data(), workers, nullptr, 0, &n_tasks, nullptr, nullptr, nullptr)) return fail("count call", B, P, kind, split);
    std::unique_ptr<DagTask[]> tasks(new DagTask[(size_t)n_tasks]());      // exactly n_tasks records
    unsigned int qf[9];
    if (psoap_dag_plan_sky(B, P, first.data(), workers, tasks.get(), n_tasks, &n_tasks, &n_slots, &n_ctrs, qf))
        return fail("list call", B, P, kind, split);
    // PARTs ahead of their final, their ranges tiling [first[j], q); slots and counters inside the counts
    // (an all-zero envelope gives the dense list, in whatever scheme the planner picks: hashed, not looked into)
    bool any = false;
    for (int v : first) any = any || v > 0;
    std::map<std::tuple<int, int, int>, int> pos;
    for (long long t = 0; any && t < n_tasks; ++t) {
        const DagTask& k = tasks[(size_t)t];
        const auto key = std::make_tuple((int)k.b, (int)k.q, (int)k.j);
        if (k.b >= B || k.q > k.j || k.j >= P || first[k.j] > k.q) return fail("a task outside the envelope", B, P, kind, split);
        if (!pos.count(key)) pos[key] = first[k.j];
        if (pos[key] < 0) return fail("a task behind its tile's final", B, P, kind, split);
        if (k.pa != pos[key] || k.pb < k.pa || k.pb > k.q) return fail("a range out of turn", B, P, kind, split);
        const bool part = (k.type & DAG_TYPE_MASK) == DAG_PART;
        if (part && (k.pb == k.pa || k.slot >= n_slots || k.ctr >= n_ctrs)) return fail("a PART's range, slot or counter", B, P, kind, split);
        if (!part && k.S > 1 && ((k.ctr & DAG_CTR_MASK) >= n_ctrs || k.slot + (k.S - 1u) > n_slots)) return fail("a final's slots or counter", B, P, kind, split);
        if (!part && k.pb != k.q) return fail("a final that stops short of its row", B, P, kind, split);
        pos[key] = part ? k.pb : -1;
    }
    long long tiles = 0;
    for (int j = 0; j < P; ++j) tiles += j + 1 - first[(size_t)j];
    if (any && (long long)pos.size() != tiles * B) return fail("tiles missing", B, P, kind, split);
    for (const auto& kv : pos)
        if (kv.second != -1) return fail("a tile without its final", B, P, kind, split);
    printf("plan_sky B=%d P=%d kind=%d workers=%d split=%d : n_tasks=%lld n_slots=%lld n_ctrs=%lld queue_first=%016llx tasks=%016llx\n", B, P,
           kind, workers, split, n_tasks, n_slots, n_ctrs, fnv1a(qf, sizeof qf), fnv1a(tasks.get(), sizeof(DagTask) * (size_t)n_tasks));
}

int main()
{
    for (int P : {2, 3, 10, 16, 47})
        for (int B : {2, 9, 16, 32}) {
            if (B * P * P > 40000) continue;
            for (int kind = 0; kind < 5; ++kind)
                for (int workers : {7, 512})
                    for (int split : {1, 0}) one_case(B, P, kind, workers, split);
        }
    return g_failed;
}
