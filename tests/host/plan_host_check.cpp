// plan_host_check.cpp -- the planner and the pure-host entry points of the C ABI (psoap_amd/csrc/plan_abi.hpp) as a
// stand-alone host program: no HIP header, no HIP library.  tests/test_plan_host.py builds it with AddressSanitizer and
// UBSan and runs it; every output buffer has exactly the reported size, so an overrun is a sanitizer report.  One line per
// case: the entry point, its parameters, " : ", and per output a count or the FNV-1a hash of the array's bytes -- the test
// makes the same calls into libpsoap_gp.so and expects the same lines.
#include <stdio.h>

#include <memory>
#include <string>

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
template <class T>
static u64 fnv1a(const std::vector<T>& v) { return fnv1a(v.data(), sizeof(T) * v.size()); }

static int g_failed = 0;
static void check(int rc, const char* what)
{
    if (rc == 0) return;
    fprintf(stderr, "%s: returned %d (%s)\n", what, rc, psoap_last_error());
    g_failed = 1;
}

// heap buffers of exactly n elements (operator new[]: redzones on both sides)
template <class T>
struct Exact {
    std::unique_ptr<T[]> p;
    size_t n;
    explicit Exact(size_t n_) : p(new T[n_]()), n(n_) {}
    u64 hash() const { return fnv1a(p.get(), sizeof(T) * n); }
};

static std::string join(const std::vector<int>& v)
{
    std::string s;
    for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + std::to_string(v[i]);
    return s;
}

// ---- the task lists ---------------------------------------------------------------------------------
struct Counts {
    long long n_tasks = 0, n_slots = 0, n_ctrs = 0;
};
static void print_list(const Counts& c, const unsigned int* qf, const Exact<DagTask>& tasks)
{
    printf("n_tasks=%lld n_slots=%lld n_ctrs=%lld", c.n_tasks, c.n_slots, c.n_ctrs);
    if (qf) printf(" queue_first=%016llx", fnv1a(qf, sizeof(unsigned int) * 9));
    printf(" tasks=%016llx\n", tasks.hash());
}

static void case_plan(int B, int P, int workers)
{
    Counts c;
    check(psoap_dag_plan(B, P, workers, nullptr, 0, &c.n_tasks, nullptr, nullptr, nullptr), "psoap_dag_plan");
    Exact<DagTask> tasks((size_t)c.n_tasks);
    unsigned int qf[9];
    check(psoap_dag_plan(B, P, workers, tasks.p.get(), c.n_tasks, &c.n_tasks, &c.n_slots, &c.n_ctrs, qf), "psoap_dag_plan");
    printf("plan B=%d P=%d workers=%d : ", B, P, workers);
    print_list(c, qf, tasks);
}

// band of width w: tile (q, j) exists iff j - q <= w (w = 0: the dense list)
static std::vector<int> band(int P, int w)
{
    std::vector<int> first((size_t)P, 0);
    for (int j = 0; j < P && w > 0; ++j) first[j] = j - w > 0 ? j - w : 0;
    return first;
}
static void case_plan_sky(int B, int P, int width, int workers)
{
    const std::vector<int> first = band(P, width);
    Counts c;
    check(psoap_dag_plan_sky(B, P, first.data(), workers, nullptr, 0, &c.n_tasks, nullptr, nullptr, nullptr), "psoap_dag_plan_sky");
    Exact<DagTask> tasks((size_t)c.n_tasks);
    unsigned int qf[9];
    check(psoap_dag_plan_sky(B, P, first.data(), workers, tasks.p.get(), c.n_tasks, &c.n_tasks, &c.n_slots, &c.n_ctrs, qf),
          "psoap_dag_plan_sky");
    printf("plan_sky B=%d P=%d width=%d workers=%d : ", B, P, width, workers);
    print_list(c, qf, tasks);
}

static void case_plan_multi(const std::vector<int>& Ps, int workers)
{
    const int B = (int)Ps.size();
    Counts c;
    check(psoap_dag_plan_multi(B, Ps.data(), workers, nullptr, 0, &c.n_tasks, nullptr, nullptr, nullptr), "psoap_dag_plan_multi");
    Exact<DagTask> tasks((size_t)c.n_tasks);
    unsigned int qf[9];
    check(psoap_dag_plan_multi(B, Ps.data(), workers, tasks.p.get(), c.n_tasks, &c.n_tasks, &c.n_slots, &c.n_ctrs, qf),
          "psoap_dag_plan_multi");
    printf("plan_multi Ps=%s workers=%d : ", join(Ps).c_str(), workers);
    print_list(c, qf, tasks);
}

static void case_plan_aug(int P, int Mt, int Ms, int workers, int scheme)
{
    Counts c;
    check(psoap_dag_plan_aug(P, Mt, Ms, workers, scheme, nullptr, 0, &c.n_tasks, nullptr, nullptr, nullptr), "psoap_dag_plan_aug");
    Exact<DagTask> tasks((size_t)c.n_tasks);
    unsigned int qf[9];
    check(psoap_dag_plan_aug(P, Mt, Ms, workers, scheme, tasks.p.get(), c.n_tasks, &c.n_tasks, &c.n_slots, &c.n_ctrs, qf),
          "psoap_dag_plan_aug");
    printf("plan_aug P=%d Mt=%d Ms=%d workers=%d scheme=%d : ", P, Mt, Ms, workers, scheme);
    print_list(c, qf, tasks);
}

static void case_stream_plan(int P, int lanes, int workers, int scheme)
{
    Counts c;
    int scheme_out = -9;
    check(psoap_stream_plan(P, lanes, workers, scheme, nullptr, 0, &c.n_tasks, nullptr, nullptr, nullptr), "psoap_stream_plan");
    Exact<DagTask> tasks((size_t)c.n_tasks);
    check(psoap_stream_plan(P, lanes, workers, scheme, tasks.p.get(), c.n_tasks, &c.n_tasks, &c.n_slots, &c.n_ctrs, &scheme_out),
          "psoap_stream_plan");
    printf("stream_plan P=%d lanes=%d workers=%d scheme=%d : scheme_out=%d ", P, lanes, workers, scheme, scheme_out);
    print_list(c, nullptr, tasks);
}

static void case_pick_workers(int B, int P, int Mt, int compute_units, int max_workers)
{
    const std::vector<int> Ps((size_t)B, P);
    int workers = -9;
    check(psoap_dag_pick_workers(B, Ps.data(), Mt, compute_units, max_workers, &workers), "psoap_dag_pick_workers");
    printf("pick_workers B=%d P=%d Mt=%d compute_units=%d max_workers=%d : workers=%d\n", B, P, Mt, compute_units, max_workers,
           workers);
}

// ---- the skyline twins ------------------------------------------------------------------------------
// Seeded ln-wavelength grids (splitmix64; every operation below is one IEEE double operation, so the test's Python
// restatement gives the same bits): one base grid per case, component k shifted by an epoch's velocity (pixel i belongs to
// epoch i mod 3), walker b by a little more.  kind 0: 53-bit uniform values; 1: sixteen distinct base values (exact key
// ties); 2: kind 0 with a NaN in the first walker's first component (and, for B > 1, in the second walker's last).
static u64 splitmix(u64& s)
{
    s += 0x9E3779B97F4A7C15ull;
    u64 z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static void sky_inputs(int c, int B, int N, int kind, u64 seed, std::vector<double>& lwl, std::vector<double>& gp)
{
    lwl.assign((size_t)B * c * N, 0.0);
    gp.assign((size_t)B * 2 * c, 0.0);
    std::vector<double> base((size_t)N);
    u64 s = seed;
    for (int i = 0; i < N; ++i) {
        const u64 u = splitmix(s);
        const double unit = kind == 1 ? (double)(u >> 60) / 16.0 : (double)(u >> 11) / 9007199254740992.0;
        base[i] = 8.5 + 0.1 * unit;
    }
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < c; ++k) {
            for (int i = 0; i < N; ++i) {
                double x = base[i] + 2e-3 * k * (double)(i % 3 - 1);
                x = x + 1e-4 * b;
                lwl[((size_t)b * c + k) * N + i] = x;
            }
            gp[(size_t)b * 2 * c + 2 * k] = 1.0 + 0.25 * k;
            gp[(size_t)b * 2 * c + 2 * k + 1] = 4.0 + k + 0.5 * b;
        }
    if (kind == 2) {
        const double nan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
        lwl[(size_t)N / 2] = nan;
        if (B > 1) lwl[((size_t)1 * c + (c - 1)) * N] = nan;
    }
}
static void case_sky(int c, int B, int N, int kind, u64 seed)
{
    std::vector<double> lwl, gp;
    sky_inputs(c, B, N, kind, seed, lwl, gp);
    const size_t P = (size_t)(N + 127) / 128;
    {
        Exact<int> first(P), perm((size_t)N);
        check(psoap_sky_first(c, N, B, lwl.data(), gp.data(), first.p.get(), perm.p.get()), "psoap_sky_first");
        printf("sky_first c=%d B=%d N=%d kind=%d seed=%llu : first=%016llx perm=%016llx\n", c, B, N, kind, seed, first.hash(),
               perm.hash());
    }
    {
        Exact<int> first(P), perm((size_t)N);
        int cand = -9;
        check(psoap_sky_order(c, N, B, lwl.data(), gp.data(), first.p.get(), perm.p.get(), &cand), "psoap_sky_order");
        printf("sky_order c=%d B=%d N=%d kind=%d seed=%llu : cand=%d first=%016llx perm=%016llx\n", c, B, N, kind, seed, cand,
               first.hash(), perm.hash());
    }
}

int main()
{
    const int Bs[] = {1, 2, 3, 8, 9, 32}, Pgrid[] = {1, 2, 3, 5, 16, 47, 64}, Ws[] = {1, 7, 256, 512}, schemes[] = {-1, 0, 1, 2};
    // (trimmed where the lists are largest -- B P^2 > 4096: two and more matrices of 47 or 64 block rows, 32 of 16; appended
    // columns: more than 72 block rows and column tiles together -- because the test hashes every list a second time, in
    // Python, at 8 MB/s)
    auto kept = [](int B, int P) { return B * P * P <= 4096; };
    for (int B : Bs)
        for (int P : Pgrid) {
            if (!kept(B, P)) continue;
            for (int w : Ws) case_plan(B, P, w);
            for (int Mt : {0, 8}) {
                case_pick_workers(B, P, Mt, 256, 512);
                case_pick_workers(B, P, Mt, 256, 256);
                case_pick_workers(B, P, Mt, 1, 7);
            }
        }
    for (const std::vector<int>& Ps : {std::vector<int>{1, 5, 16}, std::vector<int>{47, 2}, std::vector<int>{3, 3, 16, 1, 9, 2, 2, 5, 16, 7}})
        for (int w : Ws) case_plan_multi(Ps, w);
    for (int P : {3, 16, 47})
        for (int width : {0, 1, 2, P / 2})
            for (int B : {1, 9})
                for (int w : {7, 512}) case_plan_sky(B, P, width, w);
    for (int P : {1, 2, 7, 47, 64})
        for (int Mt : {1, 8, 24})
            for (int Ms : {0, 1, Mt}) {
                if (P + Mt > 72) continue;
                case_plan_aug(P, Mt, Ms, 512, -1);
                case_plan_aug(P, Mt, Ms, 7, 0);
                case_plan_aug(P, Mt, Ms, 256, 1);
            }
    for (int P : {1, 16, 64})
        for (int lanes : {1, 32, 64})
            for (int s : schemes) {
                case_stream_plan(P, lanes, 512, s);
                case_stream_plan(P, lanes, 7, s);
            }
    u64 seed = 1;
    for (int c : {1, 2, 3})
        for (int B : {1, 3})
            for (int N : {1, 127, 129, 300})
                for (int kind : {0, 1, 2}) case_sky(c, B, N, kind, seed++);
    return g_failed;
}
