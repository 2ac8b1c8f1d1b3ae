// sky_fine_host_check.cpp -- the host twin of the row-granular clip (psoap_sky_clip16, psoap_amd/csrc/plan_abi.hpp) beside
// psoap_sky_clip as a stand-alone host program: no HIP header, no HIP library.  tests/test_sky_fine_host.py builds it with
// AddressSanitizer and UBSan and runs it; every output buffer has exactly the reported size, so an overrun is a sanitizer
// report.  One line per case: the entry point, its parameters, " : ", the winning candidate, the stage or unit count and
// the FNV-1a hash of the rows -- the test makes the same calls into libpsoap_gp.so and expects the same lines.
#include <stdio.h>

#include <memory>

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

// Seeded ln-wavelength grids (splitmix64; every operation below is one IEEE double operation, so the test's Python
// restatement gives the same bits): an ascending base grid of `span` in all with a seeded jitter of a fifth of a pixel,
// component k shifted by an epoch's velocity (pixel i belongs to epoch i mod 3), walker b by a little more and with a
// shorter length scale.  kind 0: as said; 1: every run of eight pixels shares one base value (exact key ties); 2: kind 0
// with a NaN in the first walker's first component (and, for B > 1, in the second walker's last).
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
    const double step = 4e-6;      // 1.2 km/s per pixel
    for (int i = 0; i < N; ++i) {
        const u64 u = splitmix(s);
        const double unit = (double)(u >> 11) / 9007199254740992.0;
        const int at = kind == 1 ? i / 8 * 8 : i;
        base[i] = 8.5 + step * (double)at;
        if (kind != 1) base[i] = base[i] + 0.2 * step * unit;
    }
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < c; ++k) {
            for (int i = 0; i < N; ++i) {
                double x = base[i] + 2e-5 * k * (double)(i % 3 - 1);
                x = x + 1e-6 * b;
                lwl[((size_t)b * c + k) * N + i] = x;
            }
            gp[(size_t)b * 2 * c + 2 * k] = 1.0 + 0.25 * k;
            gp[(size_t)b * 2 * c + 2 * k + 1] = 6.0 + k - 1.5 * b;
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
        Exact<int> rows((size_t)B * P);
        long long units = -9;
        int cand = -9;
        check(psoap_sky_clip(c, N, B, lwl.data(), gp.data(), rows.p.get(), &units, &cand), "psoap_sky_clip");
        printf("sky_clip c=%d B=%d N=%d kind=%d seed=%llu : cand=%d units=%lld first_b=%016llx\n", c, B, N, kind, seed, cand, units,
               rows.hash());
    }
    {
        Exact<int> rows((size_t)B * P);
        long long stages = -9;
        int cand = -9;
        check(psoap_sky_clip16(c, N, B, lwl.data(), gp.data(), rows.p.get(), &stages, &cand), "psoap_sky_clip16");
        printf("sky_clip16 c=%d B=%d N=%d kind=%d seed=%llu : cand=%d stages=%lld first16_b=%016llx\n", c, B, N, kind, seed, cand,
               stages, rows.hash());
        // (every output may be null)
        check(psoap_sky_clip16(c, N, B, lwl.data(), gp.data(), nullptr, nullptr, nullptr), "psoap_sky_clip16");
    }
}

int main()
{
    u64 seed = 1;
    for (int c : {1, 2, 3})
        for (int B : {1, 3})
            for (int N : {1, 15, 127, 129, 300, 1000, 1041})
                for (int kind : {0, 1, 2}) case_sky(c, B, N, kind, seed++);
    return g_failed;
}
