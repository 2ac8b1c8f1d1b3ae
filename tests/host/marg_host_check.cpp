// marg_host_check.cpp -- the pure-host part of the continuum-marginalised likelihood (psoap_amd/csrc/marg_plan.hpp) built by a
// host compiler alone, with AddressSanitizer and UBSan (tests/test_marg_host.py): argument validation, the column layout, the
// first non-zero block row of every appended tile column, their order in the workspace, the Gram tiles and the abscissa map.
// One line per case on stdout -- the plan spelled out, for the test to compare with its own restatement -- and a non-zero
// exit status when an invariant does not hold.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../psoap_amd/csrc/marg_plan.hpp"

using namespace psoap;

static int failures = 0;

#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// epoch index from runs (id, pixels) in flattened order
static std::vector<int32_t> from_runs(const std::vector<std::pair<int, int>>& runs)
{
    std::vector<int32_t> ep;
    for (const auto& r : runs) ep.insert(ep.end(), (size_t)r.second, (int32_t)r.first);
    return ep;
}

// abscissae: pixel i of a run at 8.5 + 1e-5 i (every run starts again: epochs overlap in wavelength as real ones do)
static std::vector<double> abscissae(const std::vector<std::pair<int, int>>& runs)
{
    std::vector<double> x;
    for (const auto& r : runs)
        for (int i = 0; i < r.second; ++i) x.push_back(8.5 + 1e-5 * i);
    return x;
}

static void invariants(const MargPlan& pl, const double* x, const int32_t* epoch)
{
    EXPECT(pl.q == pl.n_epochs * (pl.order + 1) && pl.Q == (pl.q + NB - 1) / NB && pl.P == (pl.N + NB - 1) / NB);
    // every non-zero of H lies at or below the first row of its tile column, and the first row is attained
    std::vector<int> lowest((size_t)pl.Q, pl.P);
    for (int i = 0; i < pl.N; ++i)
        for (int k = 0; k <= pl.order; ++k) {
            const int t = (pl.col0[(size_t)epoch[i]] + k) / NB;
            EXPECT(i / NB >= pl.first[(size_t)t]);
            lowest[(size_t)t] = std::min(lowest[(size_t)t], i / NB);
        }
    for (int t = 0; t < pl.Q; ++t) EXPECT(lowest[(size_t)t] == pl.first[(size_t)t]);
    // the slots: a permutation in ascending order of the first rows, whose prefixes are the active sets
    std::vector<int> seen((size_t)pl.Q, 0);
    for (int s = 0; s < pl.Q; ++s) {
        EXPECT(pl.slot[(size_t)pl.column[(size_t)s]] == s);
        seen[(size_t)pl.column[(size_t)s]]++;
        EXPECT(s == 0 || pl.first[(size_t)pl.column[(size_t)s - 1]] <= pl.first[(size_t)pl.column[(size_t)s]]);
    }
    for (int t = 0; t < pl.Q; ++t) EXPECT(seen[(size_t)t] == 1);
    for (int p = 0; p < pl.P; ++p)
        for (int s = 0; s < pl.Q; ++s) EXPECT((s < pl.active[(size_t)p]) == (pl.first[(size_t)pl.column[(size_t)s]] <= p));
    // the Gram tiles: every (ti <= tj) once, row-major, K loop from the later of the two first rows
    EXPECT((int)pl.tiles.size() == pl.Q * (pl.Q + 1) / 2);
    size_t k = 0;
    for (int ti = 0; ti < pl.Q; ++ti)
        for (int tj = ti; tj < pl.Q; ++tj, ++k) {
            const MargTile& g = pl.tiles[k];
            EXPECT(g.ti == ti && g.tj == tj && g.si == pl.slot[(size_t)ti] && g.sj == pl.slot[(size_t)tj]);
            EXPECT(g.k0 == NB * std::max(pl.first[(size_t)ti], pl.first[(size_t)tj]) && g.k0 <= NB * pl.P);
        }
    // the abscissa map sends every epoch onto [-1, 1], its ends onto the ends
    for (int e = 0; e < pl.n_epochs; ++e) {
        double lo = 2.0, hi = -2.0;
        for (int i = pl.start[(size_t)e]; i < pl.start[(size_t)e] + pl.count[(size_t)e]; ++i) {
            const double u = pl.off[(size_t)e] + pl.scl[(size_t)e] * x[i];
            lo = std::min(lo, u), hi = std::max(hi, u);
        }
        if (pl.count[(size_t)e] == 0) continue;
        if (pl.scl[(size_t)e] == 0.0) EXPECT(lo == 0.0 && hi == 0.0 && pl.off[(size_t)e] == 0.0);
        else EXPECT(fabs(lo + 1.0) < 1e-9 && fabs(hi - 1.0) < 1e-9);
    }
}

static void show(const char* name, const std::vector<std::pair<int, int>>& runs, int n_epochs, int order, const double* sd = nullptr)
{
    const std::vector<int32_t> ep = from_runs(runs);
    const std::vector<double> x = abscissae(runs);
    const int N = (int)ep.size();
    std::vector<double> ones((size_t)(order < 0 ? 1 : order + 1), 1.0);
    MargPlan pl;
    const char* why = marg_plan(x.data(), ep.data(), N, n_epochs, order, sd ? sd : ones.data(), pl);
    if (why) {
        printf("%s N=%d n_epochs=%d order=%d : refused: %s\n", name, N, n_epochs, order, why);
        return;
    }
    invariants(pl, x.data(), ep.data());
    std::string f, a, t, m;
    char buf[160];
    for (int k = 0; k < pl.Q; ++k) {
        snprintf(buf, sizeof buf, " (%d,%d)", pl.first[(size_t)k], pl.slot[(size_t)k]);
        f += buf;
    }
    for (int p = 0; p < pl.P; ++p) {
        snprintf(buf, sizeof buf, " %d", pl.active[(size_t)p]);
        a += buf;
    }
    for (const MargTile& g : pl.tiles) {
        snprintf(buf, sizeof buf, " (%d,%d,%d,%d,%d)", g.ti, g.tj, g.si, g.sj, g.k0);
        t += buf;
    }
    for (int e = 0; e < pl.n_epochs; ++e) {
        snprintf(buf, sizeof buf, " (%d,%d,%d,%.17g,%.17g)", pl.col0[(size_t)e], pl.start[(size_t)e], pl.count[(size_t)e], pl.off[(size_t)e],
                 pl.scl[(size_t)e]);
        m += buf;
    }
    printf("%s N=%d n_epochs=%d order=%d : q %d Q %d | first%s | active%s | tiles%s | epochs%s\n", name, N, n_epochs, order, pl.q, pl.Q,
           f.c_str(), a.c_str(), t.c_str(), m.c_str());
}

int main()
{
    // the cases of tests/marg_reference.py
    show("a", {{0, 25}, {1, 25}, {2, 25}, {3, 25}}, 4, 1);
    show("b", {{0, 64}, {1, 64}}, 2, 0);
    show("c", {{0, 43}, {1, 43}, {2, 43}}, 3, 2);
    show("d", {{0, 128}, {1, 128}, {2, 128}}, 3, 3);
    show("e", {{2, 120}, {0, 100}, {3, 80}}, 4, 1);
    {
        std::vector<std::pair<int, int>> runs;
        for (int e = 0; e < 26; ++e) runs.push_back({e, 12});
        show("f", runs, 26, 4);
    }
    // two tile columns whose first rows are NOT monotone in the column index: epochs 0 .. 7 (columns 0 .. 127) lie last
    {
        std::vector<std::pair<int, int>> runs;
        for (int e = 8; e < 12; ++e) runs.push_back({e, 100});
        for (int e = 0; e < 8; ++e) runs.push_back({e, 50});
        show("shuffled", runs, 12, 15);
    }
    // a tile column whose epochs are all empty, and a one-pixel epoch
    show("hollow", {{0, 200}, {20, 1}}, 21, 7);
    show("single", {{0, 1}}, 1, 0);
    // refused
    show("order-", {{0, 10}}, 1, -1);
    show("order+", {{0, 10}}, 1, 16);
    show("wide", {{0, 10}}, 257, 3);
    {
        const double sd[2] = {1.0, 0.0};
        show("sd0", {{0, 10}}, 1, 1, sd);
    }
    {
        const double sd[2] = {NAN, 1.0};
        show("sdnan", {{0, 10}}, 1, 1, sd);
    }
    {
        const double sd[1] = {INFINITY};
        show("sdinf", {{0, 10}}, 1, 0, sd);
    }
    show("split", {{0, 10}, {1, 10}, {0, 1}}, 2, 1);
    show("range", {{0, 10}, {2, 10}}, 2, 1);
    show("negative", {{0, 10}, {-1, 1}}, 2, 1);
    show("none", {{0, 10}}, 0, 1);
    if (failures) {
        fprintf(stderr, "%d invariant(s) failed\n", failures);
        return 1;
    }
    return 0;
}
