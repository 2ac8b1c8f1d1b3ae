// marg_grad_host_check.cpp -- the pure-host part of the gradient of the continuum-marginalised likelihood
// (psoap_amd/csrc/marg_grad_plan.hpp) built by a host compiler alone, with AddressSanitizer and UBSan
// (tests/test_marg_grad_host.py): the layout of [K | I | Ht], every appended tile column's first row, the launches of every
// block row, the group size and the argument validation.  One line per case on stdout -- the plan spelled out, for the test to
// compare with its own restatement -- and a non-zero exit status when an invariant does not hold.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <vector>

#include "../../psoap_amd/csrc/marg_grad_plan.hpp"

using namespace psoap;

static int failures = 0;

#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

typedef std::vector<std::pair<int, int>> Runs;

static void invariants(const MargPlan& pl, const MargGradPlan& g, const std::vector<int32_t>& epoch)
{
    const int P = pl.P, Q = pl.Q;
    EXPECT(g.P == P && g.Q == Q && g.N == pl.N && g.ld == NB * (2 * P + Q) && g.tile_I == P && g.tile_H == 2 * P);
    EXPECT((int)g.tile.size() == P + Q && (int)g.first.size() == P + Q && (int)g.rows.size() == P);
    EXPECT(marg_grad_matrix_doubles(NB * P, Q) == (size_t)NB * P * (size_t)g.ld);
    // every appended column's first row: I_j is zero above block row j; a tile column of H above the first pixel of its
    // first epoch in row order (found here from the pixels themselves)
    std::vector<int> lowest((size_t)Q, P);
    for (int i = 0; i < pl.N; ++i)
        for (int k = 0; k <= pl.order; ++k) {
            const int t = (pl.col0[(size_t)epoch[(size_t)i]] + k) / NB;
            lowest[(size_t)t] = std::min(lowest[(size_t)t], i / NB);
        }
    for (int j = 0; j < P; ++j) EXPECT(g.first[(size_t)j] == j && g.tile[(size_t)j] == P + j);
    for (int t = 0; t < Q; ++t) EXPECT(g.first[(size_t)P + t] == lowest[(size_t)t] && g.tile[(size_t)P + t] == 2 * P + pl.slot[(size_t)t]);
    // the column map is a permutation of the appended tile columns P .. 2 P + Q - 1, inside the row
    std::set<int> seen(g.tile.begin(), g.tile.end());
    EXPECT((int)seen.size() == P + Q && *seen.begin() == P && *seen.rbegin() == 2 * P + Q - 1 && NB * (*seen.rbegin() + 1) == g.ld);
    // block row p: the active set -- K's tiles from p on and the appended columns whose first row is <= p -- is exactly what
    // the launches cover
    for (int p = 0; p < P; ++p) {
        const MargGradRow& r = g.rows[(size_t)p];
        std::set<int> active_solve, active_update;
        for (int j = p + 1; j < P; ++j) active_solve.insert(j);
        for (int j = p; j < P; ++j) active_update.insert(j);
        for (int a = 0; a < P + Q; ++a)
            if (g.first[(size_t)a] <= p) {
                active_solve.insert(g.tile[(size_t)a]);
                active_update.insert(g.tile[(size_t)a]);
            }
        std::set<int> solve;
        for (int x = 0; x < r.strip_k; ++x) solve.insert(p + 1 + x);
        for (int x = 0; x < r.strip_h; ++x) solve.insert(g.tile_H + x);
        EXPECT((int)solve.size() == r.strip_k + r.strip_h && solve == active_solve);
        if (p == 0) {
            EXPECT(r.update_k == 0 && r.update_h == 0);      // nothing above block row 0
            continue;
        }
        std::set<int> update;
        for (int x = 0; x < r.update_k + r.update_h; ++x) update.insert(marg_grad_update_tile(p, x, P));
        EXPECT((int)update.size() == r.update_k + r.update_h && update == active_update);
    }
}

static void show(const char* name, const Runs& runs, int n_epochs, int order)
{
    std::vector<int32_t> ep;
    std::vector<double> x;
    for (const auto& r : runs)
        for (int i = 0; i < r.second; ++i) {
            ep.push_back((int32_t)r.first);
            x.push_back(8.5 + 1e-5 * i);
        }
    const int N = (int)ep.size();
    std::vector<double> ones((size_t)order + 1, 1.0);
    MargPlan pl;
    const char* why = marg_plan(x.data(), ep.data(), N, n_epochs, order, ones.data(), pl);
    if (why) {
        fprintf(stderr, "%s: %s\n", name, why);
        ++failures;
        return;
    }
    MargGradPlan g;
    marg_grad_plan(pl, g);
    invariants(pl, g, ep);
    std::string cols, rows;
    char buf[96];
    for (int a = 0; a < g.P + g.Q; ++a) {
        snprintf(buf, sizeof buf, " (%d,%d)", g.tile[(size_t)a], g.first[(size_t)a]);
        cols += buf;
    }
    for (const MargGradRow& r : g.rows) {
        snprintf(buf, sizeof buf, " (%d,%d,%d,%d)", r.update_k, r.update_h, r.strip_k, r.strip_h);
        rows += buf;
    }
    printf("%s N=%d n_epochs=%d order=%d : ld %d | cols%s | rows%s\n", name, N, n_epochs, order, g.ld, cols.c_str(), rows.c_str());
}

static void refusal(const char* name, int B, int c, bool have, bool stale)
{
    const char* why = marg_grad_check(B, c, have, stale);
    printf("%s : %s\n", name, why ? why : "accepted");
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
        Runs runs;
        for (int e = 0; e < 26; ++e) runs.push_back({e, 12});
        show("f", runs, 26, 4);
    }
    // two tile columns of H whose first rows are NOT monotone in the column index: epochs 0 .. 7 (columns 0 .. 127) lie last
    {
        Runs runs;
        for (int e = 8; e < 12; ++e) runs.push_back({e, 100});
        for (int e = 0; e < 8; ++e) runs.push_back({e, 50});
        show("shuffled", runs, 12, 15);
    }
    // a tile column of H without a pixel: never active
    show("hollow", {{0, 200}, {20, 1}}, 21, 7);
    refusal("ok", 1, 2, true, false);
    refusal("B0", 0, 2, true, false);
    refusal("c0", 3, 0, true, false);
    refusal("c4", 3, 4, true, false);
    refusal("unset", 3, 2, false, false);
    refusal("stale", 3, 2, true, true);
    // groups: the cap of 8, the 1 GiB bound with the Ht columns counted, never fewer than one
    EXPECT(marg_grad_group_size(3, 384, 1) == 3 && marg_grad_group_size(10, 384, 1) == MARG_GRAD_GROUP_MAX);
    EXPECT(marg_grad_group_size(10, 6016, 1) == 1 && marg_grad_group_size(10, 4096, 1) == 3 && marg_grad_group_size(10, 4096, 8) == 3);
    EXPECT(marg_grad_group_size(10, 5760, 1) == 2 && marg_grad_group_size(10, 5760, 8) == 1);      // where grad_group_size gives 2
    EXPECT(marg_grad_group_size(1, 40960, 8) == 1);
    if (failures) {
        fprintf(stderr, "%d invariant(s) failed\n", failures);
        return 1;
    }
    return 0;
}
