// marg_predict_host_check.cpp -- the pure-host part of the prediction under the marginalised continuum
// (psoap_amd/csrc/marg_predict_plan.hpp) built by a host compiler alone, with AddressSanitizer and UBSan
// (tests/test_marg_predict_host.py): the layout of [K | Cx^T | Ht], every appended tile column's first row, the launches
// of every block row of both factorisations, the tiles of the Gram launch and of Sigma, the workspace bytes and the
// argument validation.  One line per case on stdout -- the plan spelled out, for the test to compare with its own
// restatement -- and a non-zero exit status when an invariant does not hold.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../psoap_amd/csrc/marg_predict_plan.hpp"

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

static void invariants(const MargPlan& pl, const MargPredictPlan& g, const std::vector<int32_t>& epoch)
{
    const int P = pl.P, Q = pl.Q, Rt = g.Rt;
    EXPECT(g.P == P && g.Q == Q && g.N == pl.N && g.R == (g.mode == 0 ? g.c * g.M : g.M) && Rt == (g.R + NB - 1) / NB);
    EXPECT(g.ld == NB * (P + Rt + Q) && g.tile_C == P && g.tile_H == P + Rt && g.S == NB * Q && g.ldm == NB * (Q + Rt));
    EXPECT((int)g.tile.size() == Rt + Q && (int)g.first.size() == Rt + Q && (int)g.rows.size() == P && (int)g.mrows.size() == Q);
    // every appended column's first row: Cx^T is dense; a tile column of H is zero above the first pixel of its first epoch
    // in row order (found here from the pixels themselves)
    std::vector<int> lowest((size_t)Q, P);
    for (int i = 0; i < pl.N; ++i)
        for (int k = 0; k <= pl.order; ++k) {
            const int t = (pl.col0[(size_t)epoch[(size_t)i]] + k) / NB;
            lowest[(size_t)t] = std::min(lowest[(size_t)t], i / NB);
        }
    for (int j = 0; j < Rt; ++j) EXPECT(g.first[(size_t)j] == 0 && g.tile[(size_t)j] == P + j);
    for (int t = 0; t < Q; ++t) EXPECT(g.first[(size_t)Rt + t] == lowest[(size_t)t] && g.tile[(size_t)Rt + t] == P + Rt + pl.slot[(size_t)t]);
    // the column map is a permutation of the appended tile columns P .. P + Rt + Q - 1, inside the row
    std::set<int> seen(g.tile.begin(), g.tile.end());
    EXPECT((int)seen.size() == Rt + Q && *seen.begin() == P && *seen.rbegin() == P + Rt + Q - 1 && NB * (*seen.rbegin() + 1) == g.ld);
    // block row p: the active set -- K's tiles from p on and the appended columns whose first row is <= p -- is exactly the
    // one contiguous range the two launches cover
    for (int p = 0; p < P; ++p) {
        const MargPredictRow& r = g.rows[(size_t)p];
        std::set<int> active;
        for (int j = p; j < P; ++j) active.insert(j);
        for (int a = 0; a < Rt + Q; ++a)
            if (g.first[(size_t)a] <= p) active.insert(g.tile[(size_t)a]);
        std::set<int> solve, update;
        for (int x = 0; x < r.strip; ++x) solve.insert(p + 1 + x);
        for (int x = 0; x < r.update; ++x) update.insert(p + x);
        active.erase(p);
        EXPECT((int)solve.size() == r.strip && solve == active);
        EXPECT(*solve.rbegin() < P + Rt + Q);
        active.insert(p);
        if (p == 0) EXPECT(r.update == 0);      // nothing above block row 0
        else EXPECT(update == active);
    }
    // the Gram launch: every upper tile of M once, every tile of G once, the K loop from the lower of the two first rows
    EXPECT((int)g.gram.size() == Q * (Q + 1) / 2 + Q * Rt);
    std::set<std::pair<int, int>> written;
    for (const MargPredictTile& t : g.gram) {
        EXPECT(t.row >= 0 && t.row < Q && t.col >= t.row && t.col < Q + Rt);
        EXPECT(written.insert({t.row, t.col}).second);
        EXPECT(t.a == P + Rt + pl.slot[(size_t)t.row] && t.k0 % NB == 0 && t.k0 >= 0 && t.k0 <= NB * P);
        if (t.col < Q) {
            EXPECT(t.b == P + Rt + pl.slot[(size_t)t.col] && t.diag == (t.row == t.col ? 1 : 0));
            EXPECT(t.k0 == NB * std::max(lowest[(size_t)t.row], lowest[(size_t)t.col]));
        } else {
            EXPECT(t.b == P + (t.col - Q) && t.diag == 0 && t.k0 == NB * lowest[(size_t)t.row]);
        }
        EXPECT(NB * (t.a + 1) <= g.ld && NB * (t.b + 1) <= g.ld);
    }
    // block row p of [M | G]: M's tiles from p on and all of G
    for (int p = 0; p < Q; ++p) {
        const MargPredictRow& r = g.mrows[(size_t)p];
        EXPECT(r.strip == Q - p - 1 + Rt && r.update == (p > 0 ? Q - p + Rt : 0) && NB * (p + 1 + r.strip) == g.ldm);
    }
    EXPECT(g.St == Rt && g.sigma_tiles == Rt * (Rt + 1) / 2);
    EXPECT(marg_predict_k_bytes(g) == sizeof(double) * (size_t)NB * P * (size_t)g.ld);
    EXPECT(marg_predict_m_bytes(g) == sizeof(double) * (size_t)g.S * (size_t)g.ldm);
    EXPECT(marg_predict_sigma_bytes(g) == sizeof(double) * (size_t)NB * Rt * (size_t)NB * Rt);
    EXPECT(marg_predict_flops(g, true, false) > marg_predict_flops(g, false, true) &&
           marg_predict_flops(g, false, true) > marg_predict_flops(g, false, false));
}

static void show(const char* name, const Runs& runs, int n_epochs, int order, int mode, int c, int M)
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
    if (!why) why = marg_predict_check(mode, c, M, true, false);
    if (why) {
        fprintf(stderr, "%s: %s\n", name, why);
        ++failures;
        return;
    }
    MargPredictPlan g;
    marg_predict_plan(pl, mode, c, M, g);
    invariants(pl, g, ep);
    std::string cols, rows, mrows, gram;
    char buf[128];
    for (size_t a = 0; a < g.tile.size(); ++a) {
        snprintf(buf, sizeof buf, " (%d,%d)", g.tile[a], g.first[a]);
        cols += buf;
    }
    for (const MargPredictRow& r : g.rows) {
        snprintf(buf, sizeof buf, " (%d,%d)", r.update, r.strip);
        rows += buf;
    }
    for (const MargPredictRow& r : g.mrows) {
        snprintf(buf, sizeof buf, " (%d,%d)", r.update, r.strip);
        mrows += buf;
    }
    for (const MargPredictTile& t : g.gram) {
        snprintf(buf, sizeof buf, " (%d,%d,%d,%d,%d,%d)", t.row, t.col, t.a, t.b, t.k0, t.diag);
        gram += buf;
    }
    printf("%s N=%d n_epochs=%d order=%d mode=%d c=%d M=%d : ld %d | cols%s | rows%s | ldm %d | mrows%s | gram%s | sigma %d %d | "
           "bytes %zu %zu %zu\n",
           name, N, n_epochs, order, mode, c, M, g.ld, cols.c_str(), rows.c_str(), g.ldm, mrows.c_str(), gram.c_str(), g.St,
           g.sigma_tiles, marg_predict_k_bytes(g), marg_predict_m_bytes(g), marg_predict_sigma_bytes(g));
}

static void refusal(const char* name, int mode, int c, int M, bool have, bool stale)
{
    const char* why = marg_predict_check(mode, c, M, have, stale);
    printf("%s : %s\n", name, why ? why : "accepted");
}

int main()
{
    // the cases of tests/marg_predict_reference.py
    show("a", {{0, 25}, {1, 25}, {2, 25}, {3, 25}}, 4, 1, 0, 2, 50);
    show("a1", {{0, 25}, {1, 25}, {2, 25}, {3, 25}}, 4, 1, 1, 2, 130);
    show("b", {{0, 64}, {1, 64}}, 2, 0, 2, 1, 128);
    show("c", {{0, 43}, {1, 43}, {2, 43}}, 3, 2, 0, 2, 65);
    show("d", {{0, 128}, {1, 128}, {2, 128}}, 3, 3, 2, 1, 129);
    show("e", {{2, 120}, {0, 100}, {3, 80}}, 4, 1, 0, 3, 43);
    {
        Runs runs;
        for (int e = 0; e < 26; ++e) runs.push_back({e, 12});
        show("f", runs, 26, 4, 0, 2, 100);
    }
    // two tile columns of H whose first rows are NOT monotone in the column index: epochs 0 .. 7 (columns 0 .. 127) lie last
    {
        Runs runs;
        for (int e = 8; e < 12; ++e) runs.push_back({e, 100});
        for (int e = 0; e < 8; ++e) runs.push_back({e, 50});
        show("shuffled", runs, 12, 15, 0, 2, 100);
    }
    // epochs 1 .. 19 without a pixel: the second tile column of H starts at the chunk's last pixel, in the last block row
    show("hollow", {{0, 200}, {20, 1}}, 21, 7, 0, 3, 50);
    refusal("ok", 0, 2, 10, true, false);
    refusal("ok-sum", 1, 2, 10, true, false);
    refusal("ok-f", 2, 1, 10, true, false);
    refusal("mode3", 3, 2, 10, true, false);
    refusal("c4", 0, 4, 10, true, false);
    refusal("M0", 0, 2, 0, true, false);
    refusal("f-c2", 2, 2, 10, true, false);
    refusal("sum-c3", 1, 3, 10, true, false);
    refusal("sum-c1", 1, 1, 10, true, false);
    refusal("comp-c1", 0, 1, 10, true, false);
    refusal("unset", 0, 2, 10, false, false);
    refusal("stale", 0, 2, 10, true, true);
    if (failures) {
        fprintf(stderr, "%d invariant(s) failed\n", failures);
        return 1;
    }
    return 0;
}
