// loo_host_check.cpp -- the pure-host part of leave-one-out cross-validation (psoap_amd/csrc/loo_plan.hpp) built by a host
// compiler alone, with AddressSanitizer and UBSan (tests/test_loo_host.py): the contiguity check, the packed-block offsets
// and the band tile list from the epoch of every pixel.  One line per case on stdout -- the layout spelled out, for the test
// to compare with its own restatement -- and a non-zero exit status when an invariant does not hold.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../psoap_amd/csrc/loo_plan.hpp"

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

static void invariants(const LooLayout& lay)
{
    const int P = round_up(lay.N, NB) / NB;
    long long off = 0, rhs = 0, wt = 0;
    int covered = 0;
    for (size_t k = 0; k < lay.blocks.size(); ++k) {
        const LooBlock& b = lay.blocks[k];
        EXPECT(b.count >= 1 && b.side == round_up(b.count, NB) && b.start >= 0 && b.start + b.count <= lay.N);
        EXPECT(b.offset == off && b.rhs == rhs && b.wt == wt);
        EXPECT(k == 0 || lay.blocks[k - 1].side <= b.side);
        EXPECT(lay.epoch_block[(size_t)b.epoch] == (int)k && lay.start[(size_t)b.epoch] == b.start && lay.count[(size_t)b.epoch] == b.count);
        for (int i = b.start; i < b.start + b.count; ++i) EXPECT(lay.pixel_block[(size_t)i] == (int)k);
        off += (long long)b.side * b.side;
        rhs += b.side;
        wt += (long long)(b.side / NB) * NB * NB;
        covered += b.count;
    }
    EXPECT(covered == lay.N && off == lay.block_doubles && rhs == lay.rhs_doubles && wt == lay.wt_doubles);
    int first = 0;
    for (const LooGroup& g : lay.groups) {
        EXPECT(g.first == first && g.count >= 1);
        for (int k = g.first; k < g.first + g.count; ++k) EXPECT(lay.blocks[(size_t)k].side == g.side);
        first += g.count;
    }
    EXPECT(first == (int)lay.blocks.size());
    // every element of every epoch's diagonal block lies in a listed tile, every listed tile meets one, none is listed twice
    std::vector<int> listed((size_t)P * P, 0);
    for (const LooTile& t : lay.tiles) {
        EXPECT(0 <= t.ti && t.ti <= t.tj && t.tj < P);
        listed[(size_t)t.ti * P + t.tj]++;
    }
    std::vector<int> needed((size_t)P * P, 0);
    for (const LooBlock& b : lay.blocks)
        for (int i = b.start; i < b.start + b.count; ++i)
            for (int j = i; j < b.start + b.count; ++j) needed[(size_t)(i / NB) * P + j / NB] = 1;
    for (size_t k = 0; k < listed.size(); ++k) EXPECT(listed[k] == needed[k]);
    for (size_t k = 1; k < lay.tiles.size(); ++k)
        EXPECT(lay.tiles[k - 1].ti < lay.tiles[k].ti || (lay.tiles[k - 1].ti == lay.tiles[k].ti && lay.tiles[k - 1].tj < lay.tiles[k].tj));
}

static void show(const char* name, const int32_t* epoch, int N, int n_epochs)
{
    LooLayout lay;
    const char* why = loo_layout(epoch, N, n_epochs, lay);
    if (why) {
        printf("%s N=%d n_epochs=%d : refused: %s\n", name, N, n_epochs, why);
        return;
    }
    invariants(lay);
    std::string s;
    char buf[128];
    for (const LooBlock& b : lay.blocks) {
        snprintf(buf, sizeof buf, " (%d,%d,%d,%d,%lld,%lld,%lld)", b.epoch, b.start, b.count, b.side, b.offset, b.rhs, b.wt);
        s += buf;
    }
    std::string g;
    for (const LooGroup& q : lay.groups) {
        snprintf(buf, sizeof buf, " (%d,%d,%d)", q.side, q.first, q.count);
        g += buf;
    }
    std::string t;
    for (const LooTile& q : lay.tiles) {
        snprintf(buf, sizeof buf, " (%d,%d)", q.ti, q.tj);
        t += buf;
    }
    printf("%s N=%d n_epochs=%d : blocks%s | groups%s | tiles%s | doubles %lld %lld %lld\n", name, N, lay.n_epochs, s.c_str(), g.c_str(),
           t.c_str(), lay.block_doubles, lay.rhs_doubles, lay.wt_doubles);
}

int main()
{
    // the cases of tests/loo_reference.py
    {
        auto ep = from_runs({{0, 25}, {1, 25}, {2, 25}, {3, 25}});
        show("a", ep.data(), 100, 4);
    }
    {
        auto ep = from_runs({{0, 128}});
        show("b", ep.data(), 128, 1);
    }
    {
        auto ep = from_runs({{0, 128}, {1, 1}});
        show("c", ep.data(), 129, 2);
    }
    {
        auto ep = from_runs({{0, 128}, {1, 128}, {2, 128}});
        show("d", ep.data(), 384, 3);
    }
    {
        auto ep = from_runs({{0, 1}, {1, 299}, {3, 130}, {4, 270}});
        show("e", ep.data(), 700, 5);
    }
    {
        auto ep = from_runs({{2, 100}, {0, 100}, {1, 100}});
        show("f", ep.data(), 300, 3);
    }
    // no epoch index: one pseudo-epoch per tile
    show("null", nullptr, 700, 0);
    show("null", nullptr, 128, 0);
    // n_e = 1 for every pixel, and n_e = N
    {
        std::vector<int32_t> ep(130);
        for (int i = 0; i < 130; ++i) ep[(size_t)i] = 129 - i;
        show("ones", ep.data(), 130, 130);
    }
    {
        std::vector<int32_t> ep(1000, 0);
        show("whole", ep.data(), 1000, 1);
    }
    // refused layouts
    {
        auto ep = from_runs({{0, 10}, {1, 10}, {0, 1}});
        show("split", ep.data(), 21, 2);
    }
    {
        auto ep = from_runs({{0, 10}, {2, 10}});
        show("range", ep.data(), 20, 2);
    }
    {
        auto ep = from_runs({{0, 10}, {-1, 1}});
        show("negative", ep.data(), 11, 2);
    }
    {
        auto ep = from_runs({{0, 10}});
        show("none", ep.data(), 10, 0);
    }
    if (failures) {
        fprintf(stderr, "%d invariant(s) failed\n", failures);
        return 1;
    }
    return 0;
}
