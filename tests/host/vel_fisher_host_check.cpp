// vel_fisher_host_check.cpp -- the host-only header of the epoch-velocity Fisher information
// (psoap_amd/csrc/vel_fisher_plan.hpp) built by a host compiler alone, with AddressSanitizer and UBSan
// (tests/test_vel_fisher_host.py).  Prints the plan of a set of epoch indices -- equal, unequal, empty, straddling and
// unsorted epochs -- and what every refusal answers; checks the plan's own invariants on the way (exit status 1 with a
// message).
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <utility>
#include <vector>

#include "../../psoap_amd/csrc/vel_fisher_plan.hpp"

using namespace psoap;

static void fail(const char* what)
{
    fprintf(stderr, "vel_fisher_host_check: %s\n", what);
    exit(1);
}

static const char* say(const char* why) { return why ? why : "accepted"; }

static void tiles_once(const std::vector<VelTile>& tiles, int P, bool upper)
{
    std::set<std::pair<int, int>> seen;
    for (const VelTile& t : tiles) {
        if (t.ti < 0 || t.ti >= P || t.tj < 0 || t.tj >= P || (upper && t.tj < t.ti)) fail("a tile outside its range");
        if (!seen.insert(std::make_pair(t.ti, t.tj)).second) fail("a tile twice");
    }
    if ((long long)seen.size() != (upper ? (long long)P * (P + 1) / 2 : (long long)P * P)) fail("a tile is missing");
}

static void run(const char* name, int c, int n_epochs, const std::vector<int32_t>& ep)
{
    const int N = (int)ep.size();
    if (vel_fisher_check(c, N, n_epochs, ep.data())) fail("a valid case was refused");
    VelFisherPlan g;
    vel_fisher_plan(c, N, n_epochs, ep.data(), g);
    if (g.Npad % NB || g.Npad < N || g.Npad - N >= NB || g.P * NB != g.Npad) fail("Npad");
    if (g.n_pairs != c * (c + 1) / 2) fail("the pairs of components");
    tiles_once(g.tiles_all, g.P, false);
    tiles_once(g.tiles_upper, g.P, true);
    // every pixel sits in a slot of its own tile row that carries its epoch; rows beyond N in none
    if ((int)g.slot_of.size() != g.Npad || (int)g.slot_first.size() != g.P + 1) fail("the slot arrays' sizes");
    if (g.slot_first[0] != 0 || g.slot_first[(size_t)g.P] != g.S) fail("the slots' ends");
    for (int i = 0; i < g.Npad; ++i) {
        const int a = g.slot_of[(size_t)i];
        if (i >= N) {
            if (a != -1) fail("a row beyond N in a slot");
            continue;
        }
        if (a < g.slot_first[(size_t)(i / NB)] || a >= g.slot_first[(size_t)(i / NB) + 1]) fail("a pixel in another tile row's slot");
        if (g.slot_epoch[(size_t)a] != ep[(size_t)i] || g.slot_block[(size_t)a] != i / NB) fail("a pixel in another epoch's slot");
    }
    // within a tile row: ascending epochs, each once, none without a pixel
    std::vector<int> used((size_t)g.S, 0);
    for (int i = 0; i < N; ++i) used[(size_t)g.slot_of[(size_t)i]]++;
    int max_slots = 0;
    for (int q = 0; q < g.P; ++q) {
        const int n = g.slot_first[(size_t)q + 1] - g.slot_first[(size_t)q];
        if (n < 1 || n > NB) fail("the slots of a tile row");
        if (n > max_slots) max_slots = n;
        for (int a = g.slot_first[(size_t)q]; a < g.slot_first[(size_t)q + 1]; ++a) {
            if (!used[(size_t)a]) fail("a slot without a pixel");
            if (a > g.slot_first[(size_t)q] && g.slot_epoch[(size_t)a - 1] >= g.slot_epoch[(size_t)a]) fail("slots out of order");
        }
    }
    if (max_slots != g.max_slots) fail("max_slots");
    // the slots of every epoch: ascending, all of them, each slot once; the pixel counts
    long long pixels = 0;
    std::vector<int> hit((size_t)g.S, 0);
    for (int e = 0; e < n_epochs; ++e) {
        int count = 0;
        for (int k = g.epoch_ptr[(size_t)e]; k < g.epoch_ptr[(size_t)e + 1]; ++k) {
            const int a = g.epoch_slots[(size_t)k];
            if (g.slot_epoch[(size_t)a] != e || hit[(size_t)a]++) fail("an epoch's slot list");
            if (k > g.epoch_ptr[(size_t)e] && g.epoch_slots[(size_t)k - 1] >= a) fail("an epoch's slots out of order");
            count += used[(size_t)a];
        }
        if (count != g.epoch_count[(size_t)e]) fail("an epoch's pixel count");
        pixels += count;
    }
    if (pixels != N || g.epoch_ptr[(size_t)n_epochs] != g.S) fail("the epochs' slots do not cover the chunk");
    // the workspace
    const long long sq = (long long)g.Npad * g.Npad, T = (long long)c * n_epochs;
    if (g.square_doubles != (1 + 2 * c) * sq || g.part_doubles != (long long)g.n_pairs * g.S * g.S || g.out_doubles != T * T)
        fail("the workspace's doubles");
    const VelPlanOffsets o = vel_plan_offsets(g.Npad, g.P, g.S, n_epochs);
    if (o.end != g.Npad + (g.P + 1) + 2ll * g.S + (n_epochs + 1) + 2ll * g.P * g.P + (long long)g.P * (g.P + 1) || g.int_count != o.end)
        fail("the plan's ints");
    if (g.bytes != 8 * (g.square_doubles + g.part_doubles + g.out_doubles) + 4 * g.int_count) fail("the bytes");
    std::vector<int> packed;
    vel_plan_pack(g, packed);
    if ((long long)packed.size() != o.end) fail("the packed plan's size");
    for (int i = 0; i < g.Npad; ++i)
        if (packed[(size_t)(o.slot_of + i)] != g.slot_of[(size_t)i]) fail("the packed slots");
    for (size_t t = 0; t < g.tiles_upper.size(); ++t)
        if (packed[(size_t)o.tiles_upper + 2 * t] != g.tiles_upper[t].ti || packed[(size_t)o.tiles_upper + 2 * t + 1] != g.tiles_upper[t].tj)
            fail("the packed tiles");
    printf("plan %s c=%d N=%d E=%d : P %d S %d max %d | first", name, c, N, n_epochs, g.P, g.S, g.max_slots);
    for (int q = 0; q <= g.P; ++q) printf(" %d", g.slot_first[(size_t)q]);
    printf(" | epochs");
    for (int a = 0; a < g.S && a < 24; ++a) printf(" %d", g.slot_epoch[(size_t)a]);
    printf(" | tiles %zu %zu | bytes %lld\n", g.tiles_all.size(), g.tiles_upper.size(), g.bytes);
}

int main()
{
    std::vector<int32_t> ep;
    // six equal epochs of 50: an epoch straddles rows 128 and 256
    for (int i = 0; i < 300; ++i) ep.push_back(i / 50);
    run("equal", 2, 6, ep);
    // unequal epochs, one of them empty (3), two unused indices at the end
    ep.clear();
    const int sizes[] = {7, 121, 1, 0, 130, 41};
    for (int e = 0; e < 6; ++e)
        for (int k = 0; k < sizes[e]; ++k) ep.push_back(e);
    run("unequal", 3, 8, ep);
    // exactly one tile, one epoch
    ep.assign(128, 0);
    run("one", 1, 1, ep);
    // one tile plus one row
    ep.assign(129, 0);
    ep[128] = 1;
    run("plus-one", 2, 2, ep);
    // epoch ids descending along the chunk
    ep.clear();
    for (int i = 0; i < 260; ++i) ep.push_back(4 - i / 52);
    run("descending", 2, 5, ep);
    // no order at all: a fixed pseudo-random epoch per pixel, 140 epochs -- more than a tile row has rows
    ep.clear();
    unsigned s = 12345u;
    for (int i = 0; i < 400; ++i) {
        s = s * 1664525u + 1013904223u;
        ep.push_back((int32_t)((s >> 8) % 140u));
    }
    run("scattered", 3, 140, ep);
    printf("limits : NB %d VEL_MAX_EPOCHS %d\n", NB, VEL_MAX_EPOCHS);

    ep.assign(10, 0);
    ep[4] = 2;
    printf("check ok : %s\n", say(vel_fisher_check(2, 10, 3, ep.data())));
    printf("check c0 : %s\n", say(vel_fisher_check(0, 10, 3, ep.data())));
    printf("check c4 : %s\n", say(vel_fisher_check(4, 10, 3, ep.data())));
    printf("check N0 : %s\n", say(vel_fisher_check(2, 0, 3, ep.data())));
    printf("check E0 : %s\n", say(vel_fisher_check(2, 10, 0, ep.data())));
    printf("check E-neg : %s\n", say(vel_fisher_check(2, 10, -1, ep.data())));
    printf("check E-limit : %s\n", say(vel_fisher_check(2, 10, VEL_MAX_EPOCHS, ep.data())));
    printf("check E-huge : %s\n", say(vel_fisher_check(2, 10, VEL_MAX_EPOCHS + 1, ep.data())));
    printf("check null : %s\n", say(vel_fisher_check(2, 10, 3, nullptr)));
    printf("check index-high : %s\n", say(vel_fisher_check(2, 10, 2, ep.data())));
    ep[7] = -1;
    printf("check index-neg : %s\n", say(vel_fisher_check(2, 10, 3, ep.data())));
    return 0;
}
