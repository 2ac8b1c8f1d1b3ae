// mix_host_check.cpp -- the host-only header of the mixture moments (psoap_amd/csrc/mix_plan.hpp) built by a host compiler
// alone, with AddressSanitizer and UBSan (tests/test_mix_host.py).  Prints the plan over a grid of (R, S_max, want_sigma)
// -- the padded sizes, the upper tiles in launch order, the doubles of every buffer and the bytes -- and what every argument
// check answers; checks the plan's own invariants on the way (exit status 1 with a message).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <utility>

#include "../../psoap_amd/csrc/mix_plan.hpp"

using namespace psoap;

static void fail(const char* what)
{
    fprintf(stderr, "mix_host_check: %s\n", what);
    exit(1);
}

static const char* say(const char* why) { return why ? why : "accepted"; }

int main()
{
    const int Rs[] = {1, 127, 128, 129, 256, 3072};
    const int Ss[] = {1, KB - 1, KB, KB + 1, MIX_MAX_S};
    for (int R : Rs)
        for (int S : Ss)
            for (int want = 0; want < 2; ++want) {
                if (mix_check_plan(R, S, want)) fail("a valid shape was refused");
                MixPlan g;
                mix_plan(R, S, want, g);
                if (g.Rpad % NB || g.Rpad < R || g.Rpad - R >= NB || g.Rt * NB != g.Rpad) fail("Rpad");
                if (g.Spad % KB || g.Spad < S || g.Spad - S >= KB) fail("Spad");
                if (mix_depth(S) != g.Spad || mix_depth(1) != KB) fail("the K loop's depth");
                const long long want_tiles = want ? (long long)g.Rt * (g.Rt + 1) / 2 : 0;
                if ((long long)g.tiles.size() != want_tiles) fail("the number of tiles");
                // every upper tile exactly once, none below the diagonal, none outside
                std::set<std::pair<int, int>> seen;
                for (const MixTile& t : g.tiles) {
                    if (t.ti < 0 || t.tj < t.ti || t.tj >= g.Rt) fail("a tile outside the upper triangle");
                    if (!seen.insert(std::make_pair(t.ti, t.tj)).second) fail("a tile twice");
                    if ((long long)NB * (t.tj + 1) > g.Rpad) fail("a tile outside the buffer");
                }
                if ((long long)seen.size() != want_tiles) fail("a tile is missing");
                const long long r2 = (long long)g.Rpad * g.Rpad;
                if (g.sbar_doubles != (want ? r2 : g.Rpad) || g.out_doubles != (want ? r2 : 0)) fail("the accumulators' size");
                if (g.mu_doubles != (long long)g.Spad * g.Rpad || g.small_doubles != g.Spad + 3ll * g.Rpad + 1) fail("the stacked means' size");
                if (g.bytes != 8 * (g.sbar_doubles + g.out_doubles + 2 * g.mu_doubles + g.small_doubles)) fail("the bytes");
                printf("plan R=%d S=%d sigma=%d : Rpad %d Spad %d Rt %d | tiles", R, S, want, g.Rpad, g.Spad, g.Rt);
                if (g.Rt <= 3)
                    for (const MixTile& t : g.tiles) printf(" (%d,%d)", t.ti, t.tj);
                else
                    printf(" %zu", g.tiles.size());
                printf(" | doubles %lld %lld %lld %lld | bytes %lld\n", g.sbar_doubles, g.out_doubles, g.mu_doubles, g.small_doubles,
                       g.bytes);
            }
    printf("limits : NB %d KB %d MIX_MAX_S %d MIX_MAX_R %d\n", NB, KB, MIX_MAX_S, MIX_MAX_R);

    printf("check plan ok : %s\n", say(mix_check_plan(3072, 64, 1)));
    printf("check plan R0 : %s\n", say(mix_check_plan(0, 64, 1)));
    printf("check plan R-huge : %s\n", say(mix_check_plan(MIX_MAX_R + 1, 64, 1)));
    printf("check plan S0 : %s\n", say(mix_check_plan(128, 0, 1)));
    printf("check plan S-neg : %s\n", say(mix_check_plan(128, -4, 1)));
    printf("check plan S-limit : %s\n", say(mix_check_plan(128, MIX_MAX_S, 1)));
    printf("check plan S-huge : %s\n", say(mix_check_plan(128, MIX_MAX_S + 1, 1)));
    printf("check plan sigma2 : %s\n", say(mix_check_plan(128, 4, 2)));

    printf("check begin ok : %s\n", say(mix_check_begin(0, 0, 3, 1024, 64, 1, true)));
    printf("check begin ok-marg-var : %s\n", say(mix_check_begin(1, 2, 1, 127, 1, 0, true)));
    printf("check begin null : %s\n", say(mix_check_begin(0, 0, 3, 1024, 64, 1, false)));
    printf("check begin marg2 : %s\n", say(mix_check_begin(2, 0, 3, 1024, 64, 1, true)));
    printf("check begin mode3 : %s\n", say(mix_check_begin(0, 3, 3, 1024, 64, 1, true)));
    printf("check begin c4 : %s\n", say(mix_check_begin(0, 0, 4, 1024, 64, 1, true)));
    printf("check begin M0 : %s\n", say(mix_check_begin(0, 0, 2, 0, 64, 1, true)));
    printf("check begin mode2-c2 : %s\n", say(mix_check_begin(0, 2, 2, 64, 64, 1, true)));
    printf("check begin S0 : %s\n", say(mix_check_begin(0, 0, 2, 64, 0, 1, true)));
    printf("check begin S-huge : %s\n", say(mix_check_begin(0, 0, 2, 64, MIX_MAX_S + 1, 1, true)));
    printf("check begin R-huge : %s\n", say(mix_check_begin(0, 0, 3, MIX_MAX_R / 3 + 1, 4, 1, true)));
    printf("check begin R-mode1 : %s\n", say(mix_check_begin(0, 1, 2, MIX_MAX_R, 4, 1, true)));

    printf("check add ok : %s\n", say(mix_check_add(true, 0, 1, 1.0, true)));
    printf("check add ok-last : %s\n", say(mix_check_add(true, 15, 16, 1e-300, true)));
    printf("check add null : %s\n", say(mix_check_add(true, 0, 1, 1.0, false)));
    printf("check add no-begin : %s\n", say(mix_check_add(false, 0, 1, 1.0, true)));
    printf("check add w0 : %s\n", say(mix_check_add(true, 0, 4, 0.0, true)));
    printf("check add w-neg : %s\n", say(mix_check_add(true, 0, 4, -1.0, true)));
    printf("check add w-inf : %s\n", say(mix_check_add(true, 0, 4, INFINITY, true)));
    printf("check add w-nan : %s\n", say(mix_check_add(true, 0, 4, NAN, true)));
    printf("check add full : %s\n", say(mix_check_add(true, 4, 4, 1.0, true)));

    printf("check finish ok : %s\n", say(mix_check_finish(true, 1, 1, true, true)));
    printf("check finish ok-var : %s\n", say(mix_check_finish(true, 3, 0, false, true)));
    printf("check finish null : %s\n", say(mix_check_finish(true, 1, 1, true, false)));
    printf("check finish no-begin : %s\n", say(mix_check_finish(false, 0, 0, false, true)));
    printf("check finish sigma-in-var : %s\n", say(mix_check_finish(true, 1, 0, true, true)));
    printf("check finish empty : %s\n", say(mix_check_finish(true, 0, 1, true, true)));
    return 0;
}
