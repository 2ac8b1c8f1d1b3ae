// draw_host_check.cpp -- the host-only headers of the posterior draws (psoap_amd/csrc/draw_rng.hpp, draw_plan.hpp) built by
// a host compiler alone, with AddressSanitizer and UBSan (tests/test_draw_host.py).  Prints the generator's counter blocks
// for a list of (seed, pair, draw), the known-answer block, the 53-bit integers of each block, the plan of the factorisation
// and of the triangular product over a grid of (R, D), and what the argument check answers; checks the plan's own
// invariants on the way (exit status 1 with a message).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <tuple>

#include "../../psoap_amd/csrc/draw_plan.hpp"
#include "../../psoap_amd/csrc/draw_rng.hpp"

using namespace psoap;

static void fail(const char* what)
{
    fprintf(stderr, "draw_host_check: %s\n", what);
    exit(1);
}

int main()
{
    const PhiloxBlock kat = philox4x32_10(0, 0, 0, 0, 0, 0);
    printf("kat : %08x %08x %08x %08x\n", kat.w[0], kat.w[1], kat.w[2], kat.w[3]);
    const unsigned long long seeds[] = {0ull, 1ull, 0x123456789abcdef0ull, 0xffffffffffffffffull, 0x00000001ffffffffull};
    const uint32_t pairs[] = {0u, 1u, 63u, 64u, 131071u, 0xffffffffu};
    const uint32_t draw_ids[] = {0u, 1u, 4095u, 0xffffffffu};
    for (unsigned long long seed : seeds)
        for (uint32_t pair : pairs)
            for (uint32_t d : draw_ids) {
                const PhiloxBlock b = draw_block(seed, pair, d);
                const double u1 = draw_u_radius(b), u2 = draw_u_angle(b);
                if (!(u1 > 0.0 && u1 <= 1.0 && u2 >= 0.0 && u2 < 1.0)) fail("a uniform left its interval");
                printf("philox seed=%llu pair=%u draw=%u : %08x %08x %08x %08x | %llu %llu\n", seed, pair, d, b.w[0], b.w[1], b.w[2],
                       b.w[3], (unsigned long long)draw_bits53(b.w[0], b.w[1]), (unsigned long long)draw_bits53(b.w[2], b.w[3]));
            }
    const int Rs[] = {1, 127, 128, 129, 257}, Ds[] = {1, 128, 129};
    for (int R : Rs)
        for (int D : Ds) {
            DrawPlan g;
            draw_plan(R, D, g);
            if (g.Rpad % NB || g.Dpad % NB || g.Rpad < R || g.Dpad < D || g.Rpad - R >= NB || g.Dpad - D >= NB) fail("padding");
            if ((int)g.rows.size() != g.Rt || (int)g.tiles.size() != g.Rt * g.Dt) fail("counts");
            // every (tile, k-block) pair with k <= tj exactly once; the K-loop and the operands stay inside the buffer
            std::set<std::tuple<int, int, int>> seen;
            for (const DrawTile& t : g.tiles) {
                if (t.td < 0 || t.td >= g.Dt || t.tj < 0 || t.tj >= g.Rt || t.kblocks != t.tj + 1) fail("a tile outside the product");
                if ((long long)NB * t.kblocks > g.Rpad || g.Rpad + NB * (t.td + 1) > g.ld) fail("an operand outside the buffer");
                for (int k = 0; k < t.kblocks; ++k)
                    if (!seen.insert(std::make_tuple(t.td, t.tj, k)).second) fail("a (tile, k-block) pair twice");
            }
            if ((long long)seen.size() != (long long)g.Dt * g.Rt * (g.Rt + 1) / 2) fail("a (tile, k-block) pair is missing");
            if (2.0 * draw_trmm_units(g) != (double)g.Dt * g.Rt * (g.Rt + 1)) fail("the product's units");
            for (int p = 0; p < g.Rt; ++p) {
                const DrawRow& r = g.rows[(size_t)p];
                // the strip ends at S's last tile column: Z is no appended column of the factorisation
                if (NB * (p + 1 + r.strip) != g.Rpad || (p > 0 ? r.update != g.Rt - p : r.update != 0)) fail("a block row's extent");
            }
            printf("plan R=%d D=%d : ld %d | rows", R, D, g.ld);
            for (const DrawRow& r : g.rows) printf(" (%d,%d)", r.update, r.strip);
            printf(" | tiles");
            for (const DrawTile& t : g.tiles) printf(" (%d,%d,%d)", t.td, t.tj, t.kblocks);
            printf(" | doubles %lld %lld | units %.1f %.1f\n", g.factor_doubles, g.out_doubles, draw_update_units(g), draw_trmm_units(g));
        }
    struct {
        const char* name;
        bool valid;
        int D;
        double nugget;
    } const checks[] = {{"ok", true, 1, 1e-8},      {"ok-zero", true, 5, 0.0},      {"no-sigma", false, 5, 1e-8},
                        {"D0", true, 0, 1e-8},      {"D-neg", true, -3, 1e-8},      {"D-huge", true, DRAW_MAX_D + 1, 1e-8},
                        {"nugget-neg", true, 5, -1e-300}, {"nugget-inf", true, 5, INFINITY}, {"nugget-nan", true, 5, NAN}};
    for (const auto& c : checks) {
        const char* why = draw_check(c.valid, c.D, c.nugget);
        printf("check %s : %s\n", c.name, why ? why : "accepted");
    }
    return 0;
}
