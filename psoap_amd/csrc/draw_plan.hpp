// draw_plan.hpp -- the pure-host part of the posterior draws (draw_kernels.hpp): the layout of the factor buffer
// [S' | Z], the launches of every block row of its factorisation, the tiles and K-loops of the triangular product, the
// workspace sizes and the argument checks.  No HIP call and no HIP header: psoap_gp.hip includes it into the library, and a
// host compiler builds the same text into a stand-alone, sanitized program (tests/host/draw_host_check.cpp).
//
// The factor buffer is Rpad rows of ld = Rpad + Dpad doubles: S' = Sigma + nugget I (identity on the padded diagonal) in
// the first Rpad columns, and beside it the normals k-major, Z[i][d] = element i of draw d, zero in rows >= R and columns
// >= D.  Z is NOT an appended column block of the factorisation: the strip of block row p ends at tile column Rt - 1.
// X = Z^T U is one 128 x 128 tile per workgroup, tile (td, tj) running block rows k = 0 .. tj of U (the last one masked to
// its upper half on load); the workgroups are handed the long K-loops first.
#pragma once
#include <vector>

#include "tile_consts.hpp"

namespace psoap {

constexpr int DRAW_MAX_D = 1 << 20;      // draws of one call (the buffer's leading dimension stays far inside an int)

struct DrawRow {
    int update;      // tiles of the panel-update launch of this block row (0: none, block row 0)
    int strip;       // tiles right of the diagonal tile
};

struct DrawTile {
    int td, tj;      // rows 128 td .. of X (draws), columns 128 tj .. (elements)
    int kblocks;     // block rows 0 .. kblocks - 1 of U enter its sum: tj + 1
};

struct DrawPlan {
    int R = 0, D = 0, Rpad = 0, Dpad = 0, Rt = 0, Dt = 0, ld = 0;
    std::vector<DrawRow> rows;       // Rt
    std::vector<DrawTile> tiles;     // Dt * Rt, in launch order
    long long factor_doubles = 0;    // [S' | Z]
    long long out_doubles = 0;       // X, Dpad x Rpad
};

// launch order -> tile: the longest K-loops (the last tile column) first, the draws' row blocks of one column together
PSOAP_HD inline DrawTile draw_tile(int t, int Rt, int Dt)
{
    const int tj = Rt - 1 - t / Dt;
    return DrawTile{t % Dt, tj, tj + 1};
}

inline void draw_plan(int R, int D, DrawPlan& g)
{
    g = DrawPlan();
    g.R = R;
    g.D = D;
    g.Rpad = round_up(R, NB);
    g.Dpad = round_up(D, NB);
    g.Rt = g.Rpad / NB;
    g.Dt = g.Dpad / NB;
    g.ld = g.Rpad + g.Dpad;
    for (int p = 0; p < g.Rt; ++p) g.rows.push_back(DrawRow{p > 0 ? g.Rt - p : 0, g.Rt - p - 1});
    for (int t = 0; t < g.Rt * g.Dt; ++t) g.tiles.push_back(draw_tile(t, g.Rt, g.Dt));
    g.factor_doubles = (long long)g.Rpad * g.ld;
    g.out_doubles = (long long)g.Dpad * g.Rpad;
}

// 128^3 tile products of the factorisation's panel updates and of the triangular product
inline double draw_update_units(const DrawPlan& g)
{
    double u = 0.0;
    for (int p = 0; p < g.Rt; ++p) u += (double)p * g.rows[(size_t)p].update;
    return u;
}
inline double draw_trmm_units(const DrawPlan& g) { return 0.5 * g.Dt * (double)g.Rt * (g.Rt + 1); }

// -> nullptr, or why the call is refused
inline const char* draw_check(bool sigma_valid, int D, double nugget)
{
    if (!sigma_valid)
        return "no predict call has formed Sigma on this handle (psoap_chunk_predict or psoap_chunk_predict_marg with Sigma_out first)";
    if (D < 1) return "D must be at least 1";
    if (D > DRAW_MAX_D) return "D must be at most 1048576";
    if (!(nugget >= 0.0) || nugget > 1.7976931348623157e308) return "nugget must be finite and >= 0";
    return nullptr;
}

}  // namespace psoap
