// marg_predict_plan.hpp -- the pure-host part of the prediction under the marginalised continuum
// (marg_predict_kernels.hpp): argument validation, the column layout of the [K | Cx^T | Ht] workspace, every appended tile
// column's first non-zero block row, the launches of every block row of both factorisations, the tiles of the Gram launch
// and the workspace bytes.  No HIP call and no HIP header: psoap_gp.hip includes it into the library, and a host compiler
// builds the same text into a stand-alone, sanitized program (tests/host/marg_predict_host_check.cpp).  marg_plan.hpp is used
// as it is.
//
// Layout.  One matrix is Npad rows of ld = Npad + Rpad + 128 Q doubles: K's P tile columns, then the Rt = Rpad / 128 tile
// columns of Cx^T at tile column P (R = c M prediction columns in mode 0, M otherwise; dense from row 0), then the Q tile
// columns of Ht at tile column P + Rt in marg_plan.hpp's slot order (ascending first row).  At block row p the columns to
// update and solve are K's own from p on, all of Cx^T and the slots 0 .. active[p] - 1: ONE contiguous range, so every block
// row is one update launch and one strip launch, and k_marg_panel_update serves with P + Rt in the place of P.
//
// [M | G].  S = 128 Q rows of ldm = S + Rpad doubles: M = I + Wh^T Wh in the column order of H (as psoap_chunk_lnlike_marg
// keeps it), then G = Wh^T Wc.  One launch forms both: its tiles are listed here, M's upper tiles first (marg_plan.hpp's
// list), then G's row by row; the K loop of a tile starts at the first row below the zeros of both operands (Cx^T has
// none).  Block row p of its factorisation updates and solves M's tiles from p on and all of G.
//
// Sigma.  The St (St + 1) / 2 upper tiles of the Rpad x Rpad result, St = Rt, row-major over the upper triangle.
#pragma once
#include <stddef.h>

#include <vector>

#include "marg_plan.hpp"
#include "predict_plan.hpp"

namespace psoap {

struct MargPredictTile {
    int row, col;          // the tile of [M | G] that is written (col counts M's Q tile columns, then G's)
    int a, b;              // the tile columns of [K | Cx^T | Ht] whose strips are multiplied: row operand, column operand
    int k0;                // first row of the K loop (a multiple of 128; Npad: nothing to add up)
    int diag;              // a diagonal tile of M: the upper half is written, with the identity
};

struct MargPredictRow {
    int update, strip;     // blocks of the update launch (0: block row 0 has nothing above it); tiles right of the diagonal tile
};

struct MargPredictPlan {
    int N = 0, P = 0, Q = 0;
    int mode = 0, c = 0, M = 0;
    PredictShape shape;                   // the plain call's numbers for this mode, c and M (its ld is not this layout's)
    int R = 0, Rt = 0;                    // prediction columns, their tile columns: the shape's
    int ld = 0;                           // doubles per row of [K | Cx^T | Ht]
    int tile_C = 0, tile_H = 0;           // first tile column of Cx^T and of Ht
    std::vector<int> tile, first;         // per appended column (C_0 .. C_{Rt-1}, H_0 .. H_{Q-1} in the column order of H)
    std::vector<MargPredictRow> rows;     // per block row of [K | Cx^T | Ht]
    int S = 0, ldm = 0;                   // side of M, doubles per row of [M | G]
    std::vector<MargPredictTile> gram;    // the tiles of the Gram launch
    std::vector<MargPredictRow> mrows;    // per block row of [M | G]
    int St = 0, sigma_tiles = 0;          // tile rows of Sigma, its upper tiles
};

// -> nullptr, or why a call is refused (the messages of psoap_chunk_lnlike_marg for the baseline)
inline const char* marg_predict_check(int mode, int c, int M, bool have_baseline, bool stale_weight)
{
    if (mode < 0 || mode > 2 || c < 1 || c > 3 || M < 1) return "bad arguments";
    if (mode == 2 && c != 1) return "mode 2 (predict_f) needs c == 1";
    if (mode == 1 && c == 3)
        return "mode 1 with three components is not provided (the transposed mean of predict_f_g_h_sum, covariance.py:294)";
    if (mode == 1 && c != 2) return "mode 1 (the sum) needs c == 2";
    if (mode == 0 && c < 2) return "mode 0 (the components) needs c == 2 or 3";
    if (!have_baseline) return "call psoap_chunk_set_baseline first";
    if (stale_weight)
        return "psoap_chunk_set_data changed the data the baseline's weights were given for (psoap_chunk_set_baseline again)";
    return nullptr;
}

// mu0: the first prior mean (what predict_f takes off fl)
inline void marg_predict_plan(const MargPlan& pl, int mode, int c, int M, MargPredictPlan& out, double mu0 = 1.0)
{
    out = MargPredictPlan();
    const int P = pl.P, Q = pl.Q;
    out.N = pl.N;
    out.P = P;
    out.Q = Q;
    out.mode = mode;
    out.c = c;
    out.M = M;
    (void)predict_shape(mode, c, pl.N, M, mu0, out.shape);      // (never the transposed mean: marg_predict_check)
    out.R = out.shape.Rq;
    const int Rt = out.shape.Rq_pad / NB;
    out.Rt = Rt;
    out.ld = NB * (P + Rt + Q);
    out.tile_C = P;
    out.tile_H = P + Rt;
    for (int j = 0; j < Rt; ++j) {
        out.tile.push_back(out.tile_C + j);
        out.first.push_back(0);
    }
    for (int t = 0; t < Q; ++t) {
        out.tile.push_back(out.tile_H + pl.slot[(size_t)t]);
        out.first.push_back(pl.first[(size_t)t]);
    }
    for (int p = 0; p < P; ++p) {
        const int n = P - p + Rt + pl.active[(size_t)p];
        out.rows.push_back(MargPredictRow{p > 0 ? n : 0, n - 1});
    }
    out.S = NB * Q;
    out.ldm = out.S + NB * Rt;
    for (const MargTile& t : pl.tiles)
        out.gram.push_back(MargPredictTile{t.ti, t.tj, out.tile_H + t.si, out.tile_H + t.sj, t.k0, t.ti == t.tj ? 1 : 0});
    for (int t = 0; t < Q; ++t)
        for (int j = 0; j < Rt; ++j)
            out.gram.push_back(MargPredictTile{t, Q + j, out.tile_H + pl.slot[(size_t)t], out.tile_C + j, NB * pl.first[(size_t)t], 0});
    for (int p = 0; p < Q; ++p) {
        const int n = Q - p + Rt;
        out.mrows.push_back(MargPredictRow{p > 0 ? n : 0, n - 1});
    }
    out.St = Rt;
    out.sigma_tiles = Rt * (Rt + 1) / 2;
}

// bytes of the three large buffers of a call: [K | Cx^T | Ht] and Sigma in the predict workspace, [M | G] beside the
// baseline's device side
inline size_t marg_predict_k_bytes(const MargPredictPlan& g) { return sizeof(double) * (size_t)NB * g.P * (size_t)g.ld; }
inline size_t marg_predict_m_bytes(const MargPredictPlan& g) { return sizeof(double) * (size_t)g.S * (size_t)g.ldm; }
inline size_t marg_predict_sigma_bytes(const MargPredictPlan& g) { return sizeof(double) * (size_t)NB * g.Rt * (size_t)NB * g.Rt; }

// executed 128^3 products of a call, for the profiling records: the two factorisations' updates, the Gram launch (a
// diagonal tile of M issues three quarters of its MFMAs) and Sigma's two K loops
inline double marg_predict_gram_units(const MargPredictPlan& g)
{
    double u = 0.0;
    for (const MargPredictTile& t : g.gram) u += (t.diag ? 0.75 : 1.0) * (g.P - t.k0 / NB);
    return u;
}

// flops of psoap_chunk_predict_timings: the plain F_pred plus N S (S + R) + S^3 / 3 + S^2 R + S R^2 on padded sizes (the
// last term, like the plain N R^2, only when Sigma is formed: 2 S R for the variances alone)
inline double marg_predict_flops(const MargPredictPlan& g, bool sigma, bool var)
{
    const double n = (double)NB * g.P, r = (double)NB * g.Rt, s = g.S;
    return predict_flops(n, r, sigma, var) + n * s * (s + r) + s * s * s / 3.0 + s * s * r + (sigma ? s * r * r : (var ? 2.0 * s * r : 0.0));
}

}  // namespace psoap
