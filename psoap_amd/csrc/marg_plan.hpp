// marg_plan.hpp -- the pure-host part of the continuum-marginalised likelihood (marg_kernels.hpp): argument validation, the
// column layout of the basis H, where every appended tile column starts to be non-zero, the list of Gram tiles and the
// per-epoch abscissa map.  No HIP call and no HIP header: psoap_gp.hip includes it into the library, and a host compiler
// builds the same text into a stand-alone, sanitized program (tests/host/marg_host_check.cpp).
//
// Columns.  Epoch e owns the order + 1 columns e (order + 1) .. e (order + 1) + order of H (an epoch without pixels keeps
// its columns: they are zero); q = n_epochs (order + 1) columns make Q = ceil(q / 128) appended tile columns.  Every epoch's
// pixels form ONE contiguous run of the flattened chunk (as leave-one-out asks: loo_plan.hpp); the runs may come in any
// order of epoch ids.
//
// First rows.  Tile column t is zero above the first pixel row of the first epoch -- in ROW order, the minimum over the
// epochs whose columns lie in t -- and forward substitution keeps leading zeros: first[t] is that row / 128 (P for a tile
// column whose epochs are all empty), and nothing above block row first[t] is read or written.  first[] need not be
// monotone in t, so the workspace holds the appended tile columns in the order of ascending first[] (slot[t]; ties by t):
// at block row p the columns to update and solve are then the slots 0 .. active[p] - 1, contiguous with K's own columns.
//
// Gram tiles.  All Q (Q + 1) / 2 tiles (ti <= tj) of W^T W, row-major; the K loop of a tile starts at row
// 128 max(first[ti], first[tj]).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "tile_consts.hpp"

namespace psoap {

constexpr int MARG_MAX_ORDER = 15;       // = CAL_MAX_ORDER (calibrate_kernels.hpp; marg_kernels.hpp asserts it)
constexpr int MARG_MAX_Q = 1024;         // columns of H: at most 8 appended tile columns

struct MargTile {
    int ti, tj;            // ti <= tj: the tile of M (column order of H)
    int si, sj;            // the slots of the workspace that hold tile columns ti and tj
    int k0;                // first row of the K loop (a multiple of 128; Npad: nothing to add up)
};

struct MargPlan {
    int N = 0, P = 0, n_epochs = 0, order = 0;
    int q = 0, Q = 0;                      // columns of H, appended tile columns
    std::vector<int> start, count;         // per epoch id: its pixels [start, start + count) (start 0 for an empty epoch)
    std::vector<int> col0;                 // per epoch id: its first column of H
    std::vector<double> off, scl;          // per epoch id: u = off + scl x maps [min x, max x] onto [-1, 1] (0, 0: u = 0)
    std::vector<int> first;                // per tile column: first block row that can be non-zero (P: none)
    std::vector<int> slot;                 // per tile column: its position among the appended columns of the workspace
    std::vector<int> column;               // per slot: the tile column it holds
    std::vector<int> active;               // per block row p: slots 0 .. active[p] - 1 have first <= p
    std::vector<MargTile> tiles;
};

// -> nullptr, or why the arguments are refused
inline const char* marg_plan(const double* x, const int32_t* epoch, int N, int n_epochs, int order, const double* prior_sd,
                             MargPlan& out)
{
    out = MargPlan();
    if (N < 1) return "the chunk has no pixel";
    if (!x || !epoch || !prior_sd) return "null argument";
    if (order < 0 || order > MARG_MAX_ORDER) return "order must lie in [0, 15]";
    if (n_epochs < 1) return "n_epochs must be at least 1";
    if ((long long)(order + 1) * n_epochs > MARG_MAX_Q) return "(order + 1) n_epochs must not exceed 1024";
    for (int k = 0; k <= order; ++k)
        if (!(prior_sd[k] > 0.0) || !isfinite(prior_sd[k])) return "prior_sd must be finite and positive";
    const int P = round_up(N, NB) / NB;
    out.N = N;
    out.P = P;
    out.n_epochs = n_epochs;
    out.order = order;
    out.q = (order + 1) * n_epochs;
    out.Q = round_up(out.q, NB) / NB;
    out.start.assign((size_t)n_epochs, 0);
    out.count.assign((size_t)n_epochs, 0);
    for (int i = 0; i < N; ++i) {
        const int e = (int)epoch[i];
        if (e < 0 || e >= n_epochs) return "epoch index out of range";
        if (!isfinite(x[i])) return "the abscissae must be finite";
        if (out.count[e] == 0) out.start[e] = i;
        else if (out.start[e] + out.count[e] != i) return "the pixels of an epoch are not contiguous";
        out.count[e]++;
    }
    // the abscissa map of numpy.polynomial.Chebyshev(domain=[a, b]): off = (-b - a) / (b - a), scl = 2 / (b - a)
    out.col0.assign((size_t)n_epochs, 0);
    out.off.assign((size_t)n_epochs, 0.0);
    out.scl.assign((size_t)n_epochs, 0.0);
    out.first.assign((size_t)out.Q, P);
    for (int e = 0; e < n_epochs; ++e) {
        out.col0[e] = e * (order + 1);
        if (out.count[e] == 0) continue;
        double a = x[out.start[e]], b = a;
        for (int i = out.start[e]; i < out.start[e] + out.count[e]; ++i) a = std::min(a, x[i]), b = std::max(b, x[i]);
        if (b > a) {
            out.off[e] = (-b - a) / (b - a);
            out.scl[e] = 2.0 / (b - a);
        }
        for (int t = out.col0[e] / NB; t <= (out.col0[e] + order) / NB; ++t) out.first[t] = std::min(out.first[t], out.start[e] / NB);
    }
    out.column.resize((size_t)out.Q);
    for (int t = 0; t < out.Q; ++t) out.column[t] = t;
    std::stable_sort(out.column.begin(), out.column.end(), [&out](int a, int b) { return out.first[a] < out.first[b]; });
    out.slot.assign((size_t)out.Q, 0);
    for (int s = 0; s < out.Q; ++s) out.slot[out.column[s]] = s;
    out.active.assign((size_t)P, 0);
    for (int p = 0; p < P; ++p)
        for (int t = 0; t < out.Q; ++t) out.active[p] += out.first[t] <= p;
    for (int ti = 0; ti < out.Q; ++ti)
        for (int tj = ti; tj < out.Q; ++tj)
            out.tiles.push_back(MargTile{ti, tj, out.slot[ti], out.slot[tj], NB * std::max(out.first[ti], out.first[tj])});
    return nullptr;
}

}  // namespace psoap
