// vel_fisher_plan.hpp -- the pure-host part of the epoch-velocity Fisher information (vel_fisher_kernels.hpp): from the
// epoch of every pixel, the epoch bins of every tile row, the tile lists of the products and the workspace size.  No HIP
// call and no HIP header: psoap_gp.hip includes it into the library, and a host compiler builds the same text into a
// stand-alone, sanitized program (tests/host/vel_fisher_host_check.cpp).
//
// Any epoch index in [0, n_epochs) is legal, in any pixel order; an epoch may have no pixel.  The 128 rows of tile row q
// fall into the DISTINCT epochs present there: its bins ("slots"), in ascending epoch id.  Slots are numbered through the
// tile rows (slot_first[q] .. slot_first[q + 1]), S of them in all: P <= S <= min(N, P n_epochs), and about P + n_epochs for
// the epoch-major chunks of Chunk.apply_mask.  A product kernel leaves, per pair of components, the S x S matrix of the
// bin sums of its tiles -- entry (a, b) is written by the one tile (block(a), block(b)) and by nobody else -- and the
// finishing kernel adds, for epochs (e, f), the entries (a, b) with a in slots(e), b in slots(f) in that fixed order.
#pragma once
#include <stdint.h>

#include <vector>

#include "tile_consts.hpp"

namespace psoap {

struct VelTile {
    int ti, tj;
};

struct VelFisherPlan {
    int N = 0, Npad = 0, P = 0, n_epochs = 0, c = 0;
    int S = 0;                             // slots in all
    int n_pairs = 0;                       // c (c + 1) / 2 pairs of components (k >= j), pair index k (k + 1) / 2 + j
    std::vector<int> slot_of;              // (Npad) the slot of every row; -1 for rows >= N
    std::vector<int> slot_first;           // (P + 1)
    std::vector<int> slot_block;           // (S) the tile row of a slot
    std::vector<int> slot_epoch;           // (S)
    std::vector<int> epoch_ptr;            // (n_epochs + 1) into epoch_slots
    std::vector<int> epoch_slots;          // (S) the slots of epoch 0, of epoch 1, ...: ascending within an epoch
    std::vector<int> epoch_count;          // (n_epochs) pixels
    std::vector<VelTile> tiles_all;        // P P, row-major: the cross products X_kj, k > j, and Z_k
    std::vector<VelTile> tiles_upper;      // P (P + 1) / 2, row-major, ti <= tj: the symmetrised X_kk
    int max_slots = 0;                     // the most slots of one tile row
    long long int_count = 0;               // ints of the device copy (vel_plan_pack)
    long long square_doubles = 0;          // Npad^2 matrices: K^-1 and per component Dv_k and Z_k
    long long part_doubles = 0;            // n_pairs S^2
    long long out_doubles = 0;             // (c n_epochs)^2
    long long bytes = 0;                   // all of it beyond [K | I]
    double tile_units = 0.0;               // 128^3-products: c P^3 (Z) + n_pairs P^3 (X: all tiles once, or the upper ones twice)
};

// the offsets of the arrays inside the one int buffer the kernels read
struct VelPlanOffsets {
    long long slot_of, slot_first, slot_block, epoch_ptr, epoch_slots, tiles_all, tiles_upper, end;
};

inline VelPlanOffsets vel_plan_offsets(int Npad, int P, int S, int n_epochs)
{
    VelPlanOffsets o;
    o.slot_of = 0;
    o.slot_first = o.slot_of + Npad;
    o.slot_block = o.slot_first + P + 1;
    o.epoch_ptr = o.slot_block + S;
    o.epoch_slots = o.epoch_ptr + n_epochs + 1;
    o.tiles_all = o.epoch_slots + S;
    o.tiles_upper = o.tiles_all + 2ll * P * P;
    o.end = o.tiles_upper + (long long)P * (P + 1);
    return o;
}

constexpr int VEL_MAX_EPOCHS = 2048;

// -> nullptr, or why the call is refused
inline const char* vel_fisher_check(int c, int N, int n_epochs, const int32_t* epoch)
{
    if (c < 1 || c > 3) return "number of components must be 1, 2 or 3";
    if (N < 1) return "the chunk has no pixel";
    if (n_epochs < 1) return "n_epochs must be at least 1";
    if (n_epochs > VEL_MAX_EPOCHS) return "n_epochs must be at most 2048";
    if (!epoch) return "bad arguments";
    for (int i = 0; i < N; ++i)
        if (epoch[i] < 0 || epoch[i] >= n_epochs) return "epoch index out of range";
    return nullptr;
}

// (after vel_fisher_check)
inline void vel_fisher_plan(int c, int N, int n_epochs, const int32_t* epoch, VelFisherPlan& g)
{
    g = VelFisherPlan();
    g.c = c, g.N = N, g.n_epochs = n_epochs;
    g.Npad = round_up(N, NB);
    g.P = g.Npad / NB;
    g.n_pairs = c * (c + 1) / 2;
    g.slot_of.assign((size_t)g.Npad, -1);
    g.slot_first.assign((size_t)g.P + 1, 0);
    g.epoch_count.assign((size_t)n_epochs, 0);
    std::vector<int> local((size_t)n_epochs, -1);      // the slot of an epoch in the tile row at hand
    std::vector<int> present;
    for (int q = 0; q < g.P; ++q) {
        const int i0 = q * NB, i1 = (i0 + NB < N) ? i0 + NB : N;
        present.clear();
        for (int i = i0; i < i1; ++i)
            if (local[(size_t)epoch[i]] < 0) local[(size_t)epoch[i]] = 0, present.push_back((int)epoch[i]);
        // ascending epoch id (an insertion sort: at most 128 entries)
        for (size_t a = 1; a < present.size(); ++a)
            for (size_t b = a; b > 0 && present[b - 1] > present[b]; --b) {
                const int t = present[b];
                present[b] = present[b - 1], present[b - 1] = t;
            }
        g.slot_first[(size_t)q] = g.S;
        for (size_t a = 0; a < present.size(); ++a) {
            local[(size_t)present[a]] = g.S + (int)a;
            g.slot_block.push_back(q);
            g.slot_epoch.push_back(present[a]);
        }
        for (int i = i0; i < i1; ++i) {
            g.slot_of[(size_t)i] = local[(size_t)epoch[i]];
            g.epoch_count[(size_t)epoch[i]]++;
        }
        g.S += (int)present.size();
        if ((int)present.size() > g.max_slots) g.max_slots = (int)present.size();
        for (int e : present) local[(size_t)e] = -1;
    }
    g.slot_first[(size_t)g.P] = g.S;
    // the slots of every epoch, ascending (= ascending tile row): a counting sort by epoch
    g.epoch_ptr.assign((size_t)n_epochs + 1, 0);
    for (int a = 0; a < g.S; ++a) g.epoch_ptr[(size_t)g.slot_epoch[(size_t)a] + 1]++;
    for (int e = 0; e < n_epochs; ++e) g.epoch_ptr[(size_t)e + 1] += g.epoch_ptr[(size_t)e];
    g.epoch_slots.assign((size_t)g.S, 0);
    {
        std::vector<int> fill(g.epoch_ptr.begin(), g.epoch_ptr.end() - 1);
        for (int a = 0; a < g.S; ++a) g.epoch_slots[(size_t)fill[(size_t)g.slot_epoch[(size_t)a]]++] = a;
    }
    for (int ti = 0; ti < g.P; ++ti)
        for (int tj = 0; tj < g.P; ++tj) {
            g.tiles_all.push_back(VelTile{ti, tj});
            if (tj >= ti) g.tiles_upper.push_back(VelTile{ti, tj});
        }
    const long long sq = (long long)g.Npad * g.Npad, T = (long long)c * n_epochs;
    g.square_doubles = (1 + 2ll * c) * sq;
    g.part_doubles = (long long)g.n_pairs * g.S * g.S;
    g.out_doubles = T * T;
    g.int_count = vel_plan_offsets(g.Npad, g.P, g.S, n_epochs).end;
    g.bytes = 8 * (g.square_doubles + g.part_doubles + g.out_doubles) + 4 * g.int_count;
    g.tile_units = (double)(c + g.n_pairs) * g.P * g.P * g.P;
}

// the device copy: one int buffer, the arrays at vel_plan_offsets
inline void vel_plan_pack(const VelFisherPlan& g, std::vector<int>& out)
{
    const VelPlanOffsets o = vel_plan_offsets(g.Npad, g.P, g.S, g.n_epochs);
    out.assign((size_t)o.end, 0);
    for (int i = 0; i < g.Npad; ++i) out[(size_t)(o.slot_of + i)] = g.slot_of[(size_t)i];
    for (int q = 0; q <= g.P; ++q) out[(size_t)(o.slot_first + q)] = g.slot_first[(size_t)q];
    for (int a = 0; a < g.S; ++a) {
        out[(size_t)(o.slot_block + a)] = g.slot_block[(size_t)a];
        out[(size_t)(o.epoch_slots + a)] = g.epoch_slots[(size_t)a];
    }
    for (int e = 0; e <= g.n_epochs; ++e) out[(size_t)(o.epoch_ptr + e)] = g.epoch_ptr[(size_t)e];
    for (size_t t = 0; t < g.tiles_all.size(); ++t)
        out[(size_t)o.tiles_all + 2 * t] = g.tiles_all[t].ti, out[(size_t)o.tiles_all + 2 * t + 1] = g.tiles_all[t].tj;
    for (size_t t = 0; t < g.tiles_upper.size(); ++t)
        out[(size_t)o.tiles_upper + 2 * t] = g.tiles_upper[t].ti, out[(size_t)o.tiles_upper + 2 * t + 1] = g.tiles_upper[t].tj;
}

}  // namespace psoap
