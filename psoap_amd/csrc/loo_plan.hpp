// loo_plan.hpp -- the pure-host part of leave-one-out cross-validation (loo_kernels.hpp): from the epoch of every pixel,
// the contiguity check, the packed diagonal blocks of K^-1 and the list of band tiles.  No HIP call and no HIP header:
// psoap_gp.hip includes it into the library, and a host compiler builds the same text into a stand-alone, sanitized
// program (tests/host/loo_host_check.cpp).
//
// Every epoch's pixels must form ONE contiguous run of the flattened chunk (the epoch-major order of Chunk.apply_mask); the
// runs may come in any order of epoch ids, and an epoch may have no pixel.  A non-empty epoch owns one packed block: square,
// row-major, side = its pixel count rounded up to 128.  Blocks of DIFFERENT padded sides go through the staged factorisation
// in GROUPS OF EQUAL SIDE (ascending side; within a group ascending epoch id), one matrix of a batch per block, so that a
// chunk with one long and many short epochs pays sum side_e^2 doubles, not n_epochs max side^2.  The blocks of a group lie
// side^2 doubles apart, their right-hand sides side doubles apart, their inverted diagonal blocks (side / 128) 128^2 apart.
// Without an epoch index (pixel outputs only) every 128-pixel tile stands for an epoch: the band is the diagonal tiles.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "tile_consts.hpp"

namespace psoap {

// one packed block, as the host lays it out and the kernels read it (batch order)
struct LooBlock {
    long long offset;      // first double of the block in the packed storage
    long long rhs;         // first double of its right-hand side / solution
    long long wt;          // first double of its side / 128 inverted diagonal blocks
    int start, count;      // its pixels: [start, start + count)
    int side;              // count rounded up to 128
    int epoch;             // the epoch id it belongs to (the tile index without an epoch index)
};

struct LooTile {
    int ti, tj;            // ti <= tj
};

struct LooGroup {
    int side, first, count;      // blocks [first, first + count) of the batch order
};

struct LooLayout {
    int N = 0, n_epochs = 0;               // n_epochs: of the caller; the pseudo-epochs' count without an epoch index
    std::vector<int> start, count;         // per epoch id (start 0 for an empty epoch)
    std::vector<int> epoch_block;          // per epoch id: its block in batch order, -1 for an empty epoch
    std::vector<int> pixel_block;          // per pixel: its block in batch order
    std::vector<LooBlock> blocks;          // batch order
    std::vector<LooGroup> groups;
    std::vector<LooTile> tiles;            // the band, row-major (ti, then tj), each tile once
    long long block_doubles = 0, rhs_doubles = 0, wt_doubles = 0;
    int max_side = 0;
};

// -> nullptr, or why the layout is refused.  epoch == nullptr: one pseudo-epoch per 128-pixel tile (n_epochs is ignored).
inline const char* loo_layout(const int32_t* epoch, int N, int n_epochs, LooLayout& out)
{
    out = LooLayout();
    if (N < 1) return "the chunk has no pixel";
    const int P = round_up(N, NB) / NB;
    if (!epoch) n_epochs = P;
    if (n_epochs < 1) return "n_epochs must be at least 1";
    out.N = N;
    out.n_epochs = n_epochs;
    out.start.assign((size_t)n_epochs, 0);
    out.count.assign((size_t)n_epochs, 0);
    for (int i = 0; i < N; ++i) {
        const int e = epoch ? (int)epoch[i] : i / NB;
        if (e < 0 || e >= n_epochs) return "epoch index out of range";
        if (out.count[e] == 0) out.start[e] = i;
        else if (out.start[e] + out.count[e] != i) return "the pixels of an epoch are not contiguous";
        out.count[e]++;
    }
    // batch order: ascending padded side, then ascending epoch id
    std::vector<int> order;
    for (int e = 0; e < n_epochs; ++e)
        if (out.count[e] > 0) order.push_back(e);
    std::stable_sort(order.begin(), order.end(),
                     [&out](int a, int b) { return round_up(out.count[a], NB) < round_up(out.count[b], NB); });
    out.epoch_block.assign((size_t)n_epochs, -1);
    out.pixel_block.assign((size_t)N, -1);
    for (size_t k = 0; k < order.size(); ++k) {
        const int e = order[k];
        LooBlock b;
        b.start = out.start[e];
        b.count = out.count[e];
        b.side = round_up(b.count, NB);
        b.epoch = e;
        b.offset = out.block_doubles;
        b.rhs = out.rhs_doubles;
        b.wt = out.wt_doubles;
        out.block_doubles += (long long)b.side * b.side;
        out.rhs_doubles += b.side;
        out.wt_doubles += (long long)(b.side / NB) * NB * NB;
        out.max_side = std::max(out.max_side, b.side);
        if (out.groups.empty() || out.groups.back().side != b.side) out.groups.push_back(LooGroup{b.side, (int)k, 0});
        out.groups.back().count++;
        out.epoch_block[e] = (int)k;
        for (int i = b.start; i < b.start + b.count; ++i) out.pixel_block[i] = (int)k;
        out.blocks.push_back(b);
    }
    // the band: every tile (ti <= tj) that meets the diagonal block of some epoch -- both tile indices inside the epoch's
    // tile range [start / 128, (start + count - 1) / 128]
    std::vector<char> hit((size_t)P * P, 0);
    for (const LooBlock& b : out.blocks) {
        const int t0 = b.start / NB, t1 = (b.start + b.count - 1) / NB;
        for (int ti = t0; ti <= t1; ++ti)
            for (int tj = ti; tj <= t1; ++tj) hit[(size_t)ti * P + tj] = 1;
    }
    for (int ti = 0; ti < P; ++ti)
        for (int tj = ti; tj < P; ++tj)
            if (hit[(size_t)ti * P + tj]) out.tiles.push_back(LooTile{ti, tj});
    return nullptr;
}

}  // namespace psoap
