// draw_rng.hpp -- the integer core of the generator behind k_draw_normals (draw_kernels.hpp) and its host twin
// psoap_draw_philox (plan_abi.hpp): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as
// 1, 2, 3", SC'11) and the two 53-bit integers a counter block yields.  No HIP header: PSOAP_HD (tile_consts.hpp) is
// __host__ __device__ under hipcc and empty for a host compiler (tests/host/draw_host_check.cpp).
//
// The stream of a call: key = (seed low word, seed high word), counter = (pair index i >> 1 of element i within the draw,
// draw index d, 0, 0).  A block's words (w0, w1, w2, w3) give
//     k1 = (w0 >> 5) 2^26 + (w1 >> 6),   u1 = (k1 + 1) 2^-53  in (0, 1]      (the radius: log u1 is finite)
//     k2 = (w2 >> 5) 2^26 + (w3 >> 6),   u2 = k2 2^-53        in [0, 1)      (the angle)
// and Box-Muller makes elements 2 (i >> 1) and 2 (i >> 1) + 1 of draw d from them:
//     r = sqrt(-2 log u1),   z_even = r cos(2 pi u2),   z_odd = r sin(2 pi u2).
// Element i of draw d therefore depends on (seed, d, i) alone: not on the number of draws, the padding, the grid or the
// device.
#pragma once
#include <stdint.h>

#include "tile_consts.hpp"

namespace psoap {

struct PhiloxBlock {
    uint32_t w[4];
};

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // the round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // the key schedule (Weyl increments)

PSOAP_HD inline PhiloxBlock philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += PHILOX_W0, k1 += PHILOX_W1;      // (the bump after the last round is never used)
    }
    return PhiloxBlock{{c0, c1, c2, c3}};
}

// the block of (seed, pair index, draw index)
PSOAP_HD inline PhiloxBlock draw_block(unsigned long long seed, uint32_t pair, uint32_t draw)
{
    return philox4x32_10(pair, draw, 0u, 0u, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32));
}

// the 53-bit integer of two words: 27 bits of the first above 26 bits of the second
PSOAP_HD inline uint64_t draw_bits53(uint32_t hi, uint32_t lo) { return ((uint64_t)(hi >> 5) << 26) | (uint64_t)(lo >> 6); }

constexpr double DRAW_2M53 = 1.0 / 9007199254740992.0;      // 2^-53

// (both exact in fp64: k + 1 <= 2^53)
PSOAP_HD inline double draw_u_radius(const PhiloxBlock& b) { return (double)(draw_bits53(b.w[0], b.w[1]) + 1u) * DRAW_2M53; }
PSOAP_HD inline double draw_u_angle(const PhiloxBlock& b) { return (double)draw_bits53(b.w[2], b.w[3]) * DRAW_2M53; }

}  // namespace psoap
