// sky_rules.hpp -- the routines the skyline kernels (sky_kernels.hpp) share with their host twins psoap_sky_first,
// psoap_sky_order, psoap_sky_clip and psoap_sky_clip16 (plan_abi.hpp): the envelope is integer work on comparisons both sides make alike, the keys are the same
// arithmetic.  No HIP header: PSOAP_HD (tile_consts.hpp) is __host__ __device__ under hipcc and empty for a host compiler.
#pragma once
#include "tile_consts.hpp"

namespace psoap {

constexpr int SKY_MAX_N = 8192;              // beyond: identity permutation, dense plan
constexpr int SKY_MAX_P = SKY_MAX_N / NB;
constexpr int SKY_MAX_CAND = 15;             // candidate orders of a slot (three components)

// a double as an unsigned key whose order is the order of the finite values and total on all bit patterns
PSOAP_HD inline unsigned long long sky_key(double x)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// candidate orders of a slot with C components
PSOAP_HD inline int sky_n_cand(int C) { return C == 2 ? 9 : C == 3 ? 15 : 1; }

// the blend of candidate k: eighths between two components; quarters over three, for a in 0..4: for b in 0..4-a the
// weights ((4-a-b)/4, a/4, b/4) -- all exact; candidate 0 is (1, 0, 0)
PSOAP_HD inline void sky_cand_weights(int C, int k, double* w)
{
    w[0] = 1.0;
    w[1] = w[2] = 0.0;
    if (C == 2) {
        w[0] = 1.0 - k / 8.0;
        w[1] = k / 8.0;
    } else if (C == 3) {
        int at = 0;
        for (int a = 0; a <= 4; ++a)
            for (int b = 0; b <= 4 - a; ++b, ++at)
                if (at == k) {
                    w[0] = (4 - a - b) / 4.0;
                    w[1] = a / 4.0;
                    w[2] = b / 4.0;
                }
    }
}

// the key of one row: sum of w[c] x[c] left to right, no contraction; a term of weight exactly 0 is skipped and a lone
// weight of 1 hands the component's bits through (an infinity or NaN elsewhere never reaches candidate 0's key)
PSOAP_HD inline double sky_cand_key(int C, const double* w, const double* x)
{
#pragma clang fp contract(off)
    double acc = 0.0;
    bool any = false;
    for (int c = 0; c < C; ++c) {
        if (w[c] == 0.0) continue;
        const double t = w[c] == 1.0 ? x[c] : w[c] * x[c];
        acc = any ? acc + t : t;
        any = true;
    }
    return acc;
}

// tile-GEMM units per matrix of the list inside first[0 .. P): tile (q, j) runs q - first[j] of them
PSOAP_HD inline long long sky_cost(const int* first, int P)
{
    long long u = 0;
    for (int j = 0; j < P; ++j) {
        const long long d = j - first[j];
        u += d * (d + 1) / 2;
    }
    return u;
}

// p2[c] as load_gp computes it; false: a hyper-parameter is negative, zero, NaN or infinite, or amp^2 is not finite (an
// infinite a2 times an exact zero is NaN in the dense evaluation) -- every tile counts as non-zero
PSOAP_HD inline bool sky_gp(const double* gp, int C, double* p2)
{
#pragma clang fp contract(off)
    bool ok = true;
    for (int c = 0; c < C; ++c) {
        const double amp = gp[2 * c], l = gp[2 * c + 1];
        const double a2 = amp * amp;
        if (!(amp > 0.0 && a2 < __builtin_inf() && l > 0.0 && l < __builtin_inf())) ok = false;
        p2[c] = -0.5 * (C_KMS * C_KMS) / (l * l);
    }
    return ok;
}

// interval of x[i0 .. i1): [-inf, +inf] when a NaN is among them
PSOAP_HD inline void sky_interval(const double* x, int i0, int i1, double* lo, double* hi)
{
    double a = __builtin_inf(), b = -__builtin_inf();
    bool nan = false;
    for (int i = i0; i < i1; ++i) {
        const double v = x[i];
        nan = nan || !(v == v);
        a = v < a ? v : a;
        b = v > b ? v : b;
    }
    *lo = nan ? -__builtin_inf() : a;
    *hi = nan ? __builtin_inf() : b;
}

// tile (q, j) is provably +0: for every component the two row intervals lie further apart than the kernel's support
// (lo, hi: [c * P + tile])
PSOAP_HD inline bool sky_tile_zero(int q, int j, int P, int C, const double* lo, const double* hi, const double* p2)
{
#pragma clang fp contract(off)
    for (int c = 0; c < C; ++c) {
        const double g1 = lo[c * P + j] - hi[c * P + q], g2 = lo[c * P + q] - hi[c * P + j];
        const double g = g1 > g2 ? g1 : g2;
        if (!(g > 0.0)) return false;
        const double a = p2[c] * g * g;
        if (!(a <= -746.0)) return false;
    }
    return true;
}

// the smallest q <= j whose tile (q, j) is not provably zero
PSOAP_HD inline int sky_first_raw(int j, int P, int C, const double* lo, const double* hi, const double* p2, bool ok)
{
    if (!ok) return 0;
    int q = 0;
    while (q < j && sky_tile_zero(q, j, P, C, lo, hi, p2)) ++q;
    return q;
}

// clamp to the tile above the diagonal, then non-decreasing (running minimum from the right)
PSOAP_HD inline void sky_first_finish(int* first, int P)
{
    for (int j = 0; j < P; ++j) {
        const int cap = j > 0 ? j - 1 : 0;
        first[j] = first[j] < cap ? first[j] : cap;
    }
    for (int j = P - 2; j >= 0; --j) first[j] = first[j] < first[j + 1] ? first[j] : first[j + 1];
}

// ---- the same envelope by 16-row groups (SKY_G = the k-rows of one stage of the tile engine, KB) --------------------
// Row group g is rows [16 g, 16 g + 16); the columns stay whole tiles.  A group's interval lies inside its tile's, the gap
// can only grow and every rounding is monotone: a group of a provably zero tile is provably zero, so the first group of
// a column is at or beyond 8 times its first tile.
constexpr int SKY_G = KB;
constexpr int SKY_GPT = NB / SKY_G;          // groups per tile
constexpr int SKY_MAX_G = SKY_MAX_N / SKY_G;

// rows of group g against the columns of tile j are provably +0: sky_tile_zero with the row interval taken over the
// group (lo16, hi16: [c * G + group]; lo, hi: [c * P + tile])
PSOAP_HD inline bool sky_group_zero(int g, int j, int G, int P, int C, const double* lo16, const double* hi16, const double* lo,
                                    const double* hi, const double* p2)
{
#pragma clang fp contract(off)
    for (int c = 0; c < C; ++c) {
        const double g1 = lo[c * P + j] - hi16[c * G + g], g2 = lo16[c * G + g] - hi[c * P + j];
        const double d = g1 > g2 ? g1 : g2;
        if (!(d > 0.0)) return false;
        const double a = p2[c] * d * d;
        if (!(a <= -746.0)) return false;
    }
    return true;
}

// the first group of column tile j that is not provably zero, looked for below the clamp 8 max(j - 1, 0) only (every
// group there is a whole one: it lies above the last tile).  g0: groups known to be provably zero -- the kernel starts at
// 8 times the column's first tile, the host twin at 0 and checks that it ends at or beyond that
PSOAP_HD inline int sky_first16_raw(int j, int G, int P, int C, const double* lo16, const double* hi16, const double* lo,
                                    const double* hi, const double* p2, bool ok, int g0 = 0)
{
    if (!ok) return 0;
    const int cap = j > 0 ? SKY_GPT * (j - 1) : 0;
    int g = g0 < cap ? g0 : cap;
    while (g < cap && sky_group_zero(g, j, G, P, C, lo16, hi16, lo, hi, p2)) ++g;
    return g;
}

// non-decreasing (running minimum from the right; the clamp is sky_first16_raw's)
PSOAP_HD inline void sky_first16_finish(int* first16, int P)
{
    for (int j = P - 2; j >= 0; --j) first16[j] = first16[j] < first16[j + 1] ? first16[j] : first16[j + 1];
}

// 16-row stages column tile j of one matrix runs inside the list of the union `u` = first[j] when its updates start at
// group s = first16[j] (dag_update): tile (q, j), u < q <= j, multiplies block rows [u, q) -- nothing if s lies at or
// beyond row 128 q, else the last panel whole and the panels before it from max(8 u, s) on.  s = 8 first_b[j]: 8 times the
// column's share of sky_cost(first_b).  (A tile whose update the list splits runs the last panel of every part whole.)
PSOAP_HD inline long long sky_stages_col(int j, int u, int s)
{
    long long n = 0;
    const int r0 = SKY_GPT * u > s ? SKY_GPT * u : s;
    for (int q = u + 1; q <= j; ++q) {
        if (s >= SKY_GPT * q) continue;
        const int before = SKY_GPT * (q - 1) - r0;
        n += SKY_GPT + (before > 0 ? before : 0);
    }
    return n;
}

}  // namespace psoap
