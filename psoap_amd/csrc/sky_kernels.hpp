// sky_kernels.hpp -- the sorted layout of a proposal slot and its skyline ("Skyline").
//
// The covariance is a sum of squared exponentials that underflow to exactly +0 once p2 d^2 <= -746 (kern_elem4_skip,
// fill_kernels.hpp).  With the rows ordered by ln-wavelength the matrix is a band, and a Cholesky factor stays inside the
// skyline of its matrix: tile (q, j) of the factor is zero whenever tiles (0 .. q, j) of the matrix are.  Any symmetric
// permutation is valid, and with several components no single order makes every component a band: the order by one
// component's grid spreads the others by the epochs' velocity differences.  So the order is CHOSEN per upload among a few
// candidates, convex blends of the first walker's component grids (sky_cand_weights: 1, 9 or 15 of them for 1, 2 or 3
// components; candidate 0 is the first component alone).  Behind every upload into a batch slot these kernels
//   1. per candidate, rank the blended key (a total order on the BITS of the keys, ties by index: a pure function of the
//      slot's contents);
//   2. per candidate, matrix, component and 128-row tile, compute the interval of the ln-wavelengths read through the
//      candidate's permutation, and from the intervals first_b[j] -- the first block row q whose tile (q, j) is not
//      PROVABLY zero: the gap g between the two intervals is a lower bound of every |d| in the tile, rounding is monotone,
//      so p2 g g <= -746 in the kernel's own arithmetic implies the same for every element; first_b[j] is clamped to
//      j - 1 (the hand-over of the diagonal chain) and made non-decreasing;
//   3. per candidate, form the union over the batch, first[j] = min_b first_b[j], and its cost in tile-GEMM units
//      (sky_cost: what the planner's list executes per matrix); the smallest cost wins, ties to the lowest candidate, so
//      the plan is never larger than candidate 0's; the winner's first[] goes to pinned host memory for the planner
//      (dag_build_tasks), and the winner's first_b rows stay on the device for the kernel, which clips every matrix's
//      updates to its own envelope inside that list (DagMat::first); what the clip leaves, sum_b sky_cost(first_b), goes
//      to pinned host memory too;
//   3a. for the winner only, per matrix and column tile the first 16-row group that is not provably zero by the same test
//      (k_sky_fine; the row interval over 16 rows, the column interval over the tile): the row the updates of dag_update
//      start at, one stage of the K-loop fine; not queued under PSOAP_SKY_FINE=0, where the rows stay 8 first_b;
//   4. gather lwl, fl and sigma through the winner's permutation -- nothing is gathered for a candidate that loses.
// The routines these kernels share with the host twins psoap_sky_first (candidate 0), psoap_sky_order, psoap_sky_clip and
// psoap_sky_clip16: sky_rules.hpp.
#pragma once
#include "common.hpp"
#include "sky_rules.hpp"

namespace psoap {

// ---- device ----------------------------------------------------------------------------------------
// candidate blockIdx.y: perm[cand][rank(i)] = i, rank by (sky_key of the blended key, index); x: the first walker's C grids
__global__ __launch_bounds__(256) void k_sky_perm(const double* __restrict__ x, int C, int N, int* __restrict__ perm)
{
    __shared__ unsigned long long keys[1024];
    const int cand = blockIdx.y;
    double w[3];
    sky_cand_weights(C, cand, w);
    auto key = [&](int i) {
        double v[3] = {0.0, 0.0, 0.0};
        for (int c = 0; c < C; ++c) v[c] = x[(size_t)c * N + i];
        return sky_key(sky_cand_key(C, w, v));
    };
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long mine = i < N ? key(i) : 0ull;
    int rank = 0;
    for (int k0 = 0; k0 < N; k0 += 1024) {
        __syncthreads();
        // (past N: the largest key under an index no row has -- it counts for nobody, and the loop below has a fixed length:
        // unrolled, its LDS reads overlap; one block per compute unit has no other wavefront to hide their latency)
        for (int k = threadIdx.x; k < 1024; k += 256) keys[k] = k0 + k < N ? key(k0 + k) : ~0ull;
        __syncthreads();
#pragma unroll 16
        for (int k = 0; k < 1024; ++k) {
            const unsigned long long o = keys[k];
            rank += (o < mine || (o == mine && k0 + k < i)) ? 1 : 0;
        }
    }
    if (i < N) perm[(size_t)cand * N + rank] = i;
}

// out[row][r] = in[row][perm[*cand][r]]: blockIdx.y < rows the slot's ln-wavelengths, then the handle's fl and sigma
__global__ __launch_bounds__(256) void k_sky_gather(const int* __restrict__ perm, const int* __restrict__ cand, int N, int rows,
                                                    const double* __restrict__ lwl, double* __restrict__ lwl_s,
                                                    const double* __restrict__ fl, double* __restrict__ fl_s,
                                                    const double* __restrict__ sigma, double* __restrict__ sigma_s)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const int src = perm[(size_t)cand[0] * N + r];
    const int row = blockIdx.y;
    if (row < rows) lwl_s[(size_t)row * N + r] = lwl[(size_t)row * N + src];
    else if (row == rows) fl_s[r] = fl[src];
    else sigma_s[r] = sigma[src];
}

// first_b of matrix blockIdx.x under candidate blockIdx.y (P <= SKY_MAX_P): lwl in the upload's order, read through the
// candidate's permutation.  One wavefront per (component, tile) interval; minimum, maximum and the NaN flag do not depend
// on the order of the reduction, so the intervals are sky_interval's.
__global__ __launch_bounds__(256) void k_sky_first(const double* __restrict__ lwl, const int* __restrict__ perm,
                                                   const double* __restrict__ gp, int C, int N, int P, int* __restrict__ first_b)
{
    __shared__ double lo[3 * SKY_MAX_P], hi[3 * SKY_MAX_P];
    __shared__ int fb[SKY_MAX_P];
    const int b = blockIdx.x, cand = blockIdx.y, B = gridDim.x;
    const double* x = lwl + (size_t)b * C * N;
    const int* pm = perm + (size_t)cand * N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int idx = wave; idx < C * P; idx += 4) {
        const int c = idx / P, t = idx % P;
        const int i1 = (t + 1) * NB < N ? (t + 1) * NB : N;
        double a = __builtin_inf(), z = -__builtin_inf();
        int nan = 0;
        for (int i = t * NB + lane; i < i1; i += 64) {
            const double v = x[(size_t)c * N + pm[i]];
            nan |= !(v == v) ? 1 : 0;
            a = v < a ? v : a;
            z = v > z ? v : z;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double a2 = __shfl_xor(a, off), z2 = __shfl_xor(z, off);
            nan |= __shfl_xor(nan, off);
            a = a2 < a ? a2 : a;
            z = z2 > z ? z2 : z;
        }
        if (lane == 0) {
            lo[idx] = nan ? -__builtin_inf() : a;
            hi[idx] = nan ? __builtin_inf() : z;
        }
    }
    __syncthreads();
    double p2[3] = {0.0, 0.0, 0.0};
    const bool ok = sky_gp(gp + (size_t)b * 2 * C, C, p2);
    if ((int)threadIdx.x < P) fb[threadIdx.x] = sky_first_raw((int)threadIdx.x, P, C, lo, hi, p2, ok);
    __syncthreads();
    if (threadIdx.x == 0) sky_first_finish(fb, P);
    __syncthreads();
    if ((int)threadIdx.x < P) first_b[((size_t)cand * B + b) * P + threadIdx.x] = fb[threadIdx.x];
}

// per candidate the union over the batch and its cost; the cheapest candidate (ties: the lowest) to *cand_out, its union to
// pinned host memory; its per-matrix rows to first_w (B, P) and their cost, summed over the batch, to *units_host (pinned).
// first16_w (B, P): the same rows in 16-row groups, 8 first_w -- what DagMat::first points at until k_sky_fine refines it.
// One block; first_b (K, B, P), K <= SKY_MAX_CAND, P <= SKY_MAX_P.
__global__ __launch_bounds__(256) void k_sky_choose(const int* __restrict__ first_b, int B, int P, int K,
                                                    int* __restrict__ first_host, int* __restrict__ cand_out,
                                                    int* __restrict__ first_w, long long* __restrict__ units_host,
                                                    int* __restrict__ first16_w)
{
    __shared__ int fu[SKY_MAX_CAND * SKY_MAX_P];
    __shared__ long long cost[SKY_MAX_CAND];
    __shared__ unsigned long long units;
    __shared__ int win;
    if (threadIdx.x == 0) units = 0ull;
    for (int idx = threadIdx.x; idx < K * P; idx += 256) {
        const int k = idx / P, j = idx % P;
        const int* f = first_b + (size_t)k * B * P + j;
        int m = f[0];
        for (int b = 1; b < B; ++b) m = f[(size_t)b * P] < m ? f[(size_t)b * P] : m;
        fu[idx] = m;
    }
    __syncthreads();
    if ((int)threadIdx.x < K) cost[threadIdx.x] = sky_cost(fu + threadIdx.x * P, P);
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0;
        for (int k = 1; k < K; ++k) best = cost[k] < cost[best] ? k : best;
        win = best;
        cand_out[0] = best;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < P; j += 256) first_host[j] = fu[win * P + j];
    const int* fw = first_b + (size_t)win * B * P;
    for (int idx = threadIdx.x; idx < B * P; idx += 256) {
        first_w[idx] = fw[idx];
        first16_w[idx] = SKY_GPT * fw[idx];
    }
    for (int b = threadIdx.x; b < B; b += 256) atomicAdd(&units, (unsigned long long)sky_cost(fw + (size_t)b * P, P));
    __syncthreads();
    if (threadIdx.x == 0) units_host[0] = (long long)units;
}

// The chosen candidate's envelope of matrix blockIdx.x by 16-row groups (sky_rules.hpp: sky_first16_raw), behind
// k_sky_choose: first16_w (B, P) row blockIdx.x, and to stages_host[blockIdx.x] (pinned) the 16-row stages the matrix's
// updates then run inside the union's list (first_w (B, P): the chosen candidate's rows by tiles, their minimum is the
// union).  Sixteen lanes per group interval, four groups per wavefront and step; G = ceil(N / 16) <= SKY_MAX_G.
__global__ __launch_bounds__(256) void k_sky_fine(const double* __restrict__ lwl, const int* __restrict__ perm,
                                                  const int* __restrict__ cand, const double* __restrict__ gp, int C, int N, int P,
                                                  const int* __restrict__ first_w, int* __restrict__ first16_w,
                                                  long long* __restrict__ stages_host)
{
    __shared__ double lo16[3 * SKY_MAX_G], hi16[3 * SKY_MAX_G];
    __shared__ double lo[3 * SKY_MAX_P], hi[3 * SKY_MAX_P];
    __shared__ int f16[SKY_MAX_P];
    __shared__ unsigned long long stages;
    const int b = blockIdx.x, B = gridDim.x, G = (N + SKY_G - 1) / SKY_G;
    const double* x = lwl + (size_t)b * C * N;
    const int* pm = perm + (size_t)cand[0] * N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) stages = 0ull;
    for (int base = 4 * wave; base < C * G; base += 16) {
        // (every lane takes the shuffles; one past the end, or past N in a ragged last group, carries the neutral values)
        const int idx = base + (lane >> 4);
        const int c = idx / G, g = idx % G, i = g * SKY_G + (lane & 15);
        double a = __builtin_inf(), z = -__builtin_inf();
        int nan = 0;
        if (idx < C * G && i < N) {
            const double v = x[(size_t)c * N + pm[i]];
            nan = !(v == v) ? 1 : 0;
            a = v < a ? v : a;
            z = v > z ? v : z;
        }
        for (int off = 8; off > 0; off >>= 1) {
            const double a2 = __shfl_xor(a, off), z2 = __shfl_xor(z, off);
            nan |= __shfl_xor(nan, off);
            a = a2 < a ? a2 : a;
            z = z2 > z ? z2 : z;
        }
        if ((lane & 15) == 0 && idx < C * G) {
            lo16[idx] = nan ? -__builtin_inf() : a;
            hi16[idx] = nan ? __builtin_inf() : z;
        }
    }
    __syncthreads();
    // a tile's interval from its groups': minimum, maximum and the NaN flag (an infinite pair) do not depend on the grouping
    for (int idx = threadIdx.x; idx < C * P; idx += 256) {
        const int c = idx / P, t = idx % P;
        const int g1 = (t + 1) * SKY_GPT < G ? (t + 1) * SKY_GPT : G;
        double a = __builtin_inf(), z = -__builtin_inf();
        for (int g = t * SKY_GPT; g < g1; ++g) {
            a = lo16[c * G + g] < a ? lo16[c * G + g] : a;
            z = hi16[c * G + g] > z ? hi16[c * G + g] : z;
        }
        lo[idx] = a;
        hi[idx] = z;
    }
    __syncthreads();
    double p2[3] = {0.0, 0.0, 0.0};
    const bool ok = sky_gp(gp + (size_t)b * 2 * C, C, p2);
    if ((int)threadIdx.x < P)
        f16[threadIdx.x] = sky_first16_raw((int)threadIdx.x, G, P, C, lo16, hi16, lo, hi, p2, ok,
                                           SKY_GPT * first_w[(size_t)b * P + threadIdx.x]);
    __syncthreads();
    if (threadIdx.x == 0) sky_first16_finish(f16, P);
    __syncthreads();
    if ((int)threadIdx.x < P) {
        const int j = threadIdx.x;
        int u = first_w[j];
        for (int k = 1; k < B; ++k) u = first_w[(size_t)k * P + j] < u ? first_w[(size_t)k * P + j] : u;
        first16_w[(size_t)b * P + j] = f16[j];
        atomicAdd(&stages, (unsigned long long)sky_stages_col(j, u, f16[j]));
    }
    __syncthreads();
    if (threadIdx.x == 0) stages_host[b] = (long long)stages;
}

}  // namespace psoap
