// sky_kernels.hpp -- the sorted layout of a proposal slot and its skyline ("Skyline").
//
// The covariance is a sum of squared exponentials that underflow to exactly +0 once p2 d^2 <= -746 (kern_elem4_skip,
// fill_kernels.hpp).  With the rows ordered by ln-wavelength the matrix is a band, and a Cholesky factor stays inside the
// skyline of its matrix: tile (q, j) of the factor is zero whenever tiles (0 .. q, j) of the matrix are.  Behind every
// upload into a batch slot these kernels
//   1. rank the first walker's first component (a total order on the BITS of the keys, ties by index: a pure function of
//      the slot's contents) and gather lwl, fl and sigma through that permutation;
//   2. compute, per matrix, component and 128-row tile, the interval of the sorted ln-wavelengths, and from the intervals
//      first_b[j] -- the first block row q whose tile (q, j) is not PROVABLY zero: the gap g between the two intervals is
//      a lower bound of every |d| in the tile, rounding is monotone, so p2 g g <= -746 in the kernel's own arithmetic
//      implies the same for every element;
//   3. clamp first_b[j] <= j - 1 (the hand-over of the diagonal chain), make it non-decreasing, and write the union over
//      the batch, first[j] = min_b first_b[j], to pinned host memory for the planner (dag_build_tasks).
// The routines marked __host__ __device__ are shared with the host twin psoap_sky_first (psoap_gp.hip).
#pragma once
#include "common.hpp"

namespace psoap {

constexpr int SKY_MAX_N = 8192;              // beyond: identity permutation, dense plan
constexpr int SKY_MAX_P = SKY_MAX_N / NB;

// a double as an unsigned key whose order is the order of the finite values and total on all bit patterns
__host__ __device__ inline unsigned long long sky_key(double x)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// p2[c] as load_gp computes it; false: a hyper-parameter is negative, zero, NaN or infinite, or amp^2 is not finite (an
// infinite a2 times an exact zero is NaN in the dense evaluation) -- every tile counts as non-zero
__host__ __device__ inline bool sky_gp(const double* gp, int C, double* p2)
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
__host__ __device__ inline void sky_interval(const double* x, int i0, int i1, double* lo, double* hi)
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
__host__ __device__ inline bool sky_tile_zero(int q, int j, int P, int C, const double* lo, const double* hi, const double* p2)
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
__host__ __device__ inline int sky_first_raw(int j, int P, int C, const double* lo, const double* hi, const double* p2, bool ok)
{
    if (!ok) return 0;
    int q = 0;
    while (q < j && sky_tile_zero(q, j, P, C, lo, hi, p2)) ++q;
    return q;
}

// clamp to the tile above the diagonal, then non-decreasing (running minimum from the right)
__host__ __device__ inline void sky_first_finish(int* first, int P)
{
    for (int j = 0; j < P; ++j) {
        const int cap = j > 0 ? j - 1 : 0;
        first[j] = first[j] < cap ? first[j] : cap;
    }
    for (int j = P - 2; j >= 0; --j) first[j] = first[j] < first[j + 1] ? first[j] : first[j + 1];
}

// ---- device ----------------------------------------------------------------------------------------
// perm[rank(i)] = i, rank by (sky_key, index); x: the N keys
__global__ __launch_bounds__(256) void k_sky_perm(const double* __restrict__ x, int N, int* __restrict__ perm)
{
    __shared__ unsigned long long keys[1024];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long mine = i < N ? sky_key(x[i]) : 0ull;
    int rank = 0;
    for (int k0 = 0; k0 < N; k0 += 1024) {
        __syncthreads();
        for (int k = threadIdx.x; k < 1024; k += 256) keys[k] = k0 + k < N ? sky_key(x[k0 + k]) : 0ull;
        __syncthreads();
        const int n = N - k0 < 1024 ? N - k0 : 1024;
        for (int k = 0; k < n; ++k) {
            const unsigned long long o = keys[k];
            rank += (o < mine || (o == mine && k0 + k < i)) ? 1 : 0;
        }
    }
    if (i < N) perm[rank] = i;
}

// out[row][r] = in[row][perm[r]]: blockIdx.y < rows the slot's ln-wavelengths, then the handle's fl and sigma
__global__ __launch_bounds__(256) void k_sky_gather(const int* __restrict__ perm, int N, int rows,
                                                    const double* __restrict__ lwl, double* __restrict__ lwl_s,
                                                    const double* __restrict__ fl, double* __restrict__ fl_s,
                                                    const double* __restrict__ sigma, double* __restrict__ sigma_s)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const int src = perm[r];
    const int row = blockIdx.y;
    if (row < rows) lwl_s[(size_t)row * N + r] = lwl[(size_t)row * N + src];
    else if (row == rows) fl_s[r] = fl[src];
    else sigma_s[r] = sigma[src];
}

// first_b of matrix blockIdx.x (P <= SKY_MAX_P)
__global__ __launch_bounds__(256) void k_sky_first(const double* __restrict__ lwl_s, const double* __restrict__ gp, int C, int N,
                                                   int P, int* __restrict__ first_b)
{
    __shared__ double lo[3 * SKY_MAX_P], hi[3 * SKY_MAX_P];
    __shared__ int fb[SKY_MAX_P];
    const int b = blockIdx.x;
    const double* x = lwl_s + (size_t)b * C * N;
    for (int idx = threadIdx.x; idx < C * P; idx += 256) {
        const int c = idx / P, t = idx % P;
        const int i1 = (t + 1) * NB < N ? (t + 1) * NB : N;
        sky_interval(x + (size_t)c * N, t * NB, i1, &lo[idx], &hi[idx]);
    }
    __syncthreads();
    double p2[3] = {0.0, 0.0, 0.0};
    const bool ok = sky_gp(gp + (size_t)b * 2 * C, C, p2);
    if ((int)threadIdx.x < P) fb[threadIdx.x] = sky_first_raw((int)threadIdx.x, P, C, lo, hi, p2, ok);
    __syncthreads();
    if (threadIdx.x == 0) sky_first_finish(fb, P);
    __syncthreads();
    if ((int)threadIdx.x < P) first_b[(size_t)b * P + threadIdx.x] = fb[threadIdx.x];
}

// the union over the batch, to pinned host memory
__global__ void k_sky_union(const int* __restrict__ first_b, int B, int P, int* __restrict__ first_host)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P) return;
    int m = first_b[j];
    for (int b = 1; b < B; ++b) m = first_b[(size_t)b * P + j] < m ? first_b[(size_t)b * P + j] : m;
    first_host[j] = m;
}

}  // namespace psoap
