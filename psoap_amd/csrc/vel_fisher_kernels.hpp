// vel_fisher_kernels.hpp -- Fisher information of the per-epoch radial velocities at fixed hyper-parameters (not in the
// reference): the (c E, c E) matrix F[(k, e), (j, f)] = 1/2 tr(K^-1 K_(k,e) K^-1 K_(j,f)) for the velocity v[k, e] of every
// component k at every epoch e, whatever E is.
//
// The grids are x_k[n] = lwl[n] - v[k, epoch(n)] / c_kms; with d = x_k[n] - x_k[m], p_k = -1/2 c_kms^2 / l_k^2, G = K^-1 and the
// antisymmetric, cross-epoch-only matrix
//   Dv_k[m, n] = a_k^2 2 p_k d exp(p_k d^2) / c_kms * [epoch(m) != epoch(n)]
// the covariance derivative of v[k, e] is P_e R + R^T P_e^T, R the rows of Dv_k in epoch e.  With Z_k = G Dv_k (so that
// A_k = Dv_k G = -Z_k^T) and X_kj = Dv_k G Dv_j^T = Z_k^T Dv_j the generic trace becomes
//   F[(k, e), (j, f)] = sum over m in e, n in f of ( Z_k[n, m] Z_j[m, n] + G[m, n] X_kj[m, n] ):
// epoch-block sums of two element-wise products, c + c (c + 1) / 2 dense products in all.
//
// The staged factorisation of [K | I] and k_fisher_kinv run as for the generic Fisher information (fisher_kernels.hpp).  Then
//   k_vel_dv_fill        Dv_k, every tile of every component; exp() as the fills evaluate it; rows and columns >= N and
//                        within-epoch entries exact zeros; antisymmetric bit for bit
//   k_vel_z              Z_k = G Dv_k, every tile (K = Npad)
//   k_vel_contract<SYM>  one workgroup per tile of X_kj, formed in the MFMA accumulators and never stored; the epilogue
//                        multiplies by the G tile, adds the product of the two Z tiles and bins the 128 x 128 elements by
//                        (epoch of the row, epoch of the column) into the tile's own entries of an S x S matrix of bin sums
//                        (vel_fisher_plan.hpp: S slots, the distinct epochs of every tile row)
//   k_vel_finish         F[(k, e), (j, f)] from the bin sums, for (k, e) >= (j, f), mirrored: F == F^T bit for bit
//
// X_kk is symmetric only up to rounding and an upper tile stands for its mirror image too, so (the lesson of
// fisher_kernels.hpp) SYM runs both K-loops, Z_k^T Dv_k and Dv_k^T Z_k, into one accumulator over the upper tiles: the
// flops of one K-loop over all tiles, and the antisymmetric part of the rounding error cancels inside the accumulation.  A
// diagonal tile takes its elements row < col once and row == col half: the finishing kernel adds every bin sum and its
// mirror image.  X_kj, k > j, is not symmetric: every tile, one K-loop; the block (j, k) of F is the transpose of (k, j).
//
// Workspace beyond [K | I] and K^-1: 2 c Npad^2 doubles (Dv_k, Z_k) + c (c + 1) / 2 S^2 + (c E)^2 doubles and the plan's ints.
// Pixels in no epoch order are legal and cost more.  S is P + E or so for an epoch-major chunk and at most min(Npad, P E): the
// bin sums then grow to c (c + 1) / 2 Npad^2 doubles (48 Npad^2 bytes at c = 3: 3.2 GB at N = 8192, as much again as Dv_k and
// Z_k).  The binning loop of k_vel_contract makes one pass over a wave's 64 elements and one 6-step butterfly per bin: 1 to 9
// bins per tile for an epoch-major chunk, E^2 for pixels scattered over E < 128 epochs (400 at E = 20), at most 128 x 128.  By
// the instruction count a pass is of the order of a microsecond, so the worst case is some 20 ms per tile -- tenths of a second
// to a second per call at N = 6000 .. 8192 against 37 .. 152 ms of products; estimated, not measured.  Sort by epoch to avoid it.
// Flops beyond the factorisation and K^-1: 2 c N^3 (Z) + c (c + 1) N^3 (X), whatever E is.
// fp64 throughout, no atomics, every sum in an order fixed by (N, c, epoch_index).
#pragma once
#include "fisher_kernels.hpp"
#include "vel_fisher_plan.hpp"

namespace psoap {

// Dv_k, every tile (grid (P P, c)), in the layout of k_fisher_tangent_fill.
__global__ __launch_bounds__(256) void k_vel_dv_fill(double* __restrict__ Dv, size_t sq, int Npad, int N, int P,
                                                     const double* __restrict__ lwl, const double* __restrict__ gp,
                                                     const int* __restrict__ pixel_epoch /* (N) the epoch of every pixel */)
{
    __shared__ double xrow[NB];
    __shared__ int erow[NB];
    const int ti = blockIdx.x / P, tj = blockIdx.x % P, k = blockIdx.y;
    const int tid = threadIdx.x;
    const int i0 = ti * NB, j0 = tj * NB;
    double p2, coef;
    {
#pragma clang fp contract(off)
        const double a = gp[2 * k], l = gp[2 * k + 1];      // (as load_gp rounds them)
        p2 = -0.5 * (C_KMS * C_KMS) / (l * l);
        coef = (a * a) * 2.0 * p2 / C_KMS;
    }
    const double* x = lwl + (size_t)k * N;
    if (tid < NB) {
        const int i = i0 + tid;
        xrow[tid] = (i < N) ? x[i] : 0.0;
        erow[tid] = (i < N) ? pixel_epoch[i] : -1;
    }
    const int w = tid >> 6, rg = (tid >> 4) & 3, cp = tid & 15;
    const int ja = j0 + 32 * w + 2 * cp, jb = ja + 1;
    const double xa = (ja < N) ? x[ja] : 0.0, xb = (jb < N) ? x[jb] : 0.0;
    const int ea = (ja < N) ? pixel_epoch[ja] : -2, eb = (jb < N) ? pixel_epoch[jb] : -2;
    double* out = Dv + (size_t)k * sq;
    __syncthreads();
#pragma unroll 1
    for (int g4 = 0; g4 < NB / 16; ++g4) {
        double d[8], a[8], e[8];
        bool live = false;
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
#pragma clang fp contract(off)
            const double xi = xrow[16 * g4 + rg + 4 * s4];
            d[2 * s4] = xa - xi;
            d[2 * s4 + 1] = xb - xi;
            a[2 * s4] = p2 * d[2 * s4] * d[2 * s4];
            a[2 * s4 + 1] = p2 * d[2 * s4 + 1] * d[2 * s4 + 1];
            live = live || !(a[2 * s4] <= -746.0) || !(a[2 * s4 + 1] <= -746.0);
        }
        // exp() = +0 for the whole wave: no evaluation.  The entries below are then 0 * (coef d), zeros that carry the sign of d
        // -- as an exp() that underflows in a live wave leaves them -- while within-epoch and padding entries are +0.  "Exact
        // zeros" means either; every product and sum downstream treats the two alike.
        if (__builtin_amdgcn_ballot_w64(live) != 0ull) {
            exp_nonpos_batch<8>(a, e);
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) e[q] = 0.0;
        }
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
#pragma clang fp contract(off)
            const int r = 16 * g4 + rg + 4 * s4;
            const int ei = erow[r];      // -1 beyond N: never equal to ea, eb >= 0; the columns beyond N carry -2
            d2 v;
            v.x = (ei >= 0 && ea >= 0 && ei != ea) ? e[2 * s4] * (coef * d[2 * s4]) : 0.0;
            v.y = (ei >= 0 && eb >= 0 && ei != eb) ? e[2 * s4 + 1] * (coef * d[2 * s4 + 1]) : 0.0;
            *reinterpret_cast<d2*>(out + (size_t)(i0 + r) * Npad + ja) = v;
        }
    }
}

// Z_k = G Dv_k: Z[q][m] = sum_i G[i][q] Dv_k[i][m] (G is symmetric, so its block columns are the k-major operand).
// grid (P P, c): tile t of `tiles` (the plan's row-major list)
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_vel_z(const double* __restrict__ Kinv, const double* __restrict__ Dv,
                                                          size_t sq, int Npad, const int* __restrict__ tiles,
                                                          double* __restrict__ Z)
{
    const int tq = tiles[2 * blockIdx.x], tm = tiles[2 * blockIdx.x + 1];
    const double* D = Dv + (size_t)blockIdx.y * sq;
    double* Zk = Z + (size_t)blockIdx.y * sq;
    Tile t;
    t.zero();
    tile_gemm_tn(t, Kinv + NB * tq, (size_t)Npad, D + NB * tm, (size_t)Npad, Npad);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double* p0 = Zk + (size_t)(NB * tq + tile_row(wr, m, lane, r)) * Npad + NB * tm + tile_col(wc, 0, lane);
#pragma unroll
            for (int n = 0; n < 4; ++n) p0[16 * n] = t.acc[m][n][r];
        }
}

// One workgroup per tile (ti, tj) of X = Z_k^T Dv_j -- SYM (k == j): per UPPER tile of Z_k^T Dv_k + Dv_k^T Z_k = 2 X_sym --
// then, element by element, val = Z_k[col][row] Z_j[row][col] + G[row][col] X[row][col] and its bin sums: entry
// (slot(row), slot(col)) of `part` (S x S; this tile owns the entries of its slots and nobody else writes them).  Rows and
// columns >= N carry slot -1 and enter no bin.  SYM, diagonal tile: row < col once, row == col half, row > col not at all.
// A wave adds its elements of a bin in the fixed order (m, n, r), the 64 lanes meet in a butterfly, the four waves in LDS
// in the order 0, 1, 2, 3.
template <bool SYM>
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_vel_contract(const double* __restrict__ Kinv, const double* __restrict__ Zk,
                                                                 const double* __restrict__ Zj, const double* __restrict__ Dk,
                                                                 const double* __restrict__ Dj, int Npad, int S,
                                                                 const int* __restrict__ tiles, const int* __restrict__ slot_of,
                                                                 const int* __restrict__ slot_first, double* __restrict__ part)
{
    constexpr int PASS = (int)(GEMM_LDS_BYTES / sizeof(double)) / 4;      // bins per pass through LDS: four wave sums each
    const int ti = tiles[2 * blockIdx.x], tj = tiles[2 * blockIdx.x + 1];
    Tile t;
    t.zero();
    tile_gemm_tn(t, Zk + NB * ti, (size_t)Npad, Dj + NB * tj, (size_t)Npad, Npad);
    if (SYM) tile_gemm_tn(t, Dk + NB * ti, (size_t)Npad, Zk + NB * tj, (size_t)Npad, Npad);      // (+ its transpose's tile)

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int sf_i = slot_first[ti], sf_j = slot_first[tj];
    const int ns_i = slot_first[ti + 1] - sf_i, ns_j = slot_first[tj + 1] - sf_j;
    const bool diag_tile = SYM && ti == tj;
    int cs[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) cs[n] = slot_of[NB * tj + tile_col(wc, n, lane)] - sf_j;      // (-1 - sf_j < 0 beyond N)
    int rs[4][4];
    // the values in place of the accumulators
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = tile_row(wr, m, lane, r);
            const size_t gi = (size_t)(NB * ti + row);
            rs[m][r] = slot_of[gi] - sf_i;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int col = tile_col(wc, n, lane);
                const size_t gj = (size_t)(NB * tj + col);
                const double g = Kinv[gi * Npad + gj];
                const double zj = Zj[gi * Npad + gj];
                const double zk = Zk[gj * Npad + gi];
                const double x = SYM ? 0.5 * t.acc[m][n][r] : t.acc[m][n][r];
                double w = 1.0;
                if (diag_tile) w = row < col ? 1.0 : (row == col ? 0.5 : 0.0);
                t.acc[m][n][r] = w * fma(g, x, zk * zj);
            }
        }
    // (the K-loop's last barrier is behind every wave: LDS is free)
    const int nbins = ns_i * ns_j;
    for (int base = 0; base < nbins; base += PASS) {
        const int count = nbins - base < PASS ? nbins - base : PASS;
        for (int q = 0; q < count; ++q) {
            const int si = (base + q) / ns_j, sj = (base + q) % ns_j;
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s += (rs[m][r] == si && cs[n] == sj) ? t.acc[m][n][r] : 0.0;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
            if (lane == 0) psoap_smem[4 * q + wave] = s;
        }
        __syncthreads();
        for (int q = tid; q < count; q += GEMM_THREADS) {
            const int si = (base + q) / ns_j, sj = (base + q) % ns_j;
            part[(size_t)(sf_i + si) * S + sf_j + sj] =
                ((psoap_smem[4 * q] + psoap_smem[4 * q + 1]) + psoap_smem[4 * q + 2]) + psoap_smem[4 * q + 3];
        }
        __syncthreads();
    }
}

// F[(k, e), (j, f)] for (k, e) >= (j, f), mirrored.  One thread per entry of the lower triangle (grid ceil(T T / 64), 64
// threads; T = c E).  k == j: U = part of the pair (k, k) holds the bin sums of the upper tiles, and
//   F = sum_{a in slots(e), b in slots(f), block(a) <= block(b)} U[a][b] + sum_{a in slots(f), b in slots(e), block(a) <= block(b)} U[a][b]
// (an element below the diagonal tiles through its mirror image); k > j: F = sum_{a in slots(e), b in slots(f)} V[a][b].
// The slots of an epoch come in ascending order; an epoch without pixels has none: an exactly-zero row and column.
__global__ __launch_bounds__(64) void k_vel_finish(const double* __restrict__ part, int S, int C, int E,
                                                   const int* __restrict__ epoch_ptr, const int* __restrict__ epoch_slots,
                                                   const int* __restrict__ slot_block, double* __restrict__ F)
{
    const long long T = (long long)C * E;
    const long long idx = (long long)blockIdx.x * 64 + threadIdx.x;
    if (idx >= T * T) return;
    const int s = (int)(idx / T), u = (int)(idx % T);
    if (s < u) return;
    const int k = s / E, e = s % E, j = u / E, f = u % E;
    const double* M = part + (size_t)(k * (k + 1) / 2 + j) * S * S;
    const int e0 = epoch_ptr[e], e1 = epoch_ptr[e + 1], f0 = epoch_ptr[f], f1 = epoch_ptr[f + 1];
    double out;
    if (k == j) {
        double s1 = 0.0, s2 = 0.0;
        for (int ia = e0; ia < e1; ++ia)
            for (int ib = f0; ib < f1; ++ib) {
                const int a = epoch_slots[ia], b = epoch_slots[ib];
                if (slot_block[a] <= slot_block[b]) s1 += M[(size_t)a * S + b];
            }
        for (int ia = f0; ia < f1; ++ia)
            for (int ib = e0; ib < e1; ++ib) {
                const int a = epoch_slots[ia], b = epoch_slots[ib];
                if (slot_block[a] <= slot_block[b]) s2 += M[(size_t)a * S + b];
            }
        out = s1 + s2;
    } else {
        out = 0.0;
        for (int ia = e0; ia < e1; ++ia)
            for (int ib = f0; ib < f1; ++ib) out += M[(size_t)epoch_slots[ia] * S + epoch_slots[ib]];
    }
    F[(size_t)s * T + u] = out;
    F[(size_t)u * T + s] = out;
}

inline hipError_t vel_fisher_configure_kernels()
{
    const int lds = (int)GEMM_LDS_BYTES;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_vel_z), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_vel_contract<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_vel_contract<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    return e;
}

// the workspace of psoap_chunk_fisher_vel beyond the Fisher workspace's K^-1 (grow-only; psoap_chunk_fisher_vel_release)
struct VelFisherWs {
    Grow<double> Dv, Z, Part, F;
    Grow<int> Plan, Epoch;
};

}  // namespace psoap
