// loo_kernels.hpp -- leave-one-out cross-validation of the GP likelihood (not in the reference; Rasmussen & Williams 5.4.2).
//
// With r = fl - mu_GP, A = K^-1 and alpha = A r (K as the likelihood builds it, noise on the diagonal):
//   pixel i            mean = fl[i] - alpha[i] / A[i][i],  var = 1 / A[i][i],
//                      logp = 1/2 log A[i][i] - alpha[i]^2 / (2 A[i][i]) - 1/2 log(2 pi)
//   epoch e, pixels I  s = A[I,I]^-1 alpha[I]  (fl[I] minus its prediction from every other epoch),  chi2 = alpha[I] . s,
//                      logp = -1/2 chi2 + 1/2 log det A[I,I] - n/2 log(2 pi)
//
// The staged factorisation of [K | I] runs as for the gradient (grad_kernels.hpp) and leaves W = U^-T, A = W^T W, and alpha.  Then
//   k_loo_band      one workgroup per band tile (ti <= tj) of W^T W -- the tiles that meet the diagonal block of some epoch,
//                   listed by the host (loo_plan.hpp) -- with the K-loop bounds of k_fisher_kinv (from row 128 tj on); the epilogue
//                   scatters every element whose row and column lie in the same epoch, and its mirror image, into that epoch's
//                   packed block
//   k_loo_pad       the identity on the padding diagonal of the packed blocks (the storage is cleared before the band runs)
//   k_loo_rhs       per block: the right-hand side alpha[I] padded with zeros, and diag(A) read off the block's diagonal
//                   BEFORE the factorisation overwrites it: pixel and epoch results rest on the same numbers
//   the library's staged kernels (chol_kernels.hpp: k_panel_update, k_potrf_diag, k_trsm_strip), one matrix of the batch per
//                   non-empty epoch, group after group of equal padded side (loo_plan.hpp says why groups): A_ee = U^T U,
//                   z = U^-T alpha[I], log det.  Every block row keeps its inverted diagonal block (U_pp^-T, k-major)
//   k_loo_finish    one workgroup per epoch: the back substitution s = U^-1 z block row by block row with those inverses,
//                   then chi2 and logp in pixel order; one more workgroup: the pixel outputs and their sum in pixel order
// Without an epoch index every 128-pixel tile stands for an epoch (the band is the diagonal tiles) and neither the
// factorisation nor the epoch workgroups run; diag(A) comes out of the same kernel with the same K loop: the same bits.
//
// Workspace beyond the gradient's [K | I] for one matrix: sum side_e^2 doubles of packed blocks (side_e = n_e rounded up to
// 128), per block row a 128 x 128 inverse, and a few N-vectors.  Flops beyond the shared factorisation (2/3 N^3): the band,
// 2 128^2 (Npad - 128 tj) per tile (a diagonal tile three quarters of that), and sum side_e^3 / 3 of block factorisations.
// fp64 throughout, no atomics, every sum in an order fixed by (N, c, epoch layout).
#pragma once
#include "grad_kernels.hpp"
#include "loo_plan.hpp"

namespace psoap {

constexpr double LOO_HALF_LOG_2PI = 0.91893853320467274178;
constexpr int LOO_CHUNK = 2048;      // doubles a sequential sum walks out of LDS at a time

// The epilogue of a band tile (ti <= tj) of a symmetric A held in the accumulators: every element whose row and column lie
// in the same epoch, and its mirror image, into that epoch's packed block.  All 256 threads; LDS: the operand buffers.
__device__ __forceinline__ void loo_band_scatter(const Tile& t, int ti, int tj, int N, const int* __restrict__ pixel_block,
                                                 const LooBlock* __restrict__ blocks, double* __restrict__ Blk)
{
    constexpr int OF = 0;                 // [NB] long long: per column of the tile, the first double of its packed block
    constexpr int IX = NB;                // then, as ints: [2][NB] the pixel's block (rows, columns), [2][NB] its position in it,
                                          // [NB] the side of the column's block
    static_assert((IX + 3 * NB) * sizeof(double) <= GEMM_LDS_BYTES, "the epilogue fits the operand buffers");
    // (the thread id passes through an opaque statement: nothing of the epilogue is computed, loaded and kept in registers
    // ahead of the K-loop)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    long long* blk_off = reinterpret_cast<long long*>(psoap_smem + OF);
    int* blk_of = reinterpret_cast<int*>(psoap_smem + IX);
    int* pos_of = blk_of + 2 * NB;
    int* side_of = pos_of + 2 * NB;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    {
        const int side = tid >> 7, idx = tid & 127;
        const int g = NB * (side ? tj : ti) + idx;
        const int b = (g < N) ? pixel_block[g] : -1;
        blk_of[side * NB + idx] = b;
        pos_of[side * NB + idx] = (b >= 0) ? g - blocks[b].start : 0;
        if (side) {
            blk_off[idx] = (b >= 0) ? blocks[b].offset : 0;
            side_of[idx] = (b >= 0) ? blocks[b].side : 0;
        }
    }
    __syncthreads();
    const bool diag_tile = ti == tj;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int col = tile_col(wc, n, lane);
        const int bc = blk_of[NB + col], pc = pos_of[NB + col], sc = side_of[col];
        double* Bc = Blk + blk_off[col];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = tile_row(wr, m, lane, r);
                // (a diagonal tile: its upper half, both ways; rows and columns >= N belong to no block)
                if (bc >= 0 && blk_of[row] == bc && (!diag_tile || row <= col)) {
                    const double v = t.acc[m][n][r];
                    const int pr = pos_of[row];
                    Bc[(size_t)pr * sc + pc] = v;
                    Bc[(size_t)pc * sc + pr] = v;
                }
            }
    }
}

__global__ __launch_bounds__(GEMM_THREADS, 2) void k_loo_band(const double* __restrict__ A, int ld, int N, int Npad,
                                                             const LooTile* __restrict__ tiles,
                                                             const int* __restrict__ pixel_block,
                                                             const LooBlock* __restrict__ blocks, double* __restrict__ Blk)
{
    const int ti = tiles[blockIdx.x].ti, tj = tiles[blockIdx.x].tj;
    const double* W = A + Npad + (size_t)NB * tj * ld;
    Tile t;
    t.zero();
    tile_gemm_tn(t, W + NB * ti, (size_t)ld, W + NB * tj, (size_t)ld, Npad - NB * tj, ti == tj);
    loo_band_scatter(t, ti, tj, N, pixel_block, blocks, Blk);
}

// ones on the padding diagonal of every packed block.  grid n_blocks, 128 threads
__global__ __launch_bounds__(128) void k_loo_pad(const LooBlock* __restrict__ blocks, double* __restrict__ Blk)
{
    const LooBlock b = blocks[blockIdx.x];
    const int i = b.count + threadIdx.x;
    if (i < b.side) Blk[b.offset + (long long)i * b.side + i] = 1.0;
}

// per block: rhs = alpha[I] padded with zeros, diag(A) off the block's diagonal, the last accumulator record cleared (as
// k_init_rhs clears it).  grid n_blocks, 256 threads
__global__ __launch_bounds__(256) void k_loo_rhs(const LooBlock* __restrict__ blocks, const double* __restrict__ Blk,
                                                 const double* __restrict__ alpha, double* __restrict__ rhs,
                                                 double* __restrict__ diag, MatAcc* __restrict__ acc)
{
    const LooBlock b = blocks[blockIdx.x];
    for (int i = threadIdx.x; i < b.side; i += 256) {
        rhs[b.rhs + i] = (i < b.count) ? alpha[b.start + i] : 0.0;
        if (i < b.count) diag[b.start + i] = Blk[b.offset + (long long)i * b.side + i];
    }
    if (threadIdx.x == 0) acc[(size_t)blockIdx.x * ACC_ROWS + ACC_ROWS - 1] = MatAcc{0.0, 0.0, 0.0, 0.0};
}

// grid n_ep + 1, 256 threads (n_ep = 0 without an epoch index).
//   blocks e < n_ep: epoch e.  U (the factored packed block), z = U^-T alpha[I] and the inverses Wt[p][i][k] = (U_pp^-1)[i][k]
//     of its diagonal blocks are there; block row p, from the last one up:
//       y[i] = z[128 p + i] - sum_{k >= 128 (p + 1)} U[128 p + i][k] s[k]     a wave per row, lanes 64 apart, a butterfly
//       s[128 p + i] = sum_k Wt[p][i][k] y[k]                                 likewise
//     then ep_resid = s, ep_chi2 = alpha[I] . s summed in pixel order by one thread (the products staged through LDS),
//     ep_logp; a block that failed to factor gives NaN in the three; an epoch without pixels 0.0, 0.0, 0
//   block n_ep: the pixel outputs, and loo_logp = sum_i pix_logp[i] in pixel order by one thread, chunk by chunk out of LDS
__global__ __launch_bounds__(256) void k_loo_finish(int N, int n_ep, const int* __restrict__ epoch_block,
                                                    const LooBlock* __restrict__ blocks, const double* __restrict__ U,
                                                    const double* __restrict__ Wt, const double* __restrict__ Z, double* sol,
                                                    const MatAcc* __restrict__ acc, const double* __restrict__ alpha,
                                                    const double* __restrict__ diag, const double* __restrict__ fl,
                                                    double* __restrict__ pix_mean, double* __restrict__ pix_var,
                                                    double* __restrict__ pix_logp, double* __restrict__ ep_resid,
                                                    double* __restrict__ ep_chi2, double* __restrict__ ep_logp,
                                                    int* __restrict__ ep_npix, double* __restrict__ loo_logp)
{
    __shared__ double y[NB];
    __shared__ double buf[LOO_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x == n_ep) {
        double total = 0.0;
        for (int c0 = 0; c0 < N; c0 += LOO_CHUNK) {
            const int n = min(LOO_CHUNK, N - c0);
            for (int j = tid; j < n; j += 256) {
                const int i = c0 + j;
                const double Aii = diag[i], a = alpha[i];
                const double lp = 0.5 * log(Aii) - a * a / (2.0 * Aii) - LOO_HALF_LOG_2PI;
                pix_mean[i] = fl[i] - a / Aii;
                pix_var[i] = 1.0 / Aii;
                pix_logp[i] = lp;
                buf[j] = lp;
            }
            __syncthreads();
            if (tid == 0)
                for (int j = 0; j < n; ++j) total += buf[j];
            __syncthreads();
        }
        if (tid == 0) *loo_logp = total;
        return;
    }
    const int e = blockIdx.x, b = epoch_block[e];
    if (b < 0) {
        if (tid == 0) {
            ep_chi2[e] = 0.0;
            ep_logp[e] = 0.0;
            ep_npix[e] = 0;
        }
        return;
    }
    const LooBlock blk = blocks[b];
    const int S = blk.side, Pb = S / NB;
    const double* Ub = U + blk.offset;
    const double* z = Z + blk.rhs;
    double* s = sol + blk.rhs;
    for (int p = Pb - 1; p >= 0; --p) {
        const int r0 = NB * p;
        for (int i = wave; i < NB; i += 4) {
            const double* Ui = Ub + (size_t)(r0 + i) * S;
            double a = 0.0;
            for (int k = r0 + NB + lane; k < S; k += 64) a = fma(Ui[k], s[k], a);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
            if (lane == 0) y[i] = z[r0 + i] - a;
        }
        __syncthreads();
        const double* Wp = Wt + blk.wt + (size_t)p * NB * NB;
        for (int i = wave; i < NB; i += 4) {
            const double* Wi = Wp + (size_t)i * NB;
            double a = fma(Wi[lane], y[lane], Wi[64 + lane] * y[64 + lane]);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
            if (lane == 0) s[r0 + i] = a;
        }
        __syncthreads();      // (s is read back from memory by the other waves: the barrier orders it within the workgroup)
    }
    const MatAcc tot = acc_total(acc + (size_t)b * ACC_ROWS, Pb);
    const bool bad = tot.info != 0.0;
    double chi2 = 0.0;
    for (int c0 = 0; c0 < blk.count; c0 += LOO_CHUNK) {
        const int n = min(LOO_CHUNK, blk.count - c0);
        for (int j = tid; j < n; j += 256) {
            const double sj = s[c0 + j];
            ep_resid[blk.start + c0 + j] = bad ? NAN : sj;
            buf[j] = alpha[blk.start + c0 + j] * sj;
        }
        __syncthreads();
        if (tid == 0)
            for (int j = 0; j < n; ++j) chi2 += buf[j];
        __syncthreads();
    }
    if (tid == 0) {
        // log det A_ee = 2 sum log U_ii (the padding is the identity: nothing from it)
        ep_chi2[e] = bad ? NAN : chi2;
        ep_logp[e] = bad ? NAN : -0.5 * chi2 + tot.logdet_half - blk.count * LOO_HALF_LOG_2PI;
        ep_npix[e] = blk.count;
    }
}

inline hipError_t loo_configure_kernels()
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_loo_band), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)GEMM_LDS_BYTES);
}

// the leave-one-out workspace of a chunk handle (grow-only; psoap_chunk_loo_release frees it)
struct LooWs {
    Grow<double> Blk, Rhs, Sol, Wt, Diag, Pix, EpResid, EpOut, Logp;
    Grow<MatAcc> Acc;
    Grow<LooBlock> Blocks;
    Grow<LooTile> Tiles;
    Grow<int> PixBlock, EpBlock, EpNpix;
};

}  // namespace psoap
