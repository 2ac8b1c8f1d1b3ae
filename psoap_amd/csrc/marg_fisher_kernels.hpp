// marg_fisher_kernels.hpp -- Fisher information (fisher_kernels.hpp) and leave-one-out cross-validation (loo_kernels.hpp)
// of the continuum-marginalised likelihood (marg_kernels.hpp): both under Kt = K + Ht Ht^T instead of K.
//
//   F_st = 1/2 tr(Kt^-1 K_s Kt^-1 K_t),   F_mu = 1^T Kt^-1 1
//   A = Kt^-1,  alpha_m = A r:  the pixel and epoch formulas in the header of loo_kernels.hpp with this A and alpha_m
// H does not depend on the hyper-parameters, the rest-frame grids or mu_GP, so dKt = dK: every tangent matrix, contraction
// and leave-one-out formula is the plain one with K^-1 -> Kt^-1 and alpha -> alpha_m.
//
// The staged factorisation of [K | I | Ht] and of [M | Xt] runs exactly as for the marginal gradient
// (marg_grad_kernels.hpp, one matrix) and leaves
//   Wi = U^-T in the I block,  Vt = U_M^-T Wh^T Wi (q' x N, q' = 128 Q) in the appended block of [M | Xt],
//   alpha_m = Wi^T (z - Wh g),  lnp with the bits of psoap_chunk_lnlike_marg,     Kt^-1 = Wi^T Wi - Vt^T Vt.
// What this header adds is the device code that forms Kt^-1 where the plain paths read K^-1:
//   k_marg_fisher_kinv        k_fisher_kinv with a second K loop of depth q' that takes Vt_ti^T Vt_tj off the same accumulators
//                             (as k_marg_grad_contract does: the MFMA only adds, the tile changes sign around the loop, which
//                             is exact); both triangles into the Fisher workspace's K^-1 slot
//   k_marg_loo_band           k_loo_band with the same second loop; the same scatter into the packed epoch blocks
//   k_marg_fisher_v1 / _mu    F_mu = |Wi 1|^2 - |Vt 1|^2: y = Wi 1 from k_fisher_w1 as it is, v = Vt 1 row by row the same way,
//                             the two sums of squares as k_fisher_mu sums them, one subtraction
// k_fisher_tangent_fill, k_fisher_gemm, k_fisher_contract, k_grad_finish, k_fisher_dot, k_loo_pad, k_loo_rhs, the staged
// kernels on the packed blocks and k_loo_finish run unchanged on what these leave.
//
// Padding.  Rows and columns >= N of Kt^-1 must be the identity, as k_fisher_kinv leaves them.  K is the identity there, so
// Wi is; the rows >= N of Ht are zero (k_marg_basis writes pixels only into a cleared buffer) and U^-T does not mix a row
// >= N with any other, so the rows >= N of Wh are zero; column j >= N of Xt = Wh^T Wi is Wh^T e_j = (row j of Wh)^T = 0,
// and the forward substitution with U_M^-T keeps a zero column zero: the columns >= N of Vt are exact zeros and the
// second loop takes nothing off those rows and columns.  The rows >= q of Vt are zero for the same reason (M is the
// identity there and Xt's rows are zero), so v = Vt 1 needs no mask on its rows.
//
// Flops beyond the plain paths (one matrix): 2 N^2 q' for Wh, 2 N^2 q' for Xt (less the zeros), 2 N q'^2 for the Gram matrix
// and Vt, N^2 q' for the second loop over the upper tiles (the band's tiles only for leave-one-out): about 3 N^2 q' on top of
// F_fisher(N, T) = (1 + 4 T) N^3, nothing per tangent.  Workspace: marg_grad_kernels.hpp's for one matrix plus Fisher's three
// Npad^2 matrices or leave-one-out's packed blocks.
// fp64 throughout, no atomics, every sum in an order fixed by (N, c, baseline layout, T).
#pragma once
#include "fisher_kernels.hpp"
#include "loo_kernels.hpp"
#include "marg_grad_kernels.hpp"

namespace psoap {

// the upper tile (ti, tj) of Kt^-1 = Wi^T Wi - Vt^T Vt in the accumulators.  W: row 128 tj of the I block of [K | I | Ht];
// Vt: the appended block of [M | Xt] after its factorisation, S = 128 Q rows of ldm doubles.  A diagonal tile leaves its
// strictly lower quadrant out (never read back).
__device__ __forceinline__ void marg_kinv_tile(Tile& t, const double* __restrict__ W, size_t ld, const double* __restrict__ Vt,
                                               size_t ldm, int S, int K, int ti, int tj)
{
    t.zero();
    tile_gemm_tn(t, W + NB * ti, ld, W + NB * tj, ld, K, ti == tj);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) t.acc[m][n] = -t.acc[m][n];
    tile_gemm_tn(t, Vt + NB * ti, ldm, Vt + NB * tj, ldm, S, ti == tj);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) t.acc[m][n] = -t.acc[m][n];
}

// Kt^-1, both triangles.  grid P (P + 1) / 2: the upper tile (ti, tj) and its mirror image
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_marg_fisher_kinv(const double* __restrict__ A, int ld, int Npad, int P,
                                                                     const double* __restrict__ Mx, int ldm, int S,
                                                                     double* __restrict__ Kinv)
{
    int ti, tj;
    decode_upper(blockIdx.x, P, ti, tj);
    Tile t;
    marg_kinv_tile(t, A + Npad + (size_t)NB * tj * ld, (size_t)ld, Mx + S, (size_t)ldm, S, Npad - NB * tj, ti, tj);
    fisher_kinv_store(t, ti, tj, Npad, Kinv);
}

// the band tiles of Kt^-1 into the packed epoch blocks.  grid: the band tiles of loo_plan.hpp
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_marg_loo_band(const double* __restrict__ A, int ld, int N, int Npad,
                                                                  const double* __restrict__ Mx, int ldm, int S,
                                                                  const LooTile* __restrict__ tiles,
                                                                  const int* __restrict__ pixel_block,
                                                                  const LooBlock* __restrict__ blocks, double* __restrict__ Blk)
{
    const int ti = tiles[blockIdx.x].ti, tj = tiles[blockIdx.x].tj;
    Tile t;
    marg_kinv_tile(t, A + Npad + (size_t)NB * tj * ld, (size_t)ld, Mx + S, (size_t)ldm, S, Npad - NB * tj, ti, tj);
    loo_band_scatter(t, ti, tj, N, pixel_block, blocks, Blk);
}

// v[k] = sum of row k of Vt over its columns q < N: thread j adds every 256th term, the 256 sums meet in a tree (as
// k_fisher_w1).  grid S, 256 threads
__global__ __launch_bounds__(256) void k_marg_fisher_v1(const double* __restrict__ Mx, int ldm, int S, int N,
                                                        double* __restrict__ v)
{
    __shared__ double red[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    const double* Vk = Mx + (size_t)k * ldm + S;
    double s = 0.0;
    for (int q = tid; q < N; q += 256) s += Vk[q];
    const double sum = block_sum_256(red, s);
    if (tid == 0) v[k] = sum;
}

// one workgroup of 256 threads: out = sum_k y[k]^2 - sum_k v[k]^2, each sum as k_fisher_mu makes it
__global__ __launch_bounds__(256) void k_marg_fisher_mu(const double* __restrict__ y, int N, const double* __restrict__ v, int S,
                                                        double* __restrict__ out)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double total[2];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const double* x = pass ? v : y;
        const int n = pass ? S : N;
        double s = 0.0;
        for (int k = tid; k < n; k += 256) s = fma(x[k], x[k], s);
        total[pass] = block_sum_256(red, s);
        __syncthreads();
    }
    if (tid == 0) *out = total[0] - total[1];
}

inline hipError_t marg_fisher_configure_kernels()
{
    const int lds = (int)GEMM_LDS_BYTES;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_fisher_kinv), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_loo_band), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    return e;
}

}  // namespace psoap
