// marg_predict_kernels.hpp -- the component spectra under the marginalised continuum: the conditional of predict_kernels.hpp
// with Kt = K + Ht Ht^T (marg_kernels.hpp) in the place of the data covariance K.  The continuum is not predicted: H enters
// through the data covariance only.
//
//   r = fl - offset, Cx (R x N), A and m0 as the plain mode has them;   mu = m0 + Cx Kt^-1 r,   Sigma = A - Cx Kt^-1 Cx^T
//   K = U^T U,  Wc = U^-T Cx^T (N x R),  Wh = U^-T Ht (N x S, S = 128 Q),  z = U^-T r
//   M = I + Wh^T Wh = U_M^T U_M,  G = Wh^T Wc (S x R),  bt = Wh^T z,  Y = U_M^-T G,  y = U_M^-T bt
//   mu    = m0 + Wc^T z - Y^T y
//   Sigma = A - Wc^T Wc + Y^T Y            (the plain Sigma plus a term of rank <= q that is positive semi-definite)
//   var   = prior - colnorm^2(Wc) + colnorm^2(Y)
// No explicit inverse, no [K | I].
//
//   k_fill_sym, k_fill_region, k_marg_load     K, Cx^T and Ht into [K | Cx^T | Ht] (marg_predict_plan.hpp: the layout)
//   k_marg_panel_update, k_potrf_diag, k_trsm_strip     its staged factorisation; block row p takes K's own columns, all of
//                                Cx^T and the slots of Ht that can be non-zero there
//   k_marg_rhs_partial / _finish   bt, as psoap_chunk_lnlike_marg makes it
//   k_marg_predict_gram          one workgroup per tile of [M | G] in the MFMA accumulators, from the tile's first non-zero
//                                row to Npad; M's diagonal tiles as k_marg_gram writes them
//   k_panel_update, k_potrf_diag, k_trsm_strip on [M | G] with bt as its right-hand side: Y and y fall out of it, as Vt does
//                                for the gradient
//   k_marg_predict_sigma         one workgroup per upper tile of Sigma: one accumulator set, a K loop of depth Npad over Wc, the
//                                sign changed (exact), a K loop of depth S over Y; A + the accumulators, mirrored below
//   k_gemv_t_partial, k_colnorm_partial over Wc and over Y, then k_marg_predict_mean / _var: the slabs in order, the depth-S
//                                sum taken off the mean and added to the variance
// fp64 throughout, no atomics, every sum in an order fixed by (N, c, M, mode, baseline layout).
//
// Workspace: Npad x (Npad + Rpad + S) doubles of [K | Cx^T | Ht] and Rpad^2 of Sigma in the predict workspace, S x (S + Rpad)
// of [M | G] beside the baseline's device side.
#pragma once
#include "marg_kernels.hpp"
#include "marg_predict_plan.hpp"
#include "predict_kernels.hpp"

namespace psoap {

// grid: the tiles of the plan.  Tile g of [M | G] = A_a^T A_b over the rows k0 .. Npad of [K | Cx^T | Ht] (above, one of the
// two strips is exactly zero); a diagonal tile of M gets the identity -- padding diagonal included -- and only its upper
// half is written (all the staged kernels read).
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_marg_predict_gram(const double* __restrict__ A, int ld, int Npad,
                                                                      const MargPredictTile* __restrict__ tiles,
                                                                      double* __restrict__ Mx, int ldm)
{
    const MargPredictTile g = tiles[blockIdx.x];
    const double* W = A + (size_t)g.k0 * ld;
    Tile t;
    t.zero();
    tile_gemm_tn(t, W + NB * g.a, (size_t)ld, W + NB * g.b, (size_t)ld, Npad - g.k0, g.diag != 0);
    // (as in k_marg_gram: no address of the epilogue is computed and kept in registers ahead of the K loop)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    double* Mt = Mx + (size_t)NB * g.row * ldm + NB * g.col;
    const bool diag_tile = g.diag != 0;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = tile_row(wr, m, lane, r), col = tile_col(wc, n, lane);
                if (!diag_tile || row <= col) Mt[(size_t)row * ldm + col] = t.acc[m][n][r] + ((diag_tile && row == col) ? 1.0 : 0.0);
            }
}

// k_syrk_sub_sym with a second K loop: S(ti, tj) += -Wc_ti^T Wc_tj + Y_ti^T Y_tj for the upper tile blockIdx.x + t0, and its
// transpose into S(tj, ti).  The MFMA only adds: the tile changes sign between the loops, which is exact.  The prior A must
// be present in the upper tiles (the lower ones are overwritten); Sigma comes out symmetric bit for bit.
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_marg_predict_sigma(const double* __restrict__ W, size_t ldw, int K,
                                                                       const double* __restrict__ Y, size_t ldy, int Ky,
                                                                       double* __restrict__ S, size_t lds, int St, int t0)
{
    int ti, tj;
    decode_upper(blockIdx.x + t0, St, ti, tj);
    Tile t;
    t.zero();
    tile_gemm_tn(t, W + (size_t)NB * ti, ldw, W + (size_t)NB * tj, ldw, K);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) t.acc[m][n] = -t.acc[m][n];
    tile_gemm_tn(t, Y + (size_t)NB * ti, ldy, Y + (size_t)NB * tj, ldy, Ky);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        double* p0 = S + (size_t)(NB * ti + tile_row(wr, m, lane, 0)) * lds + NB * tj + tile_col(wc, 0, lane);
        double c[4][4];
        tile_load16(p0, (size_t)4 * lds, c);
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = tile_row(wr, m, lane, r), col = tile_col(wc, n, lane);
                const double v = c[n][r] + t.acc[m][n][r];
                p0[(size_t)4 * r * lds + 16 * n] = v;
                if (ti != tj) S[(size_t)(NB * tj + col) * lds + NB * ti + row] = v;
            }
    }
}

// mu[q] = m0[q] + (sum of the slabs of Wc^T z, in order) - (sum of the slabs of Y^T y, in order)
__global__ void k_marg_predict_mean(const double* __restrict__ part_w, int nslab_w, const double* __restrict__ part_y,
                                    int nslab_y, int ncols, const double* __restrict__ m0, double* __restrict__ mu)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ncols) return;
    double sw = 0.0, sy = 0.0;
    for (int k = 0; k < nslab_w; ++k) sw += part_w[(size_t)k * ncols + q];
    for (int k = 0; k < nslab_y; ++k) sy += part_y[(size_t)k * ncols + q];
    mu[q] = m0[q] + (sw - sy);
}

// var[q] = (prior[q] - column norm^2 of Wc) + column norm^2 of Y, the slabs of either in order
__global__ void k_marg_predict_var(const double* __restrict__ part_w, int nslab_w, const double* __restrict__ part_y,
                                   int nslab_y, int ncols, const double* __restrict__ prior, double* __restrict__ var)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ncols) return;
    double sw = 0.0, sy = 0.0;
    for (int k = 0; k < nslab_w; ++k) sw += part_w[(size_t)k * ncols + q];
    for (int k = 0; k < nslab_y; ++k) sy += part_y[(size_t)k * ncols + q];
    var[q] = (prior[q] - sw) + sy;
}

inline hipError_t marg_predict_configure_kernels()
{
    const int lds = (int)GEMM_LDS_BYTES;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_predict_gram),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_predict_sigma), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    return e;
}

// what a call needs beyond the predict workspace and the marginal likelihood's (grow-only; psoap_chunk_marg_release frees
// it with the MargWs it belongs to)
struct MargPredictWs {
    MargPredictPlan plan;                // the last call's: the tile list is copied from here
    Grow<double> Mx, PartY;              // [M | G]; the slabs of the depth-S sums
    Grow<MargPredictTile> Tiles;
    Grow<MatAcc> AccTot;                 // the totals of the two factorisations' records
};

}  // namespace psoap
