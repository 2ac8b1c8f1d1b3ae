// marg_grad_kernels.hpp -- analytic gradient of the continuum-marginalised likelihood (marg_kernels.hpp): the gradient of
// grad_kernels.hpp under Kt = K + Ht Ht^T instead of K.
//
//   Wi = U^-T (N x N, lower triangular),  Wh = U^-T Ht (N x q'),  z = U^-T r      (K = U^T U, r = fl - mu_GP, q' = 128 Q)
//   M = I + Wh^T Wh = U_M^T U_M,  bt = Wh^T z,  y = U_M^-T bt,  g = U_M^-1 y
//   Kt^-1 = Wi^T Wi - V V^T,   V = Wi^T Wh U_M^-1  (N x q'),      alpha_m = Kt^-1 r = Wi^T (z - Wh g)
//   Q_m = alpha_m alpha_m^T - Kt^-1
// H does not depend on the hyper-parameters, the rest-frame grids or mu_GP, so every derivative is the one in the header of
// grad_kernels.hpp with Q -> Q_m and alpha -> alpha_m.
//
// The tile engine multiplies k-major strips only (gemm_core.hpp: acc += A[k][m] B[k][n]), and the contraction needs V with
// its q' columns as the k index, so V is made and kept TRANSPOSED, Vt = V^T (q' x N), and never by a product from the right:
//   Xt = Wh^T Wi                 k_marg_grad_cross: Q x P tiles, each one K loop over the rows below both operands' zeros
//   Vt = U_M^-T Xt               the forward substitution that factorising [M | Xt] performs on its appended columns: the
//                                library's k_panel_update / k_potrf_diag / k_trsm_strip on M's workspace, ld = q' + Npad,
//                                as predict factors [K | Cx^T]
// (Y = Wh U_M^-1 and V = Wi^T Y would give the same V from right-hand products the engine does not have.)
//
//   k_marg_load, k_grad_init     Ht and I into the appended blocks of [K | I | Ht] (marg_grad_plan.hpp: the layout)
//   k_marg_grad_panel_update     the update of block row p for K's tiles, I_0 .. I_p and the active slots of Ht in one launch;
//                                k_potrf_diag; k_trsm_strip twice (marg_grad_plan.hpp: why)
//   k_marg_rhs_*, k_marg_gram, the staged kernels on [M | Xt], k_marg_finish     as psoap_chunk_lnlike_marg runs them: the
//                                appended columns change no sum that feeds lnp, which comes back with that entry's bits
//   k_marg_grad_resid            z - Wh g, a wave per row, the slots in order
//   k_grad_alpha_partial / _finish   alpha_m, unchanged
//   k_marg_grad_contract<C>      k_grad_contract<C> with a second K loop of depth q' that takes Vt_ti^T Vt_tj off the same
//                                accumulators; the epilogue is grad_contract_epilogue
//   k_marg_tv_grad_contract<C>   the same two K loops under the time-variable kernel of fill_kernels.hpp: the epilogue is
//                                grad_contract_epilogue<C, true> with the handle's times and tau, the record GradTile<true>
//                                (k_tv_grad_finish adds up dlnL/dtau); H does not depend on tau, so Q -> Q_m is all there is
//   k_grad_finish                unchanged
// fp64 throughout, no atomics, every sum in an order fixed by (N, c, baseline layout).
//
// Workspace per matrix: Npad x (2 Npad + q') doubles of [K | I | Ht] (the gradient's buffer) and q' x (q' + Npad) of
// [M | Xt].  Flops per matrix beyond the plain gradient's N^3: 2 N^2 q' for Wh, 2 N^2 q' for Xt (less the zeros),
// 2 N q'^2 for the Gram matrix and Vt, N^2 q' for the second loop of the contraction.
#pragma once
#include "marg_grad_plan.hpp"
#include "marg_kernels.hpp"

namespace psoap {

static_assert(MARG_GRAD_GROUP_MAX == GRAD_GROUP_MAX && MARG_GRAD_WS_BYTES == GRAD_WS_BYTES,
              "marg_grad_plan.hpp restates the bounds of a gradient group");

// k_grad_panel_update for block row k0 of [K | I | Ht]: block x takes tile column marg_grad_update_tile(p, x, P); the K
// loop of I_j starts at row 128 j and that of slot s at row 128 first[s] (a column whose first row is p has nothing above
// it).  grid (P + 1 + active[p], B)
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_marg_grad_panel_update(double* __restrict__ Abase, size_t mat_stride,
                                                                           int ld, int k0, int P, const int* __restrict__ tab)
{
    double* Km = Abase + (size_t)blockIdx.y * mat_stride;
    const int tcol = marg_grad_update_tile(k0 / NB, blockIdx.x, P);
    const int ks = tcol >= 2 * P ? NB * tab[tcol - 2 * P] : (tcol >= P ? NB * (tcol - P) : 0);
    if (ks >= k0) return;
    const int j0 = NB * tcol;
    Tile t;
    t.zero();
    tile_gemm_tn(t, Km + (size_t)ks * ld + k0, (size_t)ld, Km + (size_t)ks * ld + j0, (size_t)ld, k0 - ks);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        double* p0 = Km + (size_t)(k0 + tile_row(wr, m, lane, 0)) * ld + j0 + tile_col(wc, 0, lane);
        double v[4][4];
        tile_load16(p0, (size_t)4 * ld, v);
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) p0[(size_t)4 * r * ld + 16 * n] = v[n][r] - t.acc[m][n][r];
    }
}

// One workgroup per tile of Xt = Wh^T Wi: rows = tile column column[s] of H, columns = pixel tile tj, over the rows from
// 128 max(first[s], tj) on (above, one of the two is exactly zero; nothing to add up: zeros), into the appended block of
// [M | Xt].  grid (Q P, B)
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_marg_grad_cross(const double* __restrict__ Abase, size_t mat_stride, int ld,
                                                                    int Npad, int P, int Q, const int* __restrict__ tab,
                                                                    double* __restrict__ Mbase, size_t m_stride, int ldm)
{
    const int s = blockIdx.x / P, tj = blockIdx.x % P;
    const int k0 = NB * max(tab[marg_tab_first(Q) + s], tj);
    const double* A = Abase + (size_t)blockIdx.y * mat_stride + (size_t)k0 * ld;
    Tile t;
    t.zero();
    tile_gemm_tn(t, A + 2 * Npad + NB * s, (size_t)ld, A + Npad + NB * tj, (size_t)ld, Npad - k0);
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));      // (as in k_marg_gram: no address of the epilogue kept in registers ahead of the K loop)
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    double* X = Mbase + (size_t)blockIdx.y * m_stride + (size_t)NB * tab[marg_tab_column(Q) + s] * ldm + NB * Q + NB * tj;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) X[(size_t)tile_row(wr, m, lane, r) * ldm + tile_col(wc, n, lane)] = t.acc[m][n][r];
}

// zt = z - Wh g: a wave per row, the slots in their order and within a slot lanes 64 apart, a butterfly; a slot whose first
// row lies below the row is neither read nor added.  g counts in the column order of H.  grid (Npad / 4, B), 256 threads
__global__ __launch_bounds__(256) void k_marg_grad_resid(const double* __restrict__ Abase, size_t mat_stride, int ld, int Npad,
                                                         int Q, const int* __restrict__ tab, const double* __restrict__ Z,
                                                         const double* __restrict__ G, double* __restrict__ Zt)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = 4 * blockIdx.x + wave;
    if (i >= Npad) return;
    const double* Wh = Abase + (size_t)b * mat_stride + (size_t)i * ld + 2 * Npad;
    const double* g = G + (size_t)b * (NB * Q);
    double a = 0.0;
    for (int s = 0; s < Q; ++s) {
        if (NB * tab[marg_tab_first(Q) + s] > i) continue;
        const double* gs = g + NB * tab[marg_tab_column(Q) + s];
        a = fma(Wh[NB * s + lane], gs[lane], a);
        a = fma(Wh[NB * s + 64 + lane], gs[64 + lane], a);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
    if (lane == 0) Zt[(size_t)b * Npad + i] = Z[(size_t)b * Npad + i] - a;
}

// k_grad_contract<C> on Kt: after G = Wi_ti^T Wi_tj a second K loop of depth 128 Q takes Vt_ti^T Vt_tj off the same
// accumulators (the MFMA only adds: the tile changes sign around the loop, which is exact), and the epilogue sees the tile
// of Kt^-1.  Vt: the appended block of [M | Xt] after its factorisation.  grid (P (P + 1) / 2, B)
// (k_marg_tv_grad_contract<C> below repeats these lines up to the epilogue call: a change here is a change there.)
template <int C>
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_marg_grad_contract(const double* __restrict__ Abase, size_t mat_stride,
                                                                       int ld, int N, int Npad, int P,
                                                                       const double* __restrict__ lwl,
                                                                       const double* __restrict__ gp,
                                                                       const double* __restrict__ alpha,
                                                                       double* __restrict__ part,
                                                                       const double* __restrict__ Mbase, size_t m_stride,
                                                                       int ldm, int S)
{
    const int b = blockIdx.y;
    int ti, tj;
    decode_upper(blockIdx.x, P, ti, tj);
    const double* W = Abase + (size_t)b * mat_stride + Npad + (size_t)NB * tj * ld;
    Tile t;
    t.zero();
    tile_gemm_tn(t, W + NB * ti, (size_t)ld, W + NB * tj, (size_t)ld, Npad - NB * tj, ti == tj);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) t.acc[m][n] = -t.acc[m][n];
    const double* Vt = Mbase + (size_t)b * m_stride + S;
    tile_gemm_tn(t, Vt + NB * ti, (size_t)ldm, Vt + NB * tj, (size_t)ldm, S, ti == tj);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) t.acc[m][n] = -t.acc[m][n];
    grad_contract_epilogue<C>(t, b, ti, tj, (int)blockIdx.x, N, Npad, P, lwl, gp, alpha, part);
}

// k_marg_grad_contract<C> on Kt = K_tv + Ht Ht^T (psoap_chunk_lnlike_marg_tv_grad): the same two K loops -- the products do not
// know how K was filled -- then grad_contract_epilogue<C, true> with the handle's times and tau (B, C): the argument formed as
// the TV fill forms it, the sum for dlnL/dtau, the GradTile<true> record k_tv_grad_finish reads.  A kernel of its own beside
// the static one, not one body for both: behind a shared inlined body k_marg_grad_contract<C> came out with other
// instructions than it has alone (profiles/marg_timevar.md; k_fill_sym did the same, profiles/timevar_fold.md).
template <int C>
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_marg_tv_grad_contract(const double* __restrict__ Abase, size_t mat_stride,
                                                                          int ld, int N, int Npad, int P,
                                                                          const double* __restrict__ lwl,
                                                                          const double* __restrict__ times,
                                                                          const double* __restrict__ gp,
                                                                          const double* __restrict__ tau,
                                                                          const double* __restrict__ alpha,
                                                                          double* __restrict__ part,
                                                                          const double* __restrict__ Mbase, size_t m_stride,
                                                                          int ldm, int S)
{
    const int b = blockIdx.y;
    int ti, tj;
    decode_upper(blockIdx.x, P, ti, tj);
    const double* W = Abase + (size_t)b * mat_stride + Npad + (size_t)NB * tj * ld;
    Tile t;
    t.zero();
    tile_gemm_tn(t, W + NB * ti, (size_t)ld, W + NB * tj, (size_t)ld, Npad - NB * tj, ti == tj);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) t.acc[m][n] = -t.acc[m][n];
    const double* Vt = Mbase + (size_t)b * m_stride + S;
    tile_gemm_tn(t, Vt + NB * ti, (size_t)ldm, Vt + NB * tj, (size_t)ldm, S, ti == tj);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) t.acc[m][n] = -t.acc[m][n];
    grad_contract_epilogue<C, true>(t, b, ti, tj, (int)blockIdx.x, N, Npad, P, lwl, gp, alpha, part, times, tau);
}

inline hipError_t marg_grad_configure_kernels()
{
    const int lds = (int)GEMM_LDS_BYTES;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_grad_panel_update),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_grad_cross), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_grad_contract<1>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_grad_contract<2>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_grad_contract<3>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_tv_grad_contract<1>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_tv_grad_contract<2>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_tv_grad_contract<3>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    return e;
}

// the workspace of the marginal gradient beyond the gradient's and the marginal likelihood's (grow-only;
// psoap_chunk_marg_release frees it with the MargWs it belongs to)
struct MargGradWs {
    Grow<double> Mx, Zt;      // [M | Xt] per matrix; z - Wh g
};

}  // namespace psoap
