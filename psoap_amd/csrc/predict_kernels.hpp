// predict_kernels.hpp -- GP conditional mean / covariance (the predict_* family).
//
// Reference (psoap/covariance.py): predict_f :25-54, predict_f_g :81-148,
// predict_f_g_sum :151-187, predict_f_g_h :190-251, predict_f_g_h_sum :253-297.
//
// All of them are   mu = m0 + Cx B^-1 (fl - off),   Sigma = A - Cx B^-1 Cx^T
// with B the noisy data covariance.  On the device B = U^T U is factored by the same
// left-looking kernels as the likelihood, with Cx^T appended to B as extra column tiles
// ([B | Cx^T], Npad x (Npad + Rpad)): the panel update and the strip solve then turn those
// columns into W = U^-T Cx^T in place, the right-hand side r = fl - off becomes z = U^-T r,
// and
//     mu = m0 + W^T z            (k_gemv_t, deterministic two-stage reduction)
//     Sigma = A - W^T W          (k_syrk_sub, fp64 MFMA tiles, K = Npad)
// so no explicit inverse or second triangular solve is needed.  The kernels and their launch helpers are here; the
// arithmetic of a call is predict_plan.hpp's, the host side predict_host.hpp's.
#pragma once

#include "chol_kernels.hpp"
#include "dag_kernel.hpp"
#include "dag_launch.hpp"
#include "fill_kernels.hpp"

namespace psoap {

struct GpHost {
    double v[6];
};

// out[i][col0 + j] = sum_{c<C} a_c^2 exp(p_c (xcol_c[j] - xrow_c[i])^2),  i < nrows, j < ncols
// (fill_V12_f semantics, pyx:61-96, summed over components left to right as the reference
// sums V12_f + V12_g (+ V12_h), covariance.py:171,279).  With sym_diag the i == j entries
// follow the fill_V11_f diagonal rule plus `nugget` (pyx:56-57; covariance.py:165).
// Scalar stores: column offsets in the predict layout are not 16-byte aligned.
template <int C>
__global__ __launch_bounds__(256) void k_fill_region(double* __restrict__ out, size_t ld, int col0, int nrows,
                                                     int ncols, const double* __restrict__ xrow, size_t xrow_stride,
                                                     const double* __restrict__ xcol, size_t xcol_stride, GpHost gph,
                                                     int sym_diag, double nugget)
{
    __shared__ double xr[C][NB];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.y * NB, j0 = blockIdx.x * NB;
    GpDev g;
    load_gp(gph.v, C, g);
    double dsum = g.a2[0];
    {
#pragma clang fp contract(off)
        for (int c = 1; c < C; ++c) dsum = dsum + g.a2[c];
    }
    if (tid < NB) {
#pragma unroll
        for (int c = 0; c < C; ++c) xr[c][tid] = (i0 + tid < nrows) ? xrow[c * xrow_stride + i0 + tid] : 0.0;
    }
    const int col = tid & 127, half = tid >> 7;
    const int j = j0 + col;
    double xj[C];
#pragma unroll
    for (int c = 0; c < C; ++c) xj[c] = (j < ncols) ? xcol[c * xcol_stride + j] : 0.0;
    __syncthreads();
    if (j >= ncols) return;
    for (int it = 0; it < NB / 2; ++it) {
        const int r = half + 2 * it;
        const int i = i0 + r;
        if (i >= nrows) break;
        double xi[C];
#pragma unroll
        for (int c = 0; c < C; ++c) xi[c] = xr[c][r];
        double v = kern_elem<C>(xi, xj, g);
        if (sym_diag && i == j) {
#pragma clang fp contract(off)
            v = dsum + nugget;
        }
        out[(size_t)i * ld + col0 + j] = v;
    }
}

// the time scales of the components a region launch evaluates, as GpHost carries their hyper-parameters
struct TauHost {
    double v[3];
};

// k_fill_region under the time-variable kernel (fill_kernels.hpp, `TV`): trow (nrows) and tcol (ncols) are the times of
// the rows and the columns in days -- ONE vector each, shared by the components --, tauh the components' time scales:
//   out[i][col0 + j] = sum_{c<C} a_c^2 exp(p_c (xcol_c[j] - xrow_c[i])^2 + q_c (tcol[j] - trow[i])^2),   q_c = tv_q2(tau_c)
// The argument is formed as every time-variable kernel forms it -- a = p * d * d, then a = a + q * dt * dt, no contraction,
// one exp -- so with tau_c = +inf (q = -0) the bits are k_fill_region's.  The sym_diag / nugget branch is k_fill_region's
// (dt = 0 there).  The tiling and the element-wise stores are k_fill_region's too: a body shared with the static fill
// changed that fill's instructions and the predict family is pinned bit for bit, so the two kernels stand
// side by side as k_fill_sym_tv and k_fill_sym do -- a change to the region's shape is made in BOTH.
template <int C>
__global__ __launch_bounds__(256) void k_fill_region_tv(double* __restrict__ out, size_t ld, int col0, int nrows, int ncols,
                                                        const double* __restrict__ xrow, size_t xrow_stride,
                                                        const double* __restrict__ xcol, size_t xcol_stride,
                                                        const double* __restrict__ trow, const double* __restrict__ tcol,
                                                        GpHost gph, TauHost tauh, int sym_diag, double nugget)
{
    __shared__ double xr[C][NB];
    __shared__ double tr[NB];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.y * NB, j0 = blockIdx.x * NB;
    GpDev g;
    load_gp(gph.v, C, g);
    double q2[C];
#pragma unroll
    for (int c = 0; c < C; ++c) q2[c] = tv_q2(tauh.v[c]);
    double dsum = g.a2[0];
    {
#pragma clang fp contract(off)
        for (int c = 1; c < C; ++c) dsum = dsum + g.a2[c];
    }
    if (tid < NB) {
#pragma unroll
        for (int c = 0; c < C; ++c) xr[c][tid] = (i0 + tid < nrows) ? xrow[c * xrow_stride + i0 + tid] : 0.0;
        tr[tid] = (i0 + tid < nrows) ? trow[i0 + tid] : 0.0;
    }
    const int col = tid & 127, half = tid >> 7;
    const int j = j0 + col;
    double xj[C];
#pragma unroll
    for (int c = 0; c < C; ++c) xj[c] = (j < ncols) ? xcol[c * xcol_stride + j] : 0.0;
    const double tj = (j < ncols) ? tcol[j] : 0.0;
    __syncthreads();
    if (j >= ncols) return;
    for (int it = 0; it < NB / 2; ++it) {
        const int r = half + 2 * it;
        const int i = i0 + r;
        if (i >= nrows) break;
        const double dt = tj - tr[r];
        double v = 0.0;
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double d = xj[c] - xr[c][r];
                double a = g.p2[c] * d * d;
                a = a + q2[c] * dt * dt;
                const double t = g.a2[c] * exp(a);
                v = (c == 0) ? t : v + t;
            }
        }
        if (sym_diag && i == j) {
#pragma clang fp contract(off)
            v = dsum + nugget;
        }
        out[(size_t)i * ld + col0 + j] = v;
    }
}

// S tile (ti, tj) -= sum_k W[k][128 ti + .] W[k][128 tj + .]   (all tiles; calibration's pass 1 / 2)
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_syrk_sub(const double* __restrict__ W, size_t ldw, int K,
                                                             double* __restrict__ S, size_t lds)
{
    const int ti = blockIdx.y, tj = blockIdx.x;
    Tile t;
    t.zero();
    tile_gemm_tn(t, W + (size_t)NB * ti, ldw, W + (size_t)NB * tj, ldw, K);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        double* p0 = S + (size_t)(NB * ti + tile_row(wr, m, lane, 0)) * lds + NB * tj + tile_col(wc, 0, lane);
        double v[4][4];
        tile_load16(p0, (size_t)4 * lds, v);
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) p0[(size_t)4 * r * lds + 16 * n] = v[n][r] - t.acc[m][n][r];
    }
}

// Symmetric form for predict's Sigma = A - W^T W (returned in full, covariance.py:143,251): one workgroup
// per UPPER tile (ti <= tj) computes S(ti, tj) -= W_ti^T W_tj and also writes its transpose into
// S(tj, ti), so the product costs N R^2 / 2 MFMA flops instead of N R^2 and Sigma is bitwise symmetric.
// The prior A must be present in the upper tiles (the lower ones are overwritten).
// t0: index of the launch's first upper tile (row-major over the upper triangle): the Sigma download streams by tile
// rows, so the product is launched in groups of tile rows, top to bottom -- rows < r of Sigma are final once the
// tile rows < r are done (their lower parts were mirrored in by the rows above).
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_syrk_sub_sym(const double* __restrict__ W, size_t ldw, int K,
                                                                 double* __restrict__ S, size_t lds, int St, int t0)
{
    int ti, tj;
    decode_upper(blockIdx.x + t0, St, ti, tj);
    Tile t;
    t.zero();
    tile_gemm_tn(t, W + (size_t)NB * ti, ldw, W + (size_t)NB * tj, ldw, K);
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
                const double v = c[n][r] - t.acc[m][n][r];
                p0[(size_t)4 * r * lds + 16 * n] = v;
                if (ti != tj) S[(size_t)(NB * tj + col) * lds + NB * ti + row] = v;
            }
    }
}

// partial[s][q] = sum_{k in slab s} W[k][q] z[k];  slabs of 256 rows, 128 columns per block
__global__ __launch_bounds__(256) void k_gemv_t_partial(const double* __restrict__ W, size_t ldw, int K, int ncols,
                                                        const double* __restrict__ z, double* __restrict__ partial)
{
    __shared__ double red[128];
    const int col = threadIdx.x & 127, half = threadIdx.x >> 7;
    const int q = blockIdx.x * 128 + col;
    const int k0 = blockIdx.y * 256;
    double s = 0.0;
    if (q < ncols) {
        for (int k = k0 + half; k < k0 + 256 && k < K; k += 2) s = fma(W[(size_t)k * ldw + q], z[k], s);
    }
    if (half == 1) red[col] = s;
    __syncthreads();
    if (half == 0 && q < ncols) partial[(size_t)blockIdx.y * ncols + q] = s + red[col];
}

__global__ void k_gemv_finish(const double* __restrict__ partial, int nslab, int ncols,
                              const double* __restrict__ m0, double* __restrict__ mu)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ncols) return;
    double s = 0.0;
    for (int k = 0; k < nslab; ++k) s += partial[(size_t)k * ncols + q];
    mu[q] = m0[q] + s;
}

// diag(Sigma) alone, for callers that only take sqrt(diag) (scripts/psoap_retrieve_ST3.py:111):
//   var[q] = prior[q] - sum_k W[k][q]^2,  partial sums over slabs of 256 rows in a fixed order
__global__ __launch_bounds__(256) void k_colnorm_partial(const double* __restrict__ W, size_t ldw, int K, int ncols,
                                                         double* __restrict__ partial)
{
    __shared__ double red[128];
    const int col = threadIdx.x & 127, half = threadIdx.x >> 7;
    const int q = blockIdx.x * 128 + col;
    const int k0 = blockIdx.y * 256;
    double s = 0.0;
    if (q < ncols) {
        for (int k = k0 + half; k < k0 + 256 && k < K; k += 2) {
            const double w = W[(size_t)k * ldw + q];
            s = fma(w, w, s);
        }
    }
    if (half == 1) red[col] = s;
    __syncthreads();
    if (half == 0 && q < ncols) partial[(size_t)blockIdx.y * ncols + q] = s + red[col];
}

__global__ void k_var_finish(const double* __restrict__ partial, int nslab, int ncols, const double* __restrict__ prior,
                             double* __restrict__ var)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ncols) return;
    double s = 0.0;
    for (int k = 0; k < nslab; ++k) s += partial[(size_t)k * ncols + q];
    var[q] = prior[q] - s;
}

__global__ void k_zero(double* __restrict__ p, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = 0.0;
}

inline hipError_t predict_configure_kernels()
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_syrk_sub),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEMM_LDS_BYTES);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_syrk_sub_sym),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEMM_LDS_BYTES);
    if (e == hipSuccess) e = dag_set_lds<true, false>();
    return e;
}

template <int C>
static void launch_region(hipStream_t st, double* out, size_t ld, int col0, int nrows, int ncols, const double* xrow,
                          size_t xrs, const double* xcol, size_t xcs, const GpHost& g, int sym, double nug)
{
    dim3 grid((ncols + NB - 1) / NB, (nrows + NB - 1) / NB);
    hipLaunchKernelGGL(k_fill_region<C>, grid, dim3(256), 0, st, out, ld, col0, nrows, ncols, xrow, xrs, xcol, xcs, g,
                       sym, nug);
}

static void launch_region_c(hipStream_t st, int C, double* out, size_t ld, int col0, int nrows, int ncols,
                            const double* xrow, size_t xrs, const double* xcol, size_t xcs, const GpHost& g, int sym,
                            double nug)
{
    with_components(C, [&](auto nc) { launch_region<nc()>(st, out, ld, col0, nrows, ncols, xrow, xrs, xcol, xcs, g, sym, nug); });
}

// launch_region_c for k_fill_region_tv: the same grid
static void launch_region_tv_c(hipStream_t st, int C, double* out, size_t ld, int col0, int nrows, int ncols, const double* xrow,
                               size_t xrs, const double* xcol, size_t xcs, const double* trow, const double* tcol, const GpHost& g,
                               const TauHost& tau, int sym, double nug)
{
    dim3 grid((ncols + NB - 1) / NB, (nrows + NB - 1) / NB);
    with_components(C, [&](auto nc) {
        hipLaunchKernelGGL(k_fill_region_tv<nc()>, grid, dim3(256), 0, st, out, ld, col0, nrows, ncols, xrow, xrs, xcol, xcs, trow,
                           tcol, g, tau, sym, nug);
    });
}

}  // namespace psoap
