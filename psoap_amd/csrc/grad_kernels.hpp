// grad_kernels.hpp -- analytic gradient of the GP log-likelihood (not in the reference, which only evaluates it).
//
//   lnL = -1/2 (r^T K^-1 r + log det K),  r = fl - mu_GP                     (covariance.py:329-331)
//   K_ij = sum_c a_c^2 exp(p_c d_cij^2) + sigma_i^2 delta_ij,  d_cij = x_c[j] - x_c[i],  p_c = -1/2 c_kms^2 / l_c^2
// With alpha = K^-1 r, Q = alpha alpha^T - K^-1 and e_cij = exp(p_c d_cij^2):
//   dlnL/da_c    = a_c sum_ij Q_ij e_cij
//   dlnL/dl_c    = 1/2 a_c^2 c_kms^2 / l_c^3 sum_ij Q_ij e_cij d_cij^2
//   dlnL/dx_c[i] = -2 p_c a_c^2 sum_j Q_ij e_cij d_cij
//   dlnL/dmu_GP  = sum_i alpha_i
//
// The staged left-looking factorisation (chol_kernels.hpp) runs on [K | I], an Npad x 2 Npad workspace per matrix: predict's
// augmented layout (predict_kernels.hpp) with Cx^T = I.  Afterwards the appended block holds W = U^-T, K^-1 = W^T W,
// r holds z = U^-T r, and alpha = W^T z.  W is lower triangular -- column tile j is zero above row 128 j -- and nothing
// above that row is ever read or written: block row p updates and solves the appended tiles j <= p only (tile columns
// p .. P + p of the workspace are contiguous, so the likelihood's kernels take them in one launch), and every K loop over
// column tile j starts at row 128 j.  Factor, solve and contraction cost N^3/3 flops each.
//
// K^-1 is never stored: k_grad_contract forms one 128 x 128 tile of W^T W in the MFMA accumulators and contracts it with
// the covariance derivatives in its epilogue.  Every sum runs in a fixed order and no kernel uses an atomic: two calls
// with the same arguments return the same bits, whatever the batch around a matrix.
#pragma once
#include "chol_kernels.hpp"
#include "fill_kernels.hpp"

namespace psoap {

// doubles per tile in the partial-sum workspace: row sums [3][128], column sums [3][128], 2 x 3 hyper-parameter sums (+ 2)
constexpr int GRAD_ROWS_OFF = 0, GRAD_COLS_OFF = 3 * NB, GRAD_HYP_OFF = 6 * NB, GRAD_TILE_DOUBLES = 6 * NB + 8;

__host__ __device__ inline int upper_index(int ti, int tj, int P) { return ti * P - ti * (ti - 1) / 2 + (tj - ti); }

// The appended block of [K | I], lower tiles only (tr >= tc): zeros, ones on the diagonal.  grid (P (P + 1) / 2, B)
__global__ __launch_bounds__(256) void k_grad_init(double* __restrict__ Abase, size_t mat_stride, int ld, int Npad, int P)
{
    int tc, tr;
    decode_upper(blockIdx.x, P, tc, tr);
    double* W = Abase + (size_t)blockIdx.y * mat_stride + Npad;
    const int col2 = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    for (int r = r0; r < NB; r += 4) {
        d2 v;
        v.x = (tr == tc && r == 2 * col2) ? 1.0 : 0.0;
        v.y = (tr == tc && r == 2 * col2 + 1) ? 1.0 : 0.0;
        *reinterpret_cast<d2*>(W + (size_t)(NB * tr + r) * ld + NB * tc + 2 * col2) = v;
    }
}

// k_panel_update for block row k0 of [K | I]: tile columns p .. P + p (grid.x = P + 1); the K loop of appended tile j
// starts at row 128 j, below the structural zeros (tile j == p has nothing above it: left as it is).
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_grad_panel_update(double* __restrict__ Abase, size_t mat_stride, int ld,
                                                                      int k0, int P)
{
    double* Km = Abase + (size_t)blockIdx.y * mat_stride;
    const int tcol = k0 / NB + blockIdx.x;
    const int ks = tcol >= P ? NB * (tcol - P) : 0;
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

// alpha = W^T z in two fixed-order stages.  partial[b][s][q] = sum over the rows k of slab s (256 rows) of W[k][q] z[k],
// from the column's first non-zero row on; slabs wholly above it are neither written nor read.  grid (P, nslab, B)
__global__ __launch_bounds__(256) void k_grad_alpha_partial(const double* __restrict__ Abase, size_t mat_stride, int ld,
                                                            int Npad, const double* __restrict__ Z,
                                                            double* __restrict__ partial, int nslab)
{
    __shared__ double red[NB];
    const int b = blockIdx.z, tq = blockIdx.x, s = blockIdx.y;
    const int col = threadIdx.x & 127, half = threadIdx.x >> 7;
    const int kend = min(256 * (s + 1), Npad);
    if (kend <= NB * tq) return;
    const int kbeg = max(256 * s, NB * tq);
    const double* W = Abase + (size_t)b * mat_stride + Npad + NB * tq + col;
    const double* z = Z + (size_t)b * Npad;
    double acc = 0.0;
    for (int k = kbeg + half; k < kend; k += 2) acc = fma(W[(size_t)k * ld], z[k], acc);
    if (half == 1) red[col] = acc;
    __syncthreads();
    if (half == 0) partial[((size_t)b * nslab + s) * Npad + NB * tq + col] = acc + red[col];
}

__global__ void k_grad_alpha_finish(const double* __restrict__ partial, int nslab, int Npad, double* __restrict__ alpha)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (q >= Npad) return;
    double s = 0.0;
    for (int k = (q / NB * NB) / 256; k < nslab; ++k) s += partial[((size_t)b * nslab + k) * Npad + q];
    alpha[(size_t)b * Npad + q] = s;
}

// One workgroup per upper tile (ti <= tj) of Q = alpha alpha^T - W^T W.  G = W_ti^T W_tj over the rows from 128 tj on
// (everything above is exactly zero), then per element the lane holds: q = alpha_i alpha_j - G_ij, e_c = exp(p_c d^2) as the
// fills evaluate it (exp_nonpos_batch and the wave-uniform underflow shortcut), and the sums
//   hyper-parameters  sum w q e_c, sum w q e_c d^2   (w = 2: the element stands for (i,j) and (j,i); 1 on the diagonal)
//   rows of block ti  sum_j q e_c d;     rows of block tj  -sum_i q e_c d   (the mirrored element has -d)
// A diagonal tile takes i <= j only; rows and columns >= N are masked.  The components are walked one after the other
// (the accumulators leave few registers), the tile's sums meet in LDS -- the operand buffers of the product, free by then --
// in a fixed order, and the workgroup stores them to its own GRAD_TILE_DOUBLES of `part`.
// The epilogue: everything after the product, on the tile t = (K^-1)[ti][tj] in the accumulators (one function, two callers:
// k_grad_contract below and k_marg_grad_contract of marg_grad_kernels.hpp, whose t is the tile of (K + Ht Ht^T)^-1).
template <int C>
__device__ __forceinline__ void grad_contract_epilogue(const Tile& t, int b, int ti, int tj, int tile_index, int N, int Npad,
                                                       int P, const double* __restrict__ lwl, const double* __restrict__ gp,
                                                       const double* __restrict__ alpha, double* __restrict__ part)
{
    constexpr int XS = 0;                 // [2][3][NB]: abscissae of the tile's rows (side 0) and columns (side 1)
    constexpr int AL = XS + 6 * NB;       // [2][NB]: alpha likewise
    constexpr int RS = AL + 2 * NB;       // [2 wc][3][NB]: row sums of the two wave columns
    constexpr int CS = RS + 6 * NB;       // [2 wr][3][NB]: column sums of the two wave rows
    constexpr int HS = CS + 6 * NB;       // [4 waves][6]
    static_assert((HS + 24) * sizeof(double) <= GEMM_LDS_BYTES, "the epilogue fits the operand buffers");
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const double* lw = lwl + (size_t)b * C * N;
    {
        const int side = tid >> 7, idx = tid & 127;
        const int g = NB * (side ? tj : ti) + idx;
#pragma unroll
        for (int c = 0; c < C; ++c) psoap_smem[XS + (side * 3 + c) * NB + idx] = (g < N) ? lw[(size_t)c * N + g] : 0.0;
        psoap_smem[AL + side * NB + idx] = alpha[(size_t)b * Npad + g];
    }
    __syncthreads();
    const bool diag_tile = ti == tj;
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        double p2;
        {
#pragma clang fp contract(off)
            const double l = gp[(size_t)b * 2 * C + 2 * c + 1];      // (as load_gp rounds it)
            p2 = -0.5 * (C_KMS * C_KMS) / (l * l);
        }
        double xj[4], aj[4], colacc[4];
        bool jok[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int col = tile_col(wc, n, lane);
            xj[n] = psoap_smem[XS + (3 + c) * NB + col];
            aj[n] = psoap_smem[AL + NB + col];
            jok[n] = NB * tj + col < N;
            colacc[n] = 0.0;
        }
        double sa = 0.0, sl = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            double xi[4], ai[4], rowacc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = tile_row(wr, m, lane, r);
                xi[r] = psoap_smem[XS + c * NB + row];
                ai[r] = psoap_smem[AL + row];
                rowacc[r] = 0.0;
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int col = tile_col(wc, n, lane);
                double d[4], a[4], e[4];
                bool live = false;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma clang fp contract(off)
                    d[r] = xj[n] - xi[r];
                    a[r] = p2 * d[r] * d[r];
                    live = live || !(a[r] <= -746.0);
                }
                if (__builtin_amdgcn_ballot_w64(live) == 0ull) continue;      // exp() = +0 for the whole wave: nothing to add
                exp_nonpos_batch<4>(a, e);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = tile_row(wr, m, lane, r);
                    const bool ok = jok[n] && NB * ti + row < N && (!diag_tile || row <= col);
                    const double qe = ok ? (ai[r] * aj[n] - t.acc[m][n][r]) * e[r] : 0.0;
                    const double w = (diag_tile && row == col) ? 1.0 : 2.0;
                    const double qed = qe * d[r];
                    sa = fma(w, qe, sa);
                    sl = fma(w * qed, d[r], sl);
                    rowacc[r] += qed;
                    colacc[n] -= qed;
                }
            }
            // the row's 16 lanes (lane & 15 = column within the block), then the two wave columns in LDS
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int off = 1; off <= 8; off <<= 1) rowacc[r] += __shfl_xor(rowacc[r], off, 64);
                if ((lane & 15) == 0) psoap_smem[RS + (wc * 3 + c) * NB + tile_row(wr, m, lane, r)] = rowacc[r];
            }
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            colacc[n] += __shfl_xor(colacc[n], 16, 64);
            colacc[n] += __shfl_xor(colacc[n], 32, 64);
            if (lane < 16) psoap_smem[CS + (wr * 3 + c) * NB + tile_col(wc, n, lane)] = colacc[n];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            sa += __shfl_xor(sa, off, 64);
            sl += __shfl_xor(sl, off, 64);
        }
        if (lane == 0) {
            psoap_smem[HS + wave * 6 + 2 * c] = sa;
            psoap_smem[HS + wave * 6 + 2 * c + 1] = sl;
        }
    }
    __syncthreads();
    double* out = part + ((size_t)b * (P * (P + 1) / 2) + tile_index) * GRAD_TILE_DOUBLES;
    {
        const int side = tid >> 7, idx = tid & 127;
        const int src = side ? CS : RS;
#pragma unroll
        for (int c = 0; c < C; ++c)
            out[(side ? GRAD_COLS_OFF : GRAD_ROWS_OFF) + c * NB + idx] =
                psoap_smem[src + c * NB + idx] + psoap_smem[src + (3 + c) * NB + idx];
    }
    if (tid < 2 * C)
        out[GRAD_HYP_OFF + tid] = ((psoap_smem[HS + tid] + psoap_smem[HS + 6 + tid]) + psoap_smem[HS + 12 + tid]) +
                                  psoap_smem[HS + 18 + tid];
}

template <int C>
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_grad_contract(const double* __restrict__ Abase, size_t mat_stride,
                                                                  int ld, int N, int Npad, int P,
                                                                  const double* __restrict__ lwl,
                                                                  const double* __restrict__ gp,
                                                                  const double* __restrict__ alpha,
                                                                  double* __restrict__ part)
{
    const int b = blockIdx.y;
    int ti, tj;
    decode_upper(blockIdx.x, P, ti, tj);
    const double* W = Abase + (size_t)b * mat_stride + Npad + (size_t)NB * tj * ld;
    Tile t;
    t.zero();
    tile_gemm_tn(t, W + NB * ti, (size_t)ld, W + NB * tj, (size_t)ld, Npad - NB * tj, ti == tj);
    grad_contract_epilogue<C>(t, b, ti, tj, (int)blockIdx.x, N, Npad, P, lwl, gp, alpha, part);
}

// The tiles' partial sums in tile order.  grid (P + 1, B), 128 threads.
//   blocks x < P:  grad_x[b][c][128 x + i]: the column sums of tiles (ti, x), ti <= x, then the row sums of tiles (x, tj), tj >= x
//   block  x == P: grad_gp[b][2C] and grad_mu[b] = sum_i alpha_i: thread k adds every 128th term, the 128 sums meet in a tree
__global__ __launch_bounds__(128) void k_grad_finish(const double* __restrict__ part, const double* __restrict__ alpha,
                                                     const double* __restrict__ gp, int C, int N, int Npad, int P,
                                                     double* __restrict__ grad_gp, double* __restrict__ grad_x,
                                                     double* __restrict__ grad_mu)
{
    __shared__ double red[128];
    const int b = blockIdx.y, x = blockIdx.x, tid = threadIdx.x;
    const int ntiles = P * (P + 1) / 2;
    const double* pb = part + (size_t)b * ntiles * GRAD_TILE_DOUBLES;
    const double* gpb = gp + (size_t)b * 2 * C;
    if (x < P) {
        const int i = NB * x + tid;
        for (int c = 0; c < C; ++c) {
            double s = 0.0;
            for (int ti = 0; ti <= x; ++ti) s += pb[(size_t)upper_index(ti, x, P) * GRAD_TILE_DOUBLES + GRAD_COLS_OFF + c * NB + tid];
            for (int tj = x; tj < P; ++tj) s += pb[(size_t)upper_index(x, tj, P) * GRAD_TILE_DOUBLES + GRAD_ROWS_OFF + c * NB + tid];
            const double a = gpb[2 * c], l = gpb[2 * c + 1];
            const double p2 = -0.5 * (C_KMS * C_KMS) / (l * l);
            if (i < N) grad_x[((size_t)b * C + c) * N + i] = -2.0 * p2 * (a * a) * s;
        }
        return;
    }
    for (int k = 0; k <= 2 * C; ++k) {
        double s = 0.0;
        if (k < 2 * C) {
            for (int t = tid; t < ntiles; t += 128) s += pb[(size_t)t * GRAD_TILE_DOUBLES + GRAD_HYP_OFF + k];
        } else {
            for (int i = tid; i < N; i += 128) s += alpha[(size_t)b * Npad + i];
        }
        __syncthreads();
        red[tid] = s;
        __syncthreads();
        for (int w = 64; w >= 1; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0) {
            if (k == 2 * C) {
                grad_mu[b] = red[0];
            } else {
                const double a = gpb[k & ~1], l = gpb[k | 1];
                grad_gp[(size_t)b * 2 * C + k] = (k & 1) ? 0.5 * (a * a) * (C_KMS * C_KMS) / (l * l * l) * red[0] : a * red[0];
            }
        }
    }
}

inline hipError_t grad_configure_kernels()
{
    const int lds = (int)GEMM_LDS_BYTES;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_grad_panel_update),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_grad_contract<1>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_grad_contract<2>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_grad_contract<3>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    return e;
}

// Matrices per group of a gradient call: a call with more proposals walks them group after group through ONE workspace,
// which is therefore bounded whatever B is -- at most GRAD_GROUP_MAX matrices and (beyond one matrix) GRAD_WS_BYTES of
// [K | I] storage: 16 Npad^2 bytes per matrix (579 MB at N = 6000).
constexpr int GRAD_GROUP_MAX = 8;
constexpr size_t GRAD_WS_BYTES = (size_t)1 << 30;

inline int grad_group_size(int B, int Npad)
{
    const size_t per = sizeof(double) * 2 * (size_t)Npad * Npad;
    size_t g = GRAD_WS_BYTES / per;
    if (g < 1) g = 1;
    if (g > (size_t)GRAD_GROUP_MAX) g = GRAD_GROUP_MAX;
    return B < (int)g ? B : (int)g;
}

// the gradient workspace of a chunk handle (grow-only; psoap_chunk_grad_release frees it)
struct GradWs {
    Grow<double> A, Wt, R, Lwl, Gp, Alpha, APart, Part, Out, GradGp, GradX, GradMu;
    Grow<MatAcc> Acc;
    // psoap_chunk_lnprob_grad (orbit_grad_kernels.hpp): the group's orbital parameters, velocities, Jacobian, dlnL/dv and
    // dlnL/dp_orb, its |v| >= c flags, and the pixels of every epoch (valid until the next psoap_chunk_set_grid)
    Grow<double> Porb, Vel, Jac, Gv, GradOrb;
    Grow<int> TooFast, EpStart, EpPix;
    bool epochs_valid = false;
    // psoap_chunk_lnlike_tv_grad (timevar_kernels.hpp): the group's time scales and dlnL/dtau
    Grow<double> Tau, GradTau;
};

}  // namespace psoap
