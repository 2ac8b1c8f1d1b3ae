// marg_kernels.hpp -- the GP likelihood with a per-epoch continuum polynomial integrated out (not in the reference, whose
// cycle_calibration fits and freezes one; Rasmussen & Williams 2.7, explicit basis functions with a Gaussian prior).
//
//   r = fl - mu_GP = H beta + f + eps,   beta ~ N(0, Lambda),   K as the likelihood builds it (noise on the diagonal)
//   H[i][e (order + 1) + k] = w[i] T_k(u_i) for the pixels i of epoch e, else 0;  Lambda = diag(s_k^2), the same for every epoch
//   Ht = H Lambda^1/2,   W = U^-T Ht,   z = U^-T r   (K = U^T U),   M = I + W^T W,   bt = W^T z
//   lnL = -1/2 (z^T z - bt^T M^-1 bt + log det K + log det M)          (no N/2 log 2 pi: the convention of grad_kernels.hpp:3)
//   E[beta] = Lambda^1/2 M^-1 bt,   Cov[beta] = Lambda^1/2 M^-1 Lambda^1/2,   corrected flux = fl - H E[beta]
//
//   k_marg_basis          Ht, once per psoap_chunk_set_baseline, into a buffer of the handle (Npad x 128 Q, zero elsewhere)
//   k_marg_load           Ht into the appended block of every matrix's [K | Ht] workspace, from each tile column's first
//                         non-zero block row on (marg_plan.hpp: the tile columns lie in the order of that row)
//   the staged factorisation of [K | Ht] with r alongside, in the layout the gradient uses for [K | I]: k_marg_panel_update
//                         (k_grad_panel_update with the first rows of the plan instead of 128 j), k_potrf_diag, k_trsm_strip;
//                         block row p takes K's own columns and the appended slots 0 .. active[p] - 1
//   k_marg_rhs_partial / _finish   bt = W^T z in two fixed-order stages (256-row slabs, then the slabs in order)
//   k_marg_gram           one workgroup per (Gram tile, matrix): a 128 x 128 tile of W^T W in the MFMA accumulators, from the
//                         tile's first non-zero row to Npad; the identity -- padding diagonal included -- in the epilogue
//   the staged kernels on M (side 128 Q, one matrix of the batch per proposal) with bt as its right-hand side: y = U_M^-T bt,
//                         the gain y^T y and log det M come out of k_potrf_diag's records.  With the covariance asked for the
//                         layout is [M | I] and the kernels are the gradient's; M^-1 = W_M^T W_M by k_fisher_kinv
//   k_marg_finish         one workgroup per matrix: lnL and its four parts from the two sets of records; g = U_M^-1 y by a
//                         back substitution with the inverted diagonal blocks potrf leaves; E[beta] = Lambda^1/2 g; fl - Ht g
//   k_marg_cov            Cov[beta] from M^-1
// fp64 throughout, no atomics, every sum in an order fixed by (N, c, epoch layout, order): a matrix's bits do not depend on
// the batch around it nor on which optional outputs are asked for.
//
// Workspace per matrix: Npad x (Npad + 128 Q) doubles of [K | Ht] -- the gradient's buffer, never more than its [K | I] --
// plus 128 Q x 256 Q of M and a few vectors; per handle Npad x 128 Q of Ht.  Flops per matrix: N^3 / 3 for K, about
// 2 N^2 q' for the solve of the appended block and N q'^2 for the Gram (q' = 128 Q, less what lies above the first rows).
#pragma once
#include "calibrate_kernels.hpp"
#include "fisher_kernels.hpp"
#include "grad_kernels.hpp"
#include "marg_plan.hpp"

namespace psoap {

static_assert(MARG_MAX_ORDER == CAL_MAX_ORDER, "marg_plan.hpp restates the bound of cheb_row's callers");

// the int tables of a baseline on the device: [Q] first block row per slot, [Q] tile column per slot, [Q] slot per tile column
__host__ __device__ inline int marg_tab_first(int) { return 0; }
__host__ __device__ inline int marg_tab_column(int Q) { return Q; }
__host__ __device__ inline int marg_tab_slot(int Q) { return 2 * Q; }

// grid ceil(N / 256).  Ht is cleared before.
__global__ __launch_bounds__(256) void k_marg_basis(double* __restrict__ Ht, int ldh, int N, int order, int Q,
                                                    const double* __restrict__ x, const int* __restrict__ epoch,
                                                    const double* __restrict__ ep_off, const double* __restrict__ ep_scl,
                                                    const double* __restrict__ weight, const double* __restrict__ sd,
                                                    const int* __restrict__ tab)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int e = epoch[i];
    double T[CAL_MAX_ORDER + 1];
    cheb_row(x[i], ep_off[e], ep_scl[e], order, T);
    const double w = weight ? weight[i] : 1.0;
    const int* slot = tab + marg_tab_slot(Q);
    for (int k = 0; k <= order; ++k) {
        const int c = e * (order + 1) + k;
        Ht[(size_t)i * ldh + NB * slot[c / NB] + (c % NB)] = (w * T[k]) * sd[k];
    }
}

// grid (Q P, B): tile (block row tr, slot s) of Ht into matrix b, where tr >= first[s]
__global__ __launch_bounds__(256) void k_marg_load(double* __restrict__ Abase, size_t mat_stride, int ld, int Npad, int P,
                                                   const double* __restrict__ Ht, int ldh, const int* __restrict__ tab)
{
    const int s = blockIdx.x / P, tr = blockIdx.x % P;
    if (tr < tab[s]) return;
    double* W = Abase + (size_t)blockIdx.y * mat_stride + Npad + NB * s;
    const double* src = Ht + NB * s;
    const int col2 = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    for (int r = r0; r < NB; r += 4) {
        const size_t row = (size_t)NB * tr + r;
        *reinterpret_cast<d2*>(W + row * ld + 2 * col2) = *reinterpret_cast<const d2*>(src + row * ldh + 2 * col2);
    }
}

// k_panel_update for block row k0 of [K | Ht]: tile columns p .. (grid.x = P - p + active[p]); the K loop of the appended
// slot s starts at row 128 first[s], below the structural zeros (a slot with first[s] == p has nothing above it).
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_marg_panel_update(double* __restrict__ Abase, size_t mat_stride, int ld,
                                                                      int k0, int P, const int* __restrict__ tab)
{
    double* Km = Abase + (size_t)blockIdx.y * mat_stride;
    const int tcol = k0 / NB + blockIdx.x;
    const int ks = tcol >= P ? NB * tab[tcol - P] : 0;
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

// bt = W^T z in two fixed-order stages, as k_grad_alpha_partial does for alpha.  partial[b][sl][c] = sum over the rows k of
// slab sl (256 rows) of W[k][c] z[k], from the column's first non-zero row on; slabs wholly above it are neither written nor
// read.  c counts in the column order of H.  grid (Q slots, nslab, B)
__global__ __launch_bounds__(256) void k_marg_rhs_partial(const double* __restrict__ Abase, size_t mat_stride, int ld, int Npad,
                                                          int Q, const int* __restrict__ tab, const double* __restrict__ Z,
                                                          double* __restrict__ partial, int nslab)
{
    __shared__ double red[NB];
    const int b = blockIdx.z, s = blockIdx.x, sl = blockIdx.y;
    const int col = threadIdx.x & 127, half = threadIdx.x >> 7;
    const int kfirst = NB * tab[s];
    const int kend = min(256 * (sl + 1), Npad);
    if (kend <= kfirst) return;
    const int kbeg = max(256 * sl, kfirst);
    const double* W = Abase + (size_t)b * mat_stride + Npad + NB * s + col;
    const double* z = Z + (size_t)b * Npad;
    double acc = 0.0;
    for (int k = kbeg + half; k < kend; k += 2) acc = fma(W[(size_t)k * ld], z[k], acc);
    if (half == 1) red[col] = acc;
    __syncthreads();
    if (half == 0) partial[((size_t)b * nslab + sl) * (NB * Q) + NB * tab[marg_tab_column(Q) + s] + col] = acc + red[col];
}

// grid (ceil(128 Q / 256), B): the slabs in order into the right-hand side of M (0 for a tile column without a row)
__global__ void k_marg_rhs_finish(const double* __restrict__ partial, int nslab, int Npad, int Q, const int* __restrict__ tab,
                                  double* __restrict__ rhs)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (c >= NB * Q) return;
    const int kfirst = NB * tab[tab[marg_tab_slot(Q) + c / NB]];
    double s = 0.0;
    if (kfirst < Npad)
        for (int k = kfirst / 256; k < nslab; ++k) s += partial[((size_t)b * nslab + k) * (NB * Q) + c];
    rhs[(size_t)b * (NB * Q) + c] = s;
}

// One workgroup per (Gram tile, matrix): M[ti][tj] = [ti == tj] I + W_ti^T W_tj over the rows from the tile's first non-zero
// row on (everything above is exactly zero in one of the two).  A diagonal tile: its upper half (all the staged kernels read).
// grid (Q (Q + 1) / 2, B)
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_marg_gram(const double* __restrict__ Abase, size_t mat_stride, int ld,
                                                              int Npad, const MargTile* __restrict__ tiles,
                                                              double* __restrict__ Mbase, size_t m_stride, int ldm)
{
    const MargTile g = tiles[blockIdx.x];
    const double* W = Abase + (size_t)blockIdx.y * mat_stride + Npad + (size_t)g.k0 * ld;
    Tile t;
    t.zero();
    tile_gemm_tn(t, W + NB * g.si, (size_t)ld, W + NB * g.sj, (size_t)ld, Npad - g.k0, g.ti == g.tj);
    // (the thread id passes through an opaque statement, as in k_loo_band: no address of the epilogue is computed and kept in
    // registers ahead of the K-loop)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    double* Mt = Mbase + (size_t)blockIdx.y * m_stride + (size_t)NB * g.ti * ldm + NB * g.tj;
    const bool diag_tile = g.ti == g.tj;
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

// grid B, 256 threads.  accK: the records of K's factorisation (z^T z, log det K), accM: those of M's (the gain y^T y,
// log det M).  out[b][5] = lnL, z^T z, log det K, gain, log det M.  With want != 0 also g = U_M^-1 y, block row by block row
// from the last one up with the inverses Wt[p][i][k] = (U_pp^-1)[i][k] potrf left (as k_loo_finish solves its blocks):
//     t[i] = y[128 p + i] - sum_{k >= 128 (p + 1)} U[128 p + i][k] g[k]      a wave per row, lanes 64 apart, a butterfly
//     g[128 p + i] = sum_k Wt[p][i][k] t[k]                                  likewise
// then beta[c] = s_(c mod (order + 1)) g[c] and fl_cor[i] = fl[i] - sum_k Ht[i][col(e_i, k)] g[col(e_i, k)], k ascending.
__global__ __launch_bounds__(256) void k_marg_finish(int N, int P, int Q, int q, int order, const MatAcc* __restrict__ accK,
                                                     const MatAcc* __restrict__ accM, const double* __restrict__ Mbase,
                                                     size_t m_stride, int ldm, const double* __restrict__ WtM,
                                                     const double* __restrict__ Y, double* G, const double* __restrict__ sd,
                                                     const int* __restrict__ epoch, const int* __restrict__ tab,
                                                     const double* __restrict__ Ht, int ldh, const double* __restrict__ fl,
                                                     double* __restrict__ out, double* __restrict__ beta,
                                                     double* __restrict__ fl_cor, int want)
{
    __shared__ double tbuf[NB];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = NB * Q;
    if (tid == 0) {
        const MatAcc aK = acc_total(accK + (size_t)b * ACC_ROWS, P), aM = acc_total(accM + (size_t)b * ACC_ROWS, Q);
        const bool bad = aK.info != 0.0 || aM.info != 0.0;
        const double quad = aK.quad, ldK = 2.0 * aK.logdet_half, gain = aM.quad, ldM = 2.0 * aM.logdet_half;
        double* o = out + (size_t)b * 5;
        o[0] = bad ? -INFINITY : -0.5 * (((quad - gain) + ldK) + ldM);
        o[1] = bad ? NAN : quad;
        o[2] = bad ? NAN : ldK;
        o[3] = bad ? NAN : gain;
        o[4] = bad ? NAN : ldM;
    }
    if (!want) return;
    const double* Ub = Mbase + (size_t)b * m_stride;
    const double* y = Y + (size_t)b * S;
    double* g = G + (size_t)b * S;
    for (int p = Q - 1; p >= 0; --p) {
        const int r0 = NB * p;
        for (int i = wave; i < NB; i += 4) {
            const double* Ui = Ub + (size_t)(r0 + i) * ldm;
            double a = 0.0;
            for (int k = r0 + NB + lane; k < S; k += 64) a = fma(Ui[k], g[k], a);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
            if (lane == 0) tbuf[i] = y[r0 + i] - a;
        }
        __syncthreads();
        const double* Wp = WtM + ((size_t)b * Q + p) * NB * NB;
        for (int i = wave; i < NB; i += 4) {
            const double* Wi = Wp + (size_t)i * NB;
            double a = fma(Wi[lane], tbuf[lane], Wi[64 + lane] * tbuf[64 + lane]);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
            if (lane == 0) g[r0 + i] = a;
        }
        __syncthreads();      // (g is read back from memory by the other waves: the barrier orders it within the workgroup)
    }
    for (int c = tid; c < q; c += 256) beta[(size_t)b * q + c] = sd[c % (order + 1)] * g[c];
    const int* slot = tab + marg_tab_slot(Q);
    for (int i = tid; i < N; i += 256) {
        const int c0 = epoch[i] * (order + 1);
        double a = 0.0;
        for (int k = 0; k <= order; ++k) {
            const int c = c0 + k;
            a = fma(Ht[(size_t)i * ldh + NB * slot[c / NB] + (c % NB)], g[c], a);
        }
        fl_cor[(size_t)b * N + i] = fl[i] - a;
    }
}

// Cov[beta][i][j] = s_i M^-1[i][j] s_j.  grid (q, B)
__global__ __launch_bounds__(256) void k_marg_cov(const double* __restrict__ Minv, int S, int q, int order,
                                                  const double* __restrict__ sd, double* __restrict__ cov)
{
    const int i = blockIdx.x, b = blockIdx.y;
    const double si = sd[i % (order + 1)];
    for (int j = threadIdx.x; j < q; j += 256)
        cov[((size_t)b * q + i) * q + j] = si * Minv[((size_t)b * S + i) * S + j] * sd[j % (order + 1)];
}

inline hipError_t marg_configure_kernels()
{
    const int lds = (int)GEMM_LDS_BYTES;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_panel_update),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_gram), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    return e;
}

// matrices per group of a call: the gradient's bound (GRAD_WS_BYTES, GRAD_GROUP_MAX) on the narrower [K | Ht]
inline int marg_group_size(int B, int Npad, int Q)
{
    const size_t per = sizeof(double) * (size_t)Npad * ((size_t)Npad + (size_t)NB * Q);
    size_t g = GRAD_WS_BYTES / per;
    if (g < 1) g = 1;
    if (g > (size_t)GRAD_GROUP_MAX) g = GRAD_GROUP_MAX;
    return B < (int)g ? B : (int)g;
}

// What psoap_chunk_set_baseline keeps on the host: psoap_chunk_marg_release frees every device buffer, and the next
// psoap_chunk_lnlike_marg builds Ht again from this.
struct MargSetup {
    bool valid = false;
    bool stale_weight = false;      // psoap_chunk_set_data since a baseline with weights: they described the old data
    MargPlan plan;
    std::vector<double> x, weight, sd;      // (weight empty: 1)
    std::vector<int32_t> epoch;
};

// the device side of a baseline and the workspace of the marginal likelihood beyond the gradient's (grow-only;
// psoap_chunk_marg_release frees it)
struct MargWs {
    bool basis_ready = false;
    Grow<double> Ht, X, Weight, EpOff, EpScl, Sd;
    Grow<int> Epoch, Tab;
    Grow<MargTile> Tiles;
    Grow<double> M, WtM, Rhs, Gam, RPart, Minv, Cov, Beta, Flc, Out;
    Grow<MatAcc> AccM;
};

}  // namespace psoap
