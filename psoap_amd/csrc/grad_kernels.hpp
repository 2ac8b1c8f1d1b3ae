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
//
// Under the time-variable kernel of fill_kernels.hpp (`TV`), e_cij = exp(p_c d_cij^2 + q_c dt_ij^2): the gradient keeps its
// formulas and gains
//   dlnL/dtau_c = 1/2 a_c^2 / tau_c^3 sum_ij Q_ij e_cij dt_ij^2            (exactly 0 at tau_c = inf)
// The factorisation, alpha and the product W_ti^T W_tj are the same; the epilogue of the contraction forms the argument as the
// fill does (so at tau = inf the value and the static gradient have the static bits) and carries one more sum per
// component, and the finishing sums add it up.
#pragma once
#include "chol_kernels.hpp"
#include "fill_kernels.hpp"

namespace psoap {

// One tile of the contraction, static or time-variable: its record in the partial-sum workspace -- row sums [3][128], column
// sums [3][128], then HYP sums per component (sa, sl and under TV st; the static record has two spare doubles) -- and the map
// of the epilogue's LDS.  Both are also those of the contractions of fisher_kernels.hpp.
template <bool TV>
struct GradTile {
    static constexpr int HYP = TV ? 3 : 2;
    static constexpr int ROWS_OFF = 0, COLS_OFF = 3 * NB, HYP_OFF = 6 * NB, DOUBLES = 6 * NB + (TV ? 9 : 8);
    static constexpr int XS = 0;                            // [2][3][NB]: abscissae of the tile's rows (side 0) and columns (side 1)
    static constexpr int AL = XS + 6 * NB;                  // [2][NB]: alpha likewise (ContractQ::Gradient only)
    static constexpr int TS = AL + 2 * NB;                  // [2][NB]: times likewise (TV only)
    static constexpr int RS = TS + (TV ? 2 * NB : 0);       // [2 wc][3][NB]: row sums of the two wave columns
    static constexpr int CS = RS + 6 * NB;                  // [2 wr][3][NB]: column sums of the two wave rows
    static constexpr int HS = CS + 6 * NB;                  // [4 waves][WS]
    static constexpr int WS = 3 * HYP;
    static_assert((HS + 4 * WS) * sizeof(double) <= GEMM_LDS_BYTES, "the epilogue fits the operand buffers");
};

// How a lane of the epilogue forms q from its element t of the accumulator tile:
//   Gradient  q = alpha_i alpha_j - t   t = (K^-1)_ij: the gradient's Q
//   Fisher    q = 1/2 t                 t = (2 G_t)_ij: the symmetrised product of fisher_kernels.hpp; no alpha is read
enum class ContractQ { Gradient, Fisher };

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
// in a fixed order, and the workgroup stores them to its own GradTile<TV>::DOUBLES of `part`.
// The epilogue: everything after the product, on the tile t = (K^-1)[ti][tj] in the accumulators (one function: the two
// kernels below, k_marg_grad_contract of marg_grad_kernels.hpp, whose t is the tile of (K + Ht Ht^T)^-1, and with
// Q = ContractQ::Fisher the two contractions of fisher_kernels.hpp, whose t is the tile of 2 G_t and whose alpha is nullptr).
// TV: e_c = exp(p_c d^2 + q_c dt^2) from `times` (N) and tau (B, C), the tile's row and column times beside its abscissae in
// LDS, and one more sum per component, st = sum w q e_c dt^2; sa, sl and the row and column sums keep their formulas and
// their order.
// Fisher: behind two K-loops the kernel has fewer registers, so the thread id passes through an opaque statement in every turn
// of the component loop: the rows, columns, masks and weights derived from it are formed again per component and not kept
// across the loop -- 64 predicates and weights held live beside the accumulators spill (profiles/timevar_fisher.md).
template <int C, bool TV = false, ContractQ Q = ContractQ::Gradient>
__device__ __forceinline__ void grad_contract_epilogue(const Tile& t, int b, int ti, int tj, int tile_index, int N, int Npad,
                                                       int P, const double* __restrict__ lwl, const double* __restrict__ gp,
                                                       const double* __restrict__ alpha, double* __restrict__ part,
                                                       const double* __restrict__ times = nullptr,
                                                       const double* __restrict__ tau = nullptr)
{
    using L = GradTile<TV>;
    constexpr int XS = L::XS, AL = L::AL, RS = L::RS, CS = L::CS, HS = L::HS, WS = L::WS;
    constexpr bool FISHER = Q == ContractQ::Fisher;
    const int tid = threadIdx.x;
    int lane = tid & 63, wave = tid >> 6;
    int wr = wave >> 1, wc = wave & 1;
    const double* lw = lwl + (size_t)b * C * N;
    {
        const int side = tid >> 7, idx = tid & 127;
        const int g = NB * (side ? tj : ti) + idx;
#pragma unroll
        for (int c = 0; c < C; ++c) psoap_smem[XS + (side * 3 + c) * NB + idx] = (g < N) ? lw[(size_t)c * N + g] : 0.0;
        if constexpr (!FISHER) psoap_smem[AL + side * NB + idx] = alpha[(size_t)b * Npad + g];
        if constexpr (TV) psoap_smem[L::TS + side * NB + idx] = (g < N) ? times[g] : 0.0;
    }
    __syncthreads();
    const bool diag_tile = ti == tj;
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        if constexpr (FISHER) {      // (the gradient keeps what it formed ahead of the loop, and its instructions)
            int tl = tid;
            asm volatile("" : "+v"(tl));
            lane = tl & 63;
            wave = tl >> 6;
            wr = wave >> 1;
            wc = wave & 1;
        }
        double p2;
        {
#pragma clang fp contract(off)
            const double l = gp[(size_t)b * 2 * C + 2 * c + 1];      // (as load_gp rounds it)
            p2 = -0.5 * (C_KMS * C_KMS) / (l * l);
        }
        [[maybe_unused]] double q2;
        if constexpr (TV) q2 = tv_q2(tau[(size_t)b * C + c]);
        double xj[4], colacc[4];
        [[maybe_unused]] double aj[4];
        bool jok[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int col = tile_col(wc, n, lane);
            xj[n] = psoap_smem[XS + (3 + c) * NB + col];
            if constexpr (!FISHER) aj[n] = psoap_smem[AL + NB + col];
            jok[n] = NB * tj + col < N;
            colacc[n] = 0.0;
        }
        double sa = 0.0, sl = 0.0;
        [[maybe_unused]] double st = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            double xi[4], rowacc[4];
            [[maybe_unused]] double ai[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = tile_row(wr, m, lane, r);
                xi[r] = psoap_smem[XS + c * NB + row];
                if constexpr (!FISHER) ai[r] = psoap_smem[AL + row];
                rowacc[r] = 0.0;
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int col = tile_col(wc, n, lane);
                // (the times are read where they are used: two more values per row and column kept across the tile would
                // not fit beside the accumulators)
                [[maybe_unused]] double tcol;
                if constexpr (TV) tcol = psoap_smem[L::TS + NB + col];
                double d[4], a[4], e[4];
                bool live = false;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma clang fp contract(off)
                    d[r] = xj[n] - xi[r];
                    [[maybe_unused]] double dt;
                    if constexpr (TV) dt = tcol - psoap_smem[L::TS + tile_row(wr, m, lane, r)];
                    a[r] = p2 * d[r] * d[r];
                    if constexpr (TV) a[r] = a[r] + q2 * dt * dt;
                    live = live || !(a[r] <= -746.0);
                }
                if (__builtin_amdgcn_ballot_w64(live) == 0ull) continue;      // exp() = +0 for the whole wave: nothing to add
                exp_nonpos_batch<4>(a, e);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = tile_row(wr, m, lane, r);
                    const bool ok = jok[n] && NB * ti + row < N && (!diag_tile || row <= col);
                    double qe;
                    if constexpr (FISHER) qe = ok ? 0.5 * t.acc[m][n][r] * e[r] : 0.0;
                    else qe = ok ? (ai[r] * aj[n] - t.acc[m][n][r]) * e[r] : 0.0;
                    const double w = (diag_tile && row == col) ? 1.0 : 2.0;
                    const double qed = qe * d[r];
                    [[maybe_unused]] double dt;
                    if constexpr (TV) {
                        // dt again from LDS, through an index the optimiser cannot match with the one above: four time
                        // differences kept across the exp are registers the kernel does not have
                        int trow = L::TS + row;
                        asm volatile("" : "+v"(trow));
                        dt = tcol - psoap_smem[trow];
                    }
                    sa = fma(w, qe, sa);
                    sl = fma(w * qed, d[r], sl);
                    if constexpr (TV) st = fma(w * qe * dt, dt, st);
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
            if constexpr (TV) st += __shfl_xor(st, off, 64);
        }
        if (lane == 0) {
            psoap_smem[HS + wave * WS + L::HYP * c] = sa;
            psoap_smem[HS + wave * WS + L::HYP * c + 1] = sl;
            if constexpr (TV) psoap_smem[HS + wave * WS + L::HYP * c + 2] = st;
        }
    }
    __syncthreads();
    double* out = part + ((size_t)b * (P * (P + 1) / 2) + tile_index) * L::DOUBLES;
    {
        const int side = tid >> 7, idx = tid & 127;
        const int src = side ? CS : RS;
#pragma unroll
        for (int c = 0; c < C; ++c)
            out[(side ? L::COLS_OFF : L::ROWS_OFF) + c * NB + idx] =
                psoap_smem[src + c * NB + idx] + psoap_smem[src + (3 + c) * NB + idx];
    }
    if (tid < L::HYP * C)
        out[L::HYP_OFF + tid] = ((psoap_smem[HS + tid] + psoap_smem[HS + WS + tid]) + psoap_smem[HS + 2 * WS + tid]) +
                                psoap_smem[HS + 3 * WS + tid];
}

// The product and the epilogue: what k_grad_contract and k_tv_grad_contract are.  grid (P (P + 1) / 2, B)
template <int C, bool TV>
__device__ __forceinline__ void grad_contract_tile(const double* __restrict__ Abase, size_t mat_stride, int ld, int N, int Npad,
                                                   int P, const double* __restrict__ lwl, const double* __restrict__ gp,
                                                   const double* __restrict__ alpha, double* __restrict__ part,
                                                   const double* __restrict__ times, const double* __restrict__ tau)
{
    const int b = blockIdx.y;
    int ti, tj;
    decode_upper(blockIdx.x, P, ti, tj);
    const double* W = Abase + (size_t)b * mat_stride + Npad + (size_t)NB * tj * ld;
    Tile t;
    t.zero();
    tile_gemm_tn(t, W + NB * ti, (size_t)ld, W + NB * tj, (size_t)ld, Npad - NB * tj, ti == tj);
    grad_contract_epilogue<C, TV>(t, b, ti, tj, (int)blockIdx.x, N, Npad, P, lwl, gp, alpha, part, times, tau);
}

template <int C>
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_grad_contract(const double* __restrict__ Abase, size_t mat_stride,
                                                                  int ld, int N, int Npad, int P,
                                                                  const double* __restrict__ lwl,
                                                                  const double* __restrict__ gp,
                                                                  const double* __restrict__ alpha,
                                                                  double* __restrict__ part)
{
    grad_contract_tile<C, false>(Abase, mat_stride, ld, N, Npad, P, lwl, gp, alpha, part, nullptr, nullptr);
}

template <int C>
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_tv_grad_contract(const double* __restrict__ Abase, size_t mat_stride,
                                                                     int ld, int N, int Npad, int P,
                                                                     const double* __restrict__ lwl,
                                                                     const double* __restrict__ times,
                                                                     const double* __restrict__ gp,
                                                                     const double* __restrict__ tau,
                                                                     const double* __restrict__ alpha,
                                                                     double* __restrict__ part)
{
    grad_contract_tile<C, true>(Abase, mat_stride, ld, N, Npad, P, lwl, gp, alpha, part, times, tau);
}

// The tiles' partial sums in tile order.  grid (P + 1, B), 128 threads.
//   blocks x < P:  grad_x[b][c][128 x + i]: the column sums of tiles (ti, x), ti <= x, then the row sums of tiles (x, tj), tj >= x
//   block  x == P: the HYP C hyper-parameter sums and sum_i alpha_i: thread k adds every 128th term, the 128 sums meet in a tree
//                  grad_gp[b][2C], under TV grad_tau[b][c] = 1/2 a_c^2 / tau_c^3 st_c, grad_mu[b]
template <bool TV>
__device__ __forceinline__ void grad_finish_sums(const double* __restrict__ part, const double* __restrict__ alpha,
                                                 const double* __restrict__ gp, int C, int N, int Npad, int P,
                                                 double* __restrict__ grad_gp, double* __restrict__ grad_x,
                                                 double* __restrict__ grad_mu, const double* __restrict__ tau,
                                                 double* __restrict__ grad_tau)
{
    using L = GradTile<TV>;
    __shared__ double red[128];
    const int b = blockIdx.y, x = blockIdx.x, tid = threadIdx.x;
    const int ntiles = P * (P + 1) / 2;
    const double* pb = part + (size_t)b * ntiles * L::DOUBLES;
    const double* gpb = gp + (size_t)b * 2 * C;
    if (x < P) {
        const int i = NB * x + tid;
        for (int c = 0; c < C; ++c) {
            double s = 0.0;
            for (int ti = 0; ti <= x; ++ti) s += pb[(size_t)upper_index(ti, x, P) * L::DOUBLES + L::COLS_OFF + c * NB + tid];
            for (int tj = x; tj < P; ++tj) s += pb[(size_t)upper_index(x, tj, P) * L::DOUBLES + L::ROWS_OFF + c * NB + tid];
            const double a = gpb[2 * c], l = gpb[2 * c + 1];
            const double p2 = -0.5 * (C_KMS * C_KMS) / (l * l);
            if (i < N) grad_x[((size_t)b * C + c) * N + i] = -2.0 * p2 * (a * a) * s;
        }
        return;
    }
    for (int k = 0; k <= L::HYP * C; ++k) {
        double s = 0.0;
        if (k < L::HYP * C) {
            for (int t = tid; t < ntiles; t += 128) s += pb[(size_t)t * L::DOUBLES + L::HYP_OFF + k];
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
            if (k == L::HYP * C) {
                grad_mu[b] = red[0];
            } else {
                const int c = k / L::HYP, what = k % L::HYP;
                const double a = gpb[2 * c], l = gpb[2 * c + 1];
                if (what == 0) {
                    grad_gp[(size_t)b * 2 * C + 2 * c] = a * red[0];
                } else if (what == 1) {
                    grad_gp[(size_t)b * 2 * C + 2 * c + 1] = 0.5 * (a * a) * (C_KMS * C_KMS) / (l * l * l) * red[0];
                } else if constexpr (TV) {
                    const double tc = tau[(size_t)b * C + c];
                    grad_tau[(size_t)b * C + c] = 0.5 * (a * a) / (tc * tc * tc) * red[0];
                }
            }
        }
    }
}

__global__ __launch_bounds__(128) void k_grad_finish(const double* __restrict__ part, const double* __restrict__ alpha,
                                                     const double* __restrict__ gp, int C, int N, int Npad, int P,
                                                     double* __restrict__ grad_gp, double* __restrict__ grad_x,
                                                     double* __restrict__ grad_mu)
{
    grad_finish_sums<false>(part, alpha, gp, C, N, Npad, P, grad_gp, grad_x, grad_mu, nullptr, nullptr);
}

__global__ __launch_bounds__(128) void k_tv_grad_finish(const double* __restrict__ part, const double* __restrict__ alpha,
                                                        const double* __restrict__ gp, const double* __restrict__ tau, int C,
                                                        int N, int Npad, int P, double* __restrict__ grad_gp,
                                                        double* __restrict__ grad_tau, double* __restrict__ grad_x,
                                                        double* __restrict__ grad_mu)
{
    grad_finish_sums<true>(part, alpha, gp, C, N, Npad, P, grad_gp, grad_x, grad_mu, tau, grad_tau);
}

// ---- the quasi-periodic kernel of fill_kernels.hpp (`QP`) ---------------------------------------------------------------------
//   e_cij = exp(p_c d_cij^2 + q_c dt_ij^2 - Gamma_c sin^2(pi dt_ij / P_c))
// The gradient keeps the time-variable formulas with this e and gains
//   dlnL/dGamma_c = -1/2 a_c^2 sum_ij Q_ij e_cij sin^2(pi dt_ij / P_c)
//   dlnL/dP_c     =  1/2 a_c^2 Gamma_c pi / P_c^2 sum_ij Q_ij e_cij dt_ij sin(2 pi dt_ij / P_c)      (exactly 0 at Gamma_c = 0)
// The tile record and the epilogue's LDS map are decided here: GradTile<true> with five sums per component -- sa, sl, st and
//   sg = sum w q e s^2,   sp = sum w q e dt (2 s co)        (s, co = sincospi(dt * rP), the pair the argument is built from)
// -- so a record is two doubles per component longer than the time-variable one.
struct QpTile {
    static constexpr int HYP = 5;
    static constexpr int ROWS_OFF = 0, COLS_OFF = 3 * NB, HYP_OFF = 6 * NB, DOUBLES = 6 * NB + 3 * HYP;
    static constexpr int XS = 0;                 // [2][3][NB]: abscissae of the tile's rows (side 0) and columns (side 1)
    static constexpr int AL = XS + 6 * NB;       // [2][NB]: alpha likewise
    static constexpr int TS = AL + 2 * NB;       // [2][NB]: times likewise
    static constexpr int RS = TS + 2 * NB;       // [2 wc][3][NB]: row sums of the two wave columns
    static constexpr int CS = RS + 6 * NB;       // [2 wr][3][NB]: column sums of the two wave rows
    static constexpr int HS = CS + 6 * NB;       // [4 waves][WS]
    static constexpr int WS = 3 * HYP;
    static_assert((HS + 4 * WS) * sizeof(double) <= GEMM_LDS_BYTES, "the epilogue fits the operand buffers");
};

// grad_contract_epilogue<C, true> (the gradient's q) with the periodic term in the argument and the two sums more.  A function
// of its own beside it: the shared one keeps its instructions.  sa, sl, st and the row and column sums are formed by the same
// operations in the same order, so at Gamma = 0 -- where the argument has the time-variable bits -- they have the
// time-variable bits.  The underflow shortcut is taken on the two-term argument first (the periodic term is <= 0), ahead of
// the sincospi, and then on the full one.
// Registers.  Beside the accumulators the kernel has none to spare, and whatever the epilogue holds too long the allocator
// takes out of the K loop's operand registers, as scratch traffic in every turn.  So nothing is kept that can be formed
// again: s and co are evaluated a second time behind the exp, by the same sincospi on the same rounded u = dt * rP (the bits
// that rebuilt the argument), where keeping s^2 and 2 s co of four elements across the exp cost 16 registers; d is the same
// subtraction again; and the column's abscissa, alpha and time come from LDS where they are used, not once per tile.  With
// that no instance has a scratch instruction in or ahead of its K loop (profiles/quasiperiodic.md has the forms that had).
// Q = ContractQ::Fisher (k_qp_fisher_contract of fisher_kernels.hpp): t is the tile of 2 G_t, q = 1/2 t, alpha is nullptr and no
// alpha row is staged or read; behind two K loops the thread id passes through an opaque statement in every turn of the
// component loop, as in grad_contract_epilogue and for its reason.  The gradient's instance keeps its instructions.
template <int C, ContractQ Q = ContractQ::Gradient>
__device__ __forceinline__ void qp_contract_epilogue(const Tile& t, int b, int ti, int tj, int tile_index, int N, int Npad,
                                                     int P, const double* __restrict__ lwl, const double* __restrict__ gp,
                                                     const double* __restrict__ alpha, double* __restrict__ part,
                                                     const double* __restrict__ times, const double* __restrict__ tau,
                                                     const double* __restrict__ gam, const double* __restrict__ per)
{
    using L = QpTile;
    constexpr int XS = L::XS, AL = L::AL, TS = L::TS, RS = L::RS, CS = L::CS, HS = L::HS, WS = L::WS;
    constexpr bool FISHER = Q == ContractQ::Fisher;
    const int tid = threadIdx.x;
    int lane = tid & 63, wave = tid >> 6;
    int wr = wave >> 1, wc = wave & 1;
    const double* lw = lwl + (size_t)b * C * N;
    {
        const int side = tid >> 7, idx = tid & 127;
        const int g = NB * (side ? tj : ti) + idx;
#pragma unroll
        for (int c = 0; c < C; ++c) psoap_smem[XS + (side * 3 + c) * NB + idx] = (g < N) ? lw[(size_t)c * N + g] : 0.0;
        if constexpr (!FISHER) psoap_smem[AL + side * NB + idx] = alpha[(size_t)b * Npad + g];
        psoap_smem[TS + side * NB + idx] = (g < N) ? times[g] : 0.0;
    }
    __syncthreads();
    const bool diag_tile = ti == tj;
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        if constexpr (FISHER) {
            int tl = tid;
            asm volatile("" : "+v"(tl));
            lane = tl & 63;
            wave = tl >> 6;
            wr = wave >> 1;
            wc = wave & 1;
        }
        double p2;
        {
#pragma clang fp contract(off)
            const double l = gp[(size_t)b * 2 * C + 2 * c + 1];      // (as load_gp rounds it)
            p2 = -0.5 * (C_KMS * C_KMS) / (l * l);
        }
        const double q2 = tv_q2(tau[(size_t)b * C + c]);
        const double rP = qp_rp(per[(size_t)b * C + c]);
        const double ng = qp_ng(gam[(size_t)b * C + c]);
        double colacc[4];
        bool jok[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            jok[n] = NB * tj + tile_col(wc, n, lane) < N;
            colacc[n] = 0.0;
        }
        double sa = 0.0, sl = 0.0, st = 0.0, sg = 0.0, sp = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            double xi[4], rowacc[4];
            [[maybe_unused]] double ai[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = tile_row(wr, m, lane, r);
                xi[r] = psoap_smem[XS + c * NB + row];
                if constexpr (!FISHER) ai[r] = psoap_smem[AL + row];
                rowacc[r] = 0.0;
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int col = tile_col(wc, n, lane);
                // (the column's abscissa, alpha and time are read where they are used, through an index the optimiser cannot
                // follow: kept across the tile they are 24 registers the kernel does not have beside the sincospi)
                int cidx = col;
                asm volatile("" : "+v"(cidx));
                const double xjn = psoap_smem[XS + (3 + c) * NB + cidx];
                [[maybe_unused]] double ajn;
                if constexpr (!FISHER) ajn = psoap_smem[AL + NB + cidx];
                const double tcol = psoap_smem[TS + NB + cidx];
                double a[4], e[4];
                bool live = false;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma clang fp contract(off)
                    const double d = xjn - xi[r];
                    const double dt = tcol - psoap_smem[TS + tile_row(wr, m, lane, r)];
                    a[r] = p2 * d * d;
                    a[r] = a[r] + q2 * dt * dt;
                    live = live || !(a[r] <= -746.0);
                }
                if (__builtin_amdgcn_ballot_w64(live) == 0ull) continue;      // exp() = +0 for the whole wave: nothing to add
                live = false;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma clang fp contract(off)
                    const double dt = tcol - psoap_smem[TS + tile_row(wr, m, lane, r)];
                    const double u = dt * rP;
                    double s, co;
                    sincospi(u, &s, &co);
                    a[r] = a[r] + ng * s * s;
                    live = live || !(a[r] <= -746.0);
                }
                if (__builtin_amdgcn_ballot_w64(live) == 0ull) continue;
                exp_nonpos_batch<4>(a, e);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = tile_row(wr, m, lane, r);
                    const bool ok = jok[n] && NB * ti + row < N && (!diag_tile || row <= col);
                    double qe;
                    if constexpr (FISHER) qe = ok ? 0.5 * t.acc[m][n][r] * e[r] : 0.0;
                    else qe = ok ? (ai[r] * ajn - t.acc[m][n][r]) * e[r] : 0.0;
                    const double w = (diag_tile && row == col) ? 1.0 : 2.0;
                    const double d = xjn - xi[r];
                    const double qed = qe * d;
                    // (dt again from LDS through an opaque index, as the time-variable epilogue does and for its reason)
                    int trow = TS + row;
                    asm volatile("" : "+v"(trow));
                    const double dt = tcol - psoap_smem[trow];
                    double s, co;
                    {
#pragma clang fp contract(off)
                        sincospi(dt * rP, &s, &co);
                    }
                    sa = fma(w, qe, sa);
                    sl = fma(w * qed, d, sl);
                    st = fma(w * qe * dt, dt, st);
                    sg = fma(w * qe, s * s, sg);
                    sp = fma(w * qe * dt, 2.0 * s * co, sp);
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
            st += __shfl_xor(st, off, 64);
            sg += __shfl_xor(sg, off, 64);
            sp += __shfl_xor(sp, off, 64);
        }
        if (lane == 0) {
            double* hs = psoap_smem + HS + wave * WS + L::HYP * c;
            hs[0] = sa;
            hs[1] = sl;
            hs[2] = st;
            hs[3] = sg;
            hs[4] = sp;
        }
    }
    __syncthreads();
    double* out = part + ((size_t)b * (P * (P + 1) / 2) + tile_index) * L::DOUBLES;
    {
        const int side = tid >> 7, idx = tid & 127;
        const int src = side ? CS : RS;
#pragma unroll
        for (int c = 0; c < C; ++c)
            out[(side ? L::COLS_OFF : L::ROWS_OFF) + c * NB + idx] =
                psoap_smem[src + c * NB + idx] + psoap_smem[src + (3 + c) * NB + idx];
    }
    if (tid < L::HYP * C)
        out[L::HYP_OFF + tid] = ((psoap_smem[HS + tid] + psoap_smem[HS + WS + tid]) + psoap_smem[HS + 2 * WS + tid]) +
                                psoap_smem[HS + 3 * WS + tid];
}

// The K loop of k_tv_grad_contract<C> and the epilogue above.  grid (P (P + 1) / 2, B)
template <int C>
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_qp_grad_contract(const double* __restrict__ Abase, size_t mat_stride,
                                                                     int ld, int N, int Npad, int P,
                                                                     const double* __restrict__ lwl,
                                                                     const double* __restrict__ times,
                                                                     const double* __restrict__ gp,
                                                                     const double* __restrict__ tau,
                                                                     const double* __restrict__ gam,
                                                                     const double* __restrict__ per,
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
    qp_contract_epilogue<C>(t, b, ti, tj, (int)blockIdx.x, N, Npad, P, lwl, gp, alpha, part, times, tau, gam, per);
}

// grad_finish_sums over QpTile records: the wavelength gradient, grad_gp, grad_tau and grad_mu by the operations and in the
// order of k_tv_grad_finish (thread k adds every 128th tile, the 128 sums meet in a tree), and
//   grad_gamma[b][c] = -1/2 a_c^2 sg_c,   grad_period[b][c] = 1/2 a_c^2 Gamma_c pi / P_c^2 sp_c  (+ 0.0: no -0 at Gamma = 0)
// grid (P + 1, B), 128 threads
__global__ __launch_bounds__(128) void k_qp_grad_finish(const double* __restrict__ part, const double* __restrict__ alpha,
                                                        const double* __restrict__ gp, const double* __restrict__ tau,
                                                        const double* __restrict__ gam, const double* __restrict__ per, int C,
                                                        int N, int Npad, int P, double* __restrict__ grad_gp,
                                                        double* __restrict__ grad_tau, double* __restrict__ grad_gamma,
                                                        double* __restrict__ grad_period, double* __restrict__ grad_x,
                                                        double* __restrict__ grad_mu)
{
    using L = QpTile;
    __shared__ double red[128];
    const int b = blockIdx.y, x = blockIdx.x, tid = threadIdx.x;
    const int ntiles = P * (P + 1) / 2;
    const double* pb = part + (size_t)b * ntiles * L::DOUBLES;
    const double* gpb = gp + (size_t)b * 2 * C;
    if (x < P) {
        const int i = NB * x + tid;
        for (int c = 0; c < C; ++c) {
            double s = 0.0;
            for (int ti = 0; ti <= x; ++ti) s += pb[(size_t)upper_index(ti, x, P) * L::DOUBLES + L::COLS_OFF + c * NB + tid];
            for (int tj = x; tj < P; ++tj) s += pb[(size_t)upper_index(x, tj, P) * L::DOUBLES + L::ROWS_OFF + c * NB + tid];
            const double a = gpb[2 * c], l = gpb[2 * c + 1];
            const double p2 = -0.5 * (C_KMS * C_KMS) / (l * l);
            if (i < N) grad_x[((size_t)b * C + c) * N + i] = -2.0 * p2 * (a * a) * s;
        }
        return;
    }
    for (int k = 0; k <= L::HYP * C; ++k) {
        double s = 0.0;
        if (k < L::HYP * C) {
            for (int t = tid; t < ntiles; t += 128) s += pb[(size_t)t * L::DOUBLES + L::HYP_OFF + k];
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
            if (k == L::HYP * C) {
                grad_mu[b] = red[0];
            } else {
                const int c = k / L::HYP, what = k % L::HYP;
                const double a = gpb[2 * c], l = gpb[2 * c + 1];
                if (what == 0) {
                    grad_gp[(size_t)b * 2 * C + 2 * c] = a * red[0];
                } else if (what == 1) {
                    grad_gp[(size_t)b * 2 * C + 2 * c + 1] = 0.5 * (a * a) * (C_KMS * C_KMS) / (l * l * l) * red[0];
                } else if (what == 2) {
                    const double tc = tau[(size_t)b * C + c];
                    grad_tau[(size_t)b * C + c] = 0.5 * (a * a) / (tc * tc * tc) * red[0];
                } else if (what == 3) {
                    grad_gamma[(size_t)b * C + c] = -0.5 * (a * a) * red[0];
                } else {
                    const double G = gam[(size_t)b * C + c], Pc = per[(size_t)b * C + c];
                    grad_period[(size_t)b * C + c] = 0.5 * (a * a) * G * 3.14159265358979323846 / (Pc * Pc) * red[0] + 0.0;
                }
            }
        }
    }
}

// the LDS attribute of every kernel here that takes the operand buffers
inline hipError_t grad_configure_kernels()
{
    const void* const kernels[] = {
        reinterpret_cast<const void*>(k_grad_panel_update),
        reinterpret_cast<const void*>(k_grad_contract<1>),    reinterpret_cast<const void*>(k_grad_contract<2>),
        reinterpret_cast<const void*>(k_grad_contract<3>),    reinterpret_cast<const void*>(k_tv_grad_contract<1>),
        reinterpret_cast<const void*>(k_tv_grad_contract<2>), reinterpret_cast<const void*>(k_tv_grad_contract<3>),
        reinterpret_cast<const void*>(k_qp_grad_contract<1>), reinterpret_cast<const void*>(k_qp_grad_contract<2>),
        reinterpret_cast<const void*>(k_qp_grad_contract<3>)};
    for (const void* k : kernels)
        if (hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEMM_LDS_BYTES)) return e;
    return hipSuccess;
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
    // psoap_chunk_lnlike_tv_grad (the TV kernels above): the group's time scales and dlnL/dtau
    Grow<double> Tau, GradTau;
    // psoap_chunk_lnlike_qp_grad (the QP kernels above): the group's Gamma and P, dlnL/dGamma and dlnL/dP
    Grow<double> Gamma, Period, GradGamma, GradPeriod;
};

}  // namespace psoap
