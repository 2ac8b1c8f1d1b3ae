// vel_newton_kernels.hpp -- the OBSERVED information of the per-epoch radial velocities (not in the reference): with
// G = K^-1 (under a baseline (K + H Lambda H^T)^-1), alpha = G r (alpha_m there) and C = G - alpha alpha^T,
//   J[s, t] = -d2 lnL / ds dt = -F[s, t] + u_s^T G u_t + 1/2 sum_mn K_st[m, n] C[m, n],   u_s = K_s alpha,
// for s = (k, e), t = (j, f): the curvature of the likelihood at the data, where F (vel_fisher_kernels.hpp) is its
// expectation.  Notation and signs are those of vel_fisher_kernels.hpp: d = x_k[n] - x_k[m], Dv_k antisymmetric and
// cross-epoch only, K_(k,e)[m, n] = Dv_k[m, n] ([m in e] - [n in e]).  Further, symmetric and cross-epoch only,
//   W_k[m, n] = a_k^2 (2 p_k + 4 p_k^2 d^2) exp(p_k d^2) / c_kms^2 * [epoch(m) != epoch(n)]
// (the within-epoch block would cancel in T below; it is an exact zero here, as in Dv_k), and the epoch-block sums
//   A_k[e, f] = sum over m in e, n in f of Dv_k[m, n] C[m, n]          g[(k, e)] = dlnL/dv[k, e] = -sum_f A_k[e, f]
//   B_k[e, f] = sum over m in e, n in f of W_k[m, n] C[m, n]           T_k = diag(rowsum(B_k)) - B_k
//   Y_k[m, f] = sum over n in f of Dv_k[m, n] alpha[n]                 u_(k,e)[m] = [m in e] sum_f Y_k[m, f] - Y_k[m, e]
// T_k is the last term of J in the diagonal block of component k (K_st = 0 for k != j).
//
//   k_vel_pair           one workgroup of 128 threads per 128 x 128 tile and component (grid (P P, c)), a thread per row:
//                        the tile's columns sorted by (slot, column) in LDS, then column after column d, the one exp(),
//                        Dv_k and W_k in registers, C from the K^-1 tile (read through its mirror image: lanes along a
//                        row of K^-1) and the two alpha slices; at the end of every column slot the thread's Y_k goes to
//                        its own entry of the partial buffer (slot-major: (c, S, Npad)) and the row sums of Dv C and W C
//                        are binned by row slot -- one thread per row slot adds the rows of LDS in ascending order -- into
//                        the tile's own entries of the S x S bin sums (the slots of vel_fisher_plan.hpp).
//                        c N^2 exponentials at most, the size of a fill; a wave whose 64 arguments all underflow skips it.
//   k_vel_u              U (Npad x Tpad, Tpad = c E padded to 128): column (k, e) from the partial buffer, the slots of
//                        epoch e in ascending order (= ascending tile column); rows >= N and columns >= c E exact zeros
//   k_vel_v              V = G U on the fp64 MFMA tile engine, 2 N^2 Tpad flops
//   k_vel_gram           U^T V in the accumulators, the tiles on and below the diagonal
//   k_vel_newton_finish  T_k and g from the bin sums, row sums over the slots in ascending order, and
//                        J = (U^T V - F) + T for (k, e) >= (j, f), mirrored: J == J^T bit for bit
//
// Registers and scratch: k_vel_pair is scalar fp64 code with three accumulators per thread, 62 VGPRs, 6656 bytes of static
// LDS (the nine 128-entry arrays) and no dynamic LDS; k_vel_v and k_vel_gram are a K-loop of the tile engine and a store
// (155 VGPRs, the 128 accumulator VGPRs of every tile kernel among them, GEMM_LDS_BYTES of dynamic LDS); k_vel_u takes 10
// VGPRs and k_vel_newton_finish 28; none has scratch or spills (DESIGN.md 3b'').  A tile of k_vel_pair with n column slots
// makes n flushes of two barriers and a 128-step LDS scan: at most 128 x 128 scan steps, for pixels in no epoch order.
// Workspace beyond psoap_chunk_fisher_vel's: c S Npad (Y) + 2 c S^2 (A, B) + 2 Npad Tpad (U, V) + Tpad^2 + (c E)^2 + c E
// doubles.  fp64 throughout, no atomics, every sum in an order fixed by (N, c, epoch_index).
#pragma once
#include "vel_fisher_kernels.hpp"

namespace psoap {

constexpr int VEL_PAIR_THREADS = NB;

__global__ __launch_bounds__(VEL_PAIR_THREADS) void k_vel_pair(
    const double* __restrict__ Kinv, const double* __restrict__ alpha, int Npad, int N, int P, int S,
    const double* __restrict__ lwl, const double* __restrict__ gp, const int* __restrict__ pixel_epoch,
    const int* __restrict__ slot_of, const int* __restrict__ slot_first, double* __restrict__ Ypart,
    double* __restrict__ Apart, double* __restrict__ Bpart)
{
    __shared__ double xcol[NB], acol[NB], ra[NB], rb[NB];
    __shared__ int ecol[NB], skey[NB], scol[NB], order[NB], rslot[NB];
    const int ti = blockIdx.x / P, tj = blockIdx.x % P, k = blockIdx.y;
    const int r = threadIdx.x;
    const int i0 = ti * NB, j0 = tj * NB;
    double p2, coef, w0, w2;
    {
#pragma clang fp contract(off)
        const double a = gp[2 * k], l = gp[2 * k + 1];      // (as k_vel_dv_fill)
        p2 = -0.5 * (C_KMS * C_KMS) / (l * l);
        coef = (a * a) * 2.0 * p2 / C_KMS;
        w0 = (a * a) * 2.0 * p2 / (C_KMS * C_KMS);
        w2 = (a * a) * 4.0 * (p2 * p2) / (C_KMS * C_KMS);
    }
    const double* x = lwl + (size_t)k * N;
    const int m = i0 + r, nc = j0 + r;
    const bool row_live = m < N;
    const double xm = row_live ? x[m] : 0.0, am = row_live ? alpha[m] : 0.0;
    const int em = row_live ? pixel_epoch[m] : -1;
    const int sf_i = slot_first[ti], sf_j = slot_first[tj];
    const int ns_i = slot_first[ti + 1] - sf_i, ns_j = slot_first[tj + 1] - sf_j;
    const int ncol = (N - j0 < NB) ? N - j0 : NB;
    const int cs = (nc < N) ? slot_of[nc] - sf_j : ns_j;      // columns >= N sort behind every slot and are never visited
    rslot[r] = row_live ? slot_of[m] - sf_i : -1;
    xcol[r] = (nc < N) ? x[nc] : 0.0;
    acol[r] = (nc < N) ? alpha[nc] : 0.0;
    ecol[r] = (nc < N) ? pixel_epoch[nc] : -2;
    skey[r] = cs;
    __syncthreads();
    {
        int rank = 0;
        for (int q = 0; q < NB; ++q) {
            const int s = skey[q];
            rank += (s < cs || (s == cs && q < r)) ? 1 : 0;
        }
        order[rank] = r;
        scol[rank] = cs;
    }
    __syncthreads();
    double* Yk = Ypart + (size_t)k * S * Npad;
    double* Ak = Apart + (size_t)k * S * S;
    double* Bk = Bpart + (size_t)k * S * S;
    double y = 0.0, sa = 0.0, sb = 0.0;
    for (int p = 0; p < ncol; ++p) {
        const int n = order[p], sj = scol[p];
        {
#pragma clang fp contract(off)
            const double d = xcol[n] - xm;
            double arg[1] = {p2 * d * d}, e[1];
            if (__builtin_amdgcn_ballot_w64(!(arg[0] <= -746.0)) != 0ull) exp_nonpos_batch<1>(arg, e);
            else e[0] = 0.0;
            const bool cross = row_live && em != ecol[n];
            const double dv = cross ? e[0] * (coef * d) : 0.0;
            const double w = cross ? e[0] * (w0 + w2 * (d * d)) : 0.0;
            const double an = acol[n];
            const double cmn = Kinv[(size_t)(j0 + n) * Npad + m] - am * an;      // K^-1 is symmetric bit for bit
            y += dv * an;
            sa += dv * cmn;
            sb += w * cmn;
        }
        if (p + 1 == ncol || scol[p + 1] != sj) {      // (the same for every thread) the column slot ends here
            Yk[(size_t)(sf_j + sj) * Npad + m] = y;
            ra[r] = sa;
            rb[r] = sb;
            __syncthreads();
            if (r < ns_i) {
                double ta = 0.0, tb = 0.0;
                for (int q = 0; q < NB; ++q)
                    if (rslot[q] == r) ta += ra[q], tb += rb[q];
                Ak[(size_t)(sf_i + r) * S + sf_j + sj] = ta;
                Bk[(size_t)(sf_i + r) * S + sf_j + sj] = tb;
            }
            __syncthreads();
            y = sa = sb = 0.0;
        }
    }
}

// U[m][(k, e)] = [m in e] sum over all slots a of Y_k[a][m] - sum over the slots a of epoch e of Y_k[a][m], both in ascending
// slot order.  grid (ceil(Npad / 256), Tpad), 256 threads: a thread per row of one column.
__global__ __launch_bounds__(256) void k_vel_u(const double* __restrict__ Ypart, int Npad, int N, int S, int C, int E, int Tpad,
                                               const int* __restrict__ pixel_epoch, const int* __restrict__ epoch_ptr,
                                               const int* __restrict__ epoch_slots, double* __restrict__ U)
{
    const int m = blockIdx.x * 256 + threadIdx.x, col = blockIdx.y;
    if (m >= Npad) return;
    double out = 0.0;
    if (m < N && col < C * E) {
        const int k = col / E, e = col % E;
        const double* Yk = Ypart + (size_t)k * S * Npad;
        double s = 0.0;
        for (int ia = epoch_ptr[e]; ia < epoch_ptr[e + 1]; ++ia) s += Yk[(size_t)epoch_slots[ia] * Npad + m];
        double q = 0.0;
        if (pixel_epoch[m] == e)
            for (int a = 0; a < S; ++a) q += Yk[(size_t)a * Npad + m];
        out = q - s;
    }
    U[(size_t)m * Tpad + col] = out;
}

// V = G U: V[q][t] = sum_i G[i][q] U[i][t].  grid (P, Tpad / 128)
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_vel_v(const double* __restrict__ Kinv, const double* __restrict__ U, int Npad,
                                                          int Tpad, double* __restrict__ V)
{
    const int tq = blockIdx.x, tt = blockIdx.y;
    Tile t;
    t.zero();
    tile_gemm_tn(t, Kinv + NB * tq, (size_t)Npad, U + NB * tt, (size_t)Tpad, Npad);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double* p0 = V + (size_t)(NB * tq + tile_row(wr, m, lane, r)) * Tpad + NB * tt + tile_col(wc, 0, lane);
#pragma unroll
            for (int n = 0; n < 4; ++n) p0[16 * n] = t.acc[m][n][r];
        }
}

// M = U^T V, the tiles with ts >= tt: M[s][t] = sum_i U[i][s] V[i][t].  grid (Tpad / 128, Tpad / 128)
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_vel_gram(const double* __restrict__ U, const double* __restrict__ V, int Npad,
                                                             int Tpad, double* __restrict__ M)
{
    const int ts = blockIdx.x, tt = blockIdx.y;
    if (tt > ts) return;
    Tile t;
    t.zero();
    tile_gemm_tn(t, U + NB * ts, (size_t)Tpad, V + NB * tt, (size_t)Tpad, Npad);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double* p0 = M + (size_t)(NB * ts + tile_row(wr, m, lane, r)) * Tpad + NB * tt + tile_col(wc, 0, lane);
#pragma unroll
            for (int n = 0; n < 4; ++n) p0[16 * n] = t.acc[m][n][r];
        }
}

// J[(k, e), (j, f)] = (M - F) + T for (k, e) >= (j, f), mirrored, and on the diagonal g[(k, e)].  One thread per entry
// (grid ceil(T T / 64), 64 threads; T = c E).  An epoch without pixels has no slot: an exactly-zero row and column.
__global__ __launch_bounds__(64) void k_vel_newton_finish(const double* __restrict__ Apart, const double* __restrict__ Bpart,
                                                          const double* __restrict__ M, const double* __restrict__ F, int S, int C,
                                                          int E, int Tpad, const int* __restrict__ epoch_ptr,
                                                          const int* __restrict__ epoch_slots, double* __restrict__ J,
                                                          double* __restrict__ grad)
{
    const long long T = (long long)C * E;
    const long long idx = (long long)blockIdx.x * 64 + threadIdx.x;
    if (idx >= T * T) return;
    const int s = (int)(idx / T), u = (int)(idx % T);
    if (s < u) return;
    const int k = s / E, e = s % E, j = u / E, f = u % E;
    const int e0 = epoch_ptr[e], e1 = epoch_ptr[e + 1], f0 = epoch_ptr[f], f1 = epoch_ptr[f + 1];
    double tt = 0.0;
    if (k == j) {
        const double* Bk = Bpart + (size_t)k * S * S;
        if (e != f) {
            double b = 0.0;
            for (int ia = e0; ia < e1; ++ia)
                for (int ib = f0; ib < f1; ++ib) b += Bk[(size_t)epoch_slots[ia] * S + epoch_slots[ib]];
            tt = -b;
        } else {
            const double* Ak = Apart + (size_t)k * S * S;
            double b = 0.0, a = 0.0;
            for (int sb = 0; sb < S; ++sb)
                for (int ia = e0; ia < e1; ++ia) {
                    b += Bk[(size_t)epoch_slots[ia] * S + sb];
                    a += Ak[(size_t)epoch_slots[ia] * S + sb];
                }
            tt = b;
            grad[s] = -a;
        }
    }
    const double out = (M[(size_t)s * Tpad + u] - F[(size_t)s * T + u]) + tt;
    J[(size_t)s * T + u] = out;
    J[(size_t)u * T + s] = out;
}

inline hipError_t vel_newton_configure_kernels()
{
    const int lds = (int)GEMM_LDS_BYTES;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_vel_v), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_vel_gram), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    return e;
}

// the workspace of psoap_chunk_info_vel beyond psoap_chunk_fisher_vel's (grow-only; psoap_chunk_fisher_vel_release frees both)
struct VelNewtonWs {
    Grow<double> Y, A, B, U, V, M, J, Grad;
};

}  // namespace psoap
