// fisher_kernels.hpp -- Fisher information of the GP likelihood (not in the reference).
//
//   F_st = 1/2 tr(K^-1 K_s K^-1 K_t) = 1/2 sum_mn K_s[m,n] G_t[m,n],  G_t = K^-1 K_t K^-1
// for tangents t = (dx_t (c, N), da_tc, dl_tc) in (grid, hyper-parameter) space, with d = x_c[n] - x_c[m], e_cmn = exp(p_c d^2):
//   K_t[m,n] = sum_c e_cmn (2 a_c da_tc + a_c^2 c_kms^2 / l_c^3 d^2 dl_tc + a_c^2 2 p_c d (dx_tc[n] - dx_tc[m]))
// F is positive semi-definite and does not depend on the data.  F_mu = 1^T K^-1 1 is the information of mu_GP.
//
// The staged factorisation of [K | I] runs as for the gradient (grad_kernels.hpp) and leaves W = U^-T.  Then
//   k_fisher_kinv             K^-1 = W^T W, tile by tile with the K-loop bounds of k_grad_contract, stored with both triangles
//                             (rows and columns >= N come out as the identity: K is the identity there)
//   per tangent t:
//   k_fisher_tangent_fill<C>  K_t, every tile, exp() as the fills evaluate it; rows and columns >= N exact zeros
//   k_fisher_gemm             Z = K_t K^-1 (every tile, K = Npad)
//   k_fisher_contract<C>      one workgroup per upper tile of G_t = 1/2 (K^-1 Z + Z^T K^-1), formed in the MFMA accumulators
//                             and never stored
//   k_grad_finish             (the gradient's, as it is) the tiles' sums in tile order
//   k_fisher_dot              F_st = tan_s . g_t for every s >= t, mirrored: F == F^T bit for bit
// The contraction's epilogue is the gradient's, grad_contract_epilogue with ContractQ::Fisher.
//
// K_s is linear in its tangent, so <K_s, G_t> is taken one factor at a time: k_fisher_contract contracts G_t with the
// derivative of K with respect to every hyper-parameter and every grid point -- the sums of k_grad_contract with Q = G_t:
//   g_t[theta] = 1/2 sum_mn G_t[m,n] dK[m,n]/dtheta,   F_st = sum_theta tan_s[theta] g_t[theta]
// 2c + c N numbers per tangent.  Forming K_s for every s >= t in the epilogue instead would ask for the 2 x 128 x c grid
// tangents of every s in LDS (192 KiB at T = 32, c = 3: more than a compute unit has) and T / 2 times the epilogue's
// arithmetic; the contraction with the derivatives costs what one gradient's does, whatever T is.  g_t depends on tangent t
// alone and F_st on (s, t) alone: a subsequence of the tangents gives the same bits in the entries it shares.
//
// G_t is symmetric, K^-1 Z is so only up to rounding, and an upper tile stands for its mirror image too: contracted as it
// comes, the antisymmetric part of the rounding error does not cancel (measured on the host in float64 at N = 300: errors of
// 4e-13 .. 1.6e-12 sqrt(F_ss F_tt) in the amplitude entries against 4e-14 .. 9e-14 for the symmetrised product).  So the
// contraction runs both K-loops, K^-1 Z and Z^T K^-1, into one accumulator tile: N^3 flops more per tangent, no storage.
//
// Workspace beyond [K | I]: THREE Npad^2 matrices (K^-1, K_t, Z) whatever T is -- 24 Npad^2 bytes, 869 MB at N = 6000 --
// plus (T + 1) (c N + 2 c) doubles of tangents and their contractions and the gradient's per-tile sums.
// Flops: the factorisation of [K | I] 2/3 N^3, K^-1 1/3 N^3, per tangent 2 N^3 (Z) + 2 N^3 (the upper tiles of G_t, two K-loops):
//   F_fisher(N, T) = (1 + 4 T) N^3.
// fp64 throughout, no atomics, every sum in an order fixed by (N, c, T).
//
// Under the time-variable kernel of fill_kernels.hpp (psoap_chunk_fisher_tv)
//   K_ij = sum_c a_c^2 e_cij + sigma_i^2 delta_ij,   e_cij = exp(p_c d_cij^2 + q_c dt_ij^2),   q_c = -1/2 / tau_c^2
// a tangent is t = (dx_t (c, N), da_tc, dl_tc, dtau_tc), and with dt = t[n] - t[m]
//   K_t[m,n] = sum_c e_cmn (2 a_c da_tc + a_c^2 c_kms^2 / l_c^3 d^2 dl_tc + a_c^2 2 p_c d (dx_tc[n] - dx_tc[m])
//                           + a_c^2 / tau_c^3 dt^2 dtau_tc)
// The launch sequence is the one above on [K | I] factored under the time-variable fill (Factored::tv), with the TV = true
// wrappers of the same two bodies and the time-variable finishing sums:
//   k_tv_fisher_tangent_fill<C>  the row times in LDS beside xrow / drow, two column times per lane, the fourth coefficient
//   k_tv_fisher_contract<C>      the tile's row and column times in LDS, the combined argument, one more hyper sum per
//                                component, sum w q e dt^2, in a GradTile<true> record
//   k_tv_grad_finish             (the time-variable gradient's, as it is) leaves g_t[tau_c] beside g_t[gp] and g_t[x]
//   k_fisher_dot                 with tan_tau and g_tau: c N + 3 c numbers
// The argument of every exp() is formed as k_fill_sym_tv forms it: a = p2 * d * d, then a = a + q2 * dt * dt, without
// contraction, one exp, the wave-uniform <= -746 shortcut on the combined argument.
//
// tau_c = +inf is the static model, bit for bit.  q2 = -0, so q2 * dt * dt = -0 whatever the sign of dt and a + (-0) = a;
// ct = a^2 / inf * dtau = 0 whatever dtau is, and its term is ADDED LAST to the static sum of the fill, s + ct * dt^2 = s
// (fused or not: the product is an exact zero); the contraction's new sum st goes nowhere near sa, sl or the row and column
// sums; k_tv_grad_finish gives g_t[tau_c] = (1/2 a^2 / inf) * st = 0; and the dot adds the tau terms AFTER the static ones,
// r + 0 = r.  So with every tau = inf the entries of F have the bits of psoap_chunk_fisher whatever tan_tau holds, and a
// tangent with nothing but dtau gives K_t = 0 and an exactly-zero row and column.
//
// Under the quasi-periodic kernel (psoap_chunk_fisher_qp), e_cij = exp(p_c d^2 + q_c dt^2 - Gamma_c s^2) with
// s, co = sincospi(dt / P_c), a tangent is t = (dx_t, da_tc, dl_tc, dtau_tc, dGamma_tc, dP_tc) and K_t gains
//   e_cmn (-a_c^2 s^2 dGamma_tc + a_c^2 Gamma_c pi / P_c^2 dt (2 s co) dP_tc)
// The launch sequence is the time-variable one on [K | I] factored under the quasi-periodic fill (Factored::qp):
//   k_qp_fisher_tangent_fill<C>  the time-variable tangent fill with the periodic term in the argument and two coefficients more
//   k_qp_fisher_contract<C>      the two K loops, then qp_contract_epilogue<C, ContractQ::Fisher> (grad_kernels.hpp): a QpTile
//                                record with the five hyper sums per component
//   k_qp_grad_finish             (the quasi-periodic gradient's, as it is) leaves g_t[Gamma_c] and g_t[P_c] beside the rest
//   k_qp_fisher_dot              k_fisher_dot's sums in its order, then the c Gamma terms, then the c period terms
// Gamma_c = 0 for every c with dGamma = 0 is the time-variable call, bit for bit, whatever P and dP are: ng = -0 leaves the
// argument as it is, cg = -a^2 0 and cq = a^2 0 pi / P^2 dP are zeros added behind the time-variable sum, the contraction's sa,
// sl, st and row and column sums are formed by the time-variable operations on the same e, k_qp_grad_finish gives
// g_t[P_c] = 0, and the dot's last 2c steps add exact zeros.  A tangent with nothing but dP_c of a component with Gamma_c = 0
// gives K_t = 0 and an exactly-zero row and column.
#pragma once
#include "grad_kernels.hpp"

namespace psoap {

constexpr int FISHER_MAX_T = 32;

// the upper tile (ti, tj) of a symmetric matrix out of the accumulators, and its mirror image (a diagonal tile: its upper
// half, both ways)
__device__ __forceinline__ void fisher_kinv_store(const Tile& t, int ti, int tj, int Npad, double* __restrict__ Kinv)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = tile_row(wr, m, lane, r), col = tile_col(wc, n, lane);
                if (ti != tj || row <= col) {
                    const double v = t.acc[m][n][r];
                    Kinv[(size_t)(NB * ti + row) * Npad + NB * tj + col] = v;
                    Kinv[(size_t)(NB * tj + col) * Npad + NB * ti + row] = v;
                }
            }
}

// K^-1 = W^T W.  grid P (P + 1) / 2: the upper tile (ti, tj) and its mirror image
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_fisher_kinv(const double* __restrict__ A, int ld, int Npad, int P,
                                                                double* __restrict__ Kinv)
{
    int ti, tj;
    decode_upper(blockIdx.x, P, ti, tj);
    const double* W = A + Npad + (size_t)NB * tj * ld;
    Tile t;
    t.zero();
    tile_gemm_tn(t, W + NB * ti, (size_t)ld, W + NB * tj, (size_t)ld, Npad - NB * tj);
    fisher_kinv_store(t, ti, tj, Npad, Kinv);
}

// K_t, every tile (grid P P), in the layout of k_fill_sym: wave w owns the 32-column block w, a lane four rows x two columns
// per step, the eight exponentials of a component through one batched, underflow-skipping evaluation.  TV: the row times in
// LDS beside xrow / drow, two column times per lane, the fourth coefficient ct[c] = a_c^2 / tau_c^3 dtau_tc.
// QP (with TV): the periodic term in the argument as k_fill_sym_qp forms it -- u = dt * rP, sincospi, a = a + ng * s * s, the
// underflow shortcut on the two-term argument first and then on the full one -- and two more coefficients,
// cg[c] = -a_c^2 dGamma_tc of e s^2 and cq[c] = a_c^2 Gamma_c pi / P_c^2 dP_tc of e dt (2 s co).  s^2 and 2 s co of the eight
// elements are kept across the exp: this kernel holds no accumulator tile.
template <int C, bool TV, bool QP = false>
__device__ __forceinline__ void fisher_tangent_fill_tile(double* __restrict__ Kt, int Npad, int N, int P,
                                                         const double* __restrict__ lwl, const double* __restrict__ times,
                                                         const double* __restrict__ gp, const double* __restrict__ tau,
                                                         const double* __restrict__ tan_x, const double* __restrict__ tan_gp,
                                                         const double* __restrict__ tan_tau,
                                                         const double* __restrict__ gam = nullptr,
                                                         const double* __restrict__ per = nullptr,
                                                         const double* __restrict__ tan_gamma = nullptr,
                                                         const double* __restrict__ tan_period = nullptr)
{
    static_assert(TV || !QP, "the periodic factor stands on the temporal one");
    __shared__ double xrow[C][NB];
    __shared__ double drow[C][NB];
    __shared__ double trow[TV ? NB : 1];      // (static: never referenced, and not allocated)
    const int ti = blockIdx.x / P, tj = blockIdx.x % P;
    const int tid = threadIdx.x;
    const int i0 = ti * NB, j0 = tj * NB;
    GpDev g;
    load_gp(gp, C, g);
    double ca[C], cl[C], cx[C];      // the coefficients of e, e d^2 and e d (dx[n] - dx[m])
    [[maybe_unused]] double q2[C], ct[C];      // TV: q_c and the coefficient of e dt^2
    [[maybe_unused]] double rP[C], ng[C], cg[C], cq[C];      // QP: 1 / P_c, -Gamma_c and the coefficients of e s^2, e dt (2 s co)
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double a = gp[2 * c], l = gp[2 * c + 1];
        ca[c] = 2.0 * a * tan_gp[2 * c];
        cl[c] = g.a2[c] * (C_KMS * C_KMS) / (l * l * l) * tan_gp[2 * c + 1];
        cx[c] = g.a2[c] * 2.0 * g.p2[c];
        if constexpr (TV) {
            const double tc = tau[c];
            q2[c] = tv_q2(tc);
            ct[c] = g.a2[c] / (tc * tc * tc) * tan_tau[c];
        }
        if constexpr (QP) {
            const double G = gam[c], Pc = per[c];
            rP[c] = qp_rp(Pc);
            ng[c] = qp_ng(G);
            cg[c] = -g.a2[c] * tan_gamma[c];
            cq[c] = g.a2[c] * G * 3.14159265358979323846 / (Pc * Pc) * tan_period[c];
        }
    }
    if (tid < NB) {
        const int i = i0 + tid;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            xrow[c][tid] = (i < N) ? lwl[(size_t)c * N + i] : 0.0;
            drow[c][tid] = (i < N) ? tan_x[(size_t)c * N + i] : 0.0;
        }
        if constexpr (TV) trow[tid] = (i < N) ? times[i] : 0.0;
    }
    const int w = tid >> 6, rg = (tid >> 4) & 3, cp = tid & 15;
    const int ja = j0 + 32 * w + 2 * cp, jb = ja + 1;
    double xa[C], xb[C], da[C], db[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        xa[c] = (ja < N) ? lwl[(size_t)c * N + ja] : 0.0;
        xb[c] = (jb < N) ? lwl[(size_t)c * N + jb] : 0.0;
        da[c] = (ja < N) ? tan_x[(size_t)c * N + ja] : 0.0;
        db[c] = (jb < N) ? tan_x[(size_t)c * N + jb] : 0.0;
    }
    [[maybe_unused]] double ta, tb;
    if constexpr (TV) {
        ta = (ja < N) ? times[ja] : 0.0;
        tb = (jb < N) ? times[jb] : 0.0;
    }
    __syncthreads();
#pragma unroll 1
    for (int g4 = 0; g4 < NB / 16; ++g4) {
        double va[4] = {0.0, 0.0, 0.0, 0.0}, vb[4] = {0.0, 0.0, 0.0, 0.0};
        [[maybe_unused]] double dta[4], dtb[4];
        if constexpr (TV) {
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const double tr = trow[16 * g4 + rg + 4 * s4];
                dta[s4] = ta - tr;
                dtb[s4] = tb - tr;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            double d[8], a[8], e[8];
            bool live = false;
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
#pragma clang fp contract(off)
                const double xi = xrow[c][16 * g4 + rg + 4 * s4];
                d[2 * s4] = xa[c] - xi;
                d[2 * s4 + 1] = xb[c] - xi;
                a[2 * s4] = g.p2[c] * d[2 * s4] * d[2 * s4];
                if constexpr (TV) a[2 * s4] = a[2 * s4] + q2[c] * dta[s4] * dta[s4];
                a[2 * s4 + 1] = g.p2[c] * d[2 * s4 + 1] * d[2 * s4 + 1];
                if constexpr (TV) a[2 * s4 + 1] = a[2 * s4 + 1] + q2[c] * dtb[s4] * dtb[s4];
                live = live || !(a[2 * s4] <= -746.0) || !(a[2 * s4 + 1] <= -746.0);
            }
            if (__builtin_amdgcn_ballot_w64(live) == 0ull) continue;      // exp() = +0 for the whole wave
            [[maybe_unused]] double s2[8], sc[8];      // QP: s^2 and 2 s co of the element
            if constexpr (QP) {
                live = false;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
#pragma clang fp contract(off)
                    const double u = ((k & 1) ? dtb[k >> 1] : dta[k >> 1]) * rP[c];
                    double s, co;
                    sincospi(u, &s, &co);
                    a[k] = a[k] + ng[c] * s * s;
                    live = live || !(a[k] <= -746.0);
                    s2[k] = s * s;
                    sc[k] = 2.0 * s * co;
                }
                if (__builtin_amdgcn_ballot_w64(live) == 0ull) continue;
            }
            exp_nonpos_batch<8>(a, e);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const double di = drow[c][16 * g4 + rg + 4 * s4];
                const double ua = d[2 * s4], ub = d[2 * s4 + 1];
                double sa = ca[c] + cl[c] * (ua * ua) + cx[c] * (ua * (da[c] - di));
                double sb = ca[c] + cl[c] * (ub * ub) + cx[c] * (ub * (db[c] - di));
                if constexpr (TV) {
                    // the static sum first, the temporal term last: at tau = inf it adds an exact zero.  (The opaque statement
                    // ends the static expression where the static kernel ends it: what is fused into multiply-adds inside
                    // it does not depend on the term that follows.)
                    asm volatile("" : "+v"(sa), "+v"(sb));
                    sa = sa + ct[c] * (dta[s4] * dta[s4]);
                    sb = sb + ct[c] * (dtb[s4] * dtb[s4]);
                }
                if constexpr (QP) {
                    // the time-variable sum first, the periodic terms last, behind an opaque statement of their own: with
                    // Gamma_c = 0 and dGamma_tc = 0 both add exact zeros, whatever P_c and dP_tc are
                    asm volatile("" : "+v"(sa), "+v"(sb));
                    sa = sa + cg[c] * s2[2 * s4];
                    sb = sb + cg[c] * s2[2 * s4 + 1];
                    sa = sa + cq[c] * (dta[s4] * sc[2 * s4]);
                    sb = sb + cq[c] * (dtb[s4] * sc[2 * s4 + 1]);
                }
                va[s4] += e[2 * s4] * sa;
                vb[s4] += e[2 * s4 + 1] * sb;
            }
        }
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int i = i0 + 16 * g4 + rg + 4 * s4;
            d2 v;
            v.x = (i < N && ja < N) ? va[s4] : 0.0;
            v.y = (i < N && jb < N) ? vb[s4] : 0.0;
            *reinterpret_cast<d2*>(Kt + (size_t)i * Npad + ja) = v;
        }
    }
}

// (one argument list for both, so that fisher_run launches either the same way: the static kernel reads none of times, tau
// and tan_tau)
template <int C>
__global__ __launch_bounds__(256) void k_fisher_tangent_fill(double* __restrict__ Kt, int Npad, int N, int P,
                                                             const double* __restrict__ lwl, const double* __restrict__ times,
                                                             const double* __restrict__ gp, const double* __restrict__ tau,
                                                             const double* __restrict__ tan_x, const double* __restrict__ tan_gp,
                                                             const double* __restrict__ tan_tau)
{
    fisher_tangent_fill_tile<C, false>(Kt, Npad, N, P, lwl, times, gp, tau, tan_x, tan_gp, tan_tau);
}

template <int C>
__global__ __launch_bounds__(256) void k_tv_fisher_tangent_fill(double* __restrict__ Kt, int Npad, int N, int P,
                                                                const double* __restrict__ lwl, const double* __restrict__ times,
                                                                const double* __restrict__ gp, const double* __restrict__ tau,
                                                                const double* __restrict__ tan_x,
                                                                const double* __restrict__ tan_gp,
                                                                const double* __restrict__ tan_tau)
{
    fisher_tangent_fill_tile<C, true>(Kt, Npad, N, P, lwl, times, gp, tau, tan_x, tan_gp, tan_tau);
}

// ... under the quasi-periodic kernel (psoap_chunk_fisher_qp): gam, per (c) and the tangent's dGamma, dP (c) behind tan_tau
template <int C>
__global__ __launch_bounds__(256) void k_qp_fisher_tangent_fill(double* __restrict__ Kt, int Npad, int N, int P,
                                                                const double* __restrict__ lwl, const double* __restrict__ times,
                                                                const double* __restrict__ gp, const double* __restrict__ tau,
                                                                const double* __restrict__ gam, const double* __restrict__ per,
                                                                const double* __restrict__ tan_x,
                                                                const double* __restrict__ tan_gp,
                                                                const double* __restrict__ tan_tau,
                                                                const double* __restrict__ tan_gamma,
                                                                const double* __restrict__ tan_period)
{
    fisher_tangent_fill_tile<C, true, true>(Kt, Npad, N, P, lwl, times, gp, tau, tan_x, tan_gp, tan_tau, gam, per, tan_gamma,
                                            tan_period);
}

// Z = K_t K^-1: Z[m][n] = sum_k K_t[k][m] K^-1[k][n] (K_t is symmetric, so its block columns are the k-major operand).
// grid P P
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_fisher_gemm(const double* __restrict__ Kt, const double* __restrict__ Kinv,
                                                                int Npad, int P, double* __restrict__ Z)
{
    const int tm = blockIdx.x / P, tn = blockIdx.x % P;
    Tile t;
    t.zero();
    tile_gemm_tn(t, Kt + NB * tm, (size_t)Npad, Kinv + NB * tn, (size_t)Npad, Npad);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double* p0 = Z + (size_t)(NB * tm + tile_row(wr, m, lane, r)) * Npad + NB * tn + tile_col(wc, 0, lane);
#pragma unroll
            for (int n = 0; n < 4; ++n) p0[16 * n] = t.acc[m][n][r];
        }
}

// One workgroup per upper tile (ti <= tj) of 2 G_t = K^-1 Z + Z^T K^-1, then the epilogue of the gradient's contraction
// (grad_contract_epilogue, ContractQ::Fisher) with q = G_t[i][j]: per component e_c = exp(p_c d^2), under TV
// exp(p_c d^2 + q_c dt^2), once per element, and the sums
//   hyper-parameters  sum w q e_c, sum w q e_c d^2, under TV sum w q e_c dt^2   (w = 2 off the diagonal: the element stands for
//                     (i,j) and (j,i); 1 on it)
//   rows of block ti  sum_j q e_c d;     rows of block tj  -sum_i q e_c d
// in the tile's own GradTile<TV>::DOUBLES of `part` (the gradient's layout: k_grad_finish / k_tv_grad_finish add them up).  A
// diagonal tile takes i <= j only; rows and columns >= N are masked (G_t is exactly zero there).  grid P (P + 1) / 2
template <int C, bool TV>
__device__ __forceinline__ void fisher_contract_tile(const double* __restrict__ Kinv, const double* __restrict__ Z, int N, int Npad,
                                                     int P, const double* __restrict__ lwl, const double* __restrict__ times,
                                                     const double* __restrict__ gp, const double* __restrict__ tau,
                                                     double* __restrict__ part)
{
    int ti, tj;
    decode_upper(blockIdx.x, P, ti, tj);
    Tile t;
    t.zero();
    tile_gemm_tn(t, Kinv + NB * ti, (size_t)Npad, Z + NB * tj, (size_t)Npad, Npad, ti == tj);
    tile_gemm_tn(t, Z + NB * ti, (size_t)Npad, Kinv + NB * tj, (size_t)Npad, Npad, ti == tj);      // (+ its transpose's tile)
    grad_contract_epilogue<C, TV, ContractQ::Fisher>(t, 0, ti, tj, (int)blockIdx.x, N, Npad, P, lwl, gp, nullptr, part, times, tau);
}

// (one argument list for both, as the tangent fills)
template <int C>
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_fisher_contract(const double* __restrict__ Kinv, const double* __restrict__ Z,
                                                                    int N, int Npad, int P, const double* __restrict__ lwl,
                                                                    const double* __restrict__ times,
                                                                    const double* __restrict__ gp,
                                                                    const double* __restrict__ tau, double* __restrict__ part)
{
    fisher_contract_tile<C, false>(Kinv, Z, N, Npad, P, lwl, times, gp, tau, part);
}

template <int C>
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_tv_fisher_contract(const double* __restrict__ Kinv, const double* __restrict__ Z,
                                                                       int N, int Npad, int P, const double* __restrict__ lwl,
                                                                       const double* __restrict__ times,
                                                                       const double* __restrict__ gp,
                                                                       const double* __restrict__ tau, double* __restrict__ part)
{
    fisher_contract_tile<C, true>(Kinv, Z, N, Npad, P, lwl, times, gp, tau, part);
}

// The two K loops of fisher_contract_tile, then the quasi-periodic epilogue (qp_contract_epilogue of grad_kernels.hpp with
// ContractQ::Fisher): e_c with the periodic term, the five hyper sums per component, a QpTile record per tile for
// k_qp_grad_finish.  grid P (P + 1) / 2
template <int C>
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_qp_fisher_contract(const double* __restrict__ Kinv, const double* __restrict__ Z,
                                                                       int N, int Npad, int P, const double* __restrict__ lwl,
                                                                       const double* __restrict__ times,
                                                                       const double* __restrict__ gp,
                                                                       const double* __restrict__ tau,
                                                                       const double* __restrict__ gam,
                                                                       const double* __restrict__ per, double* __restrict__ part)
{
    int ti, tj;
    decode_upper(blockIdx.x, P, ti, tj);
    Tile t;
    t.zero();
    tile_gemm_tn(t, Kinv + NB * ti, (size_t)Npad, Z + NB * tj, (size_t)Npad, Npad, ti == tj);
    tile_gemm_tn(t, Z + NB * ti, (size_t)Npad, Kinv + NB * tj, (size_t)Npad, Npad, ti == tj);      // (+ its transpose's tile)
    qp_contract_epilogue<C, ContractQ::Fisher>(t, 0, ti, tj, (int)blockIdx.x, N, Npad, P, lwl, gp, nullptr, part, times, tau, gam,
                                               per);
}

// F_mu = 1^T K^-1 1 = |W 1|^2 in two fixed-order stages.  y[k] = sum of row k of W over its columns q <= k, q < N (the rest is
// exactly zero): thread j adds every 256th term, the 256 sums meet in a tree (block_sum_256).  grid N, 256 threads
__global__ __launch_bounds__(256) void k_fisher_w1(const double* __restrict__ A, int ld, int Npad, int N, double* __restrict__ y)
{
    __shared__ double red[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    const double* Wk = A + (size_t)k * ld + Npad;
    double s = 0.0;
    for (int q = tid; q <= k && q < N; q += 256) s += Wk[q];
    const double sum = block_sum_256(red, s);
    if (tid == 0) y[k] = sum;
}

// one workgroup of 256 threads: out = sum_k y[k]^2, the same way
__global__ __launch_bounds__(256) void k_fisher_mu(const double* __restrict__ y, int N, double* __restrict__ out)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int k = tid; k < N; k += 256) s = fma(y[k], y[k], s);
    const double sum = block_sum_256(red, s);
    if (tid == 0) *out = sum;
}

// F[s][t] = F[t][s] = tan_s . g_t for s >= t.  grid (T, T), 256 threads: the c N grid terms strided and met in a tree, then
// the 2c hyper-parameter terms one after the other, then (tan_tau, g_tau not nullptr) the c time-scale terms likewise.  g: what
// k_grad_finish / k_tv_grad_finish made of tangent t's tiles (g_gp (T, 2c), g_tau (T, c), g_x (T, c, N))
__global__ __launch_bounds__(256) void k_fisher_dot(const double* __restrict__ tan_x, const double* __restrict__ tan_gp,
                                                    const double* __restrict__ tan_tau, const double* __restrict__ g_x,
                                                    const double* __restrict__ g_gp, const double* __restrict__ g_tau, int C,
                                                    int N, int T, double* __restrict__ F)
{
    __shared__ double red[256];
    const int s = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    if (s < t) return;
    const size_t CN = (size_t)C * N;
    const double* ts = tan_x + (size_t)s * CN;
    const double* gt = g_x + (size_t)t * CN;
    double acc = 0.0;
    for (size_t i = tid; i < CN; i += 256) acc = fma(ts[i], gt[i], acc);
    double r = block_sum_256(red, acc);
    if (tid == 0) {
        for (int k = 0; k < 2 * C; ++k) r = fma(tan_gp[(size_t)s * 2 * C + k], g_gp[(size_t)t * 2 * C + k], r);
        if (tan_tau)
            for (int k = 0; k < C; ++k) r = fma(tan_tau[(size_t)s * C + k], g_tau[(size_t)t * C + k], r);
        F[(size_t)s * T + t] = r;
        F[(size_t)t * T + s] = r;
    }
}

// k_fisher_dot under the quasi-periodic kernel: the same sums in the same order -- the c N grid terms, the 2c hyper-parameter
// terms, the c time-scale terms -- then the c Gamma terms, then the c period terms.  With tan_gamma = 0 and g_period = 0 (every
// Gamma_c = 0) the last 2c steps leave r as it is.  grid (T, T), 256 threads
__global__ __launch_bounds__(256) void k_qp_fisher_dot(const double* __restrict__ tan_x, const double* __restrict__ tan_gp,
                                                       const double* __restrict__ tan_tau, const double* __restrict__ tan_gamma,
                                                       const double* __restrict__ tan_period, const double* __restrict__ g_x,
                                                       const double* __restrict__ g_gp, const double* __restrict__ g_tau,
                                                       const double* __restrict__ g_gamma, const double* __restrict__ g_period,
                                                       int C, int N, int T, double* __restrict__ F)
{
    __shared__ double red[256];
    const int s = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    if (s < t) return;
    const size_t CN = (size_t)C * N;
    const double* ts = tan_x + (size_t)s * CN;
    const double* gt = g_x + (size_t)t * CN;
    double acc = 0.0;
    for (size_t i = tid; i < CN; i += 256) acc = fma(ts[i], gt[i], acc);
    double r = block_sum_256(red, acc);
    if (tid == 0) {
        for (int k = 0; k < 2 * C; ++k) r = fma(tan_gp[(size_t)s * 2 * C + k], g_gp[(size_t)t * 2 * C + k], r);
        for (int k = 0; k < C; ++k) r = fma(tan_tau[(size_t)s * C + k], g_tau[(size_t)t * C + k], r);
        for (int k = 0; k < C; ++k) r = fma(tan_gamma[(size_t)s * C + k], g_gamma[(size_t)t * C + k], r);
        for (int k = 0; k < C; ++k) r = fma(tan_period[(size_t)s * C + k], g_period[(size_t)t * C + k], r);
        F[(size_t)s * T + t] = r;
        F[(size_t)t * T + s] = r;
    }
}

// the LDS attribute of every kernel here that takes the operand buffers
inline hipError_t fisher_configure_kernels()
{
    const void* const kernels[] = {
        reinterpret_cast<const void*>(k_fisher_kinv),           reinterpret_cast<const void*>(k_fisher_gemm),
        reinterpret_cast<const void*>(k_fisher_contract<1>),    reinterpret_cast<const void*>(k_fisher_contract<2>),
        reinterpret_cast<const void*>(k_fisher_contract<3>),    reinterpret_cast<const void*>(k_tv_fisher_contract<1>),
        reinterpret_cast<const void*>(k_tv_fisher_contract<2>), reinterpret_cast<const void*>(k_tv_fisher_contract<3>),
        reinterpret_cast<const void*>(k_qp_fisher_contract<1>), reinterpret_cast<const void*>(k_qp_fisher_contract<2>),
        reinterpret_cast<const void*>(k_qp_fisher_contract<3>)};
    for (const void* k : kernels)
        if (hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEMM_LDS_BYTES)) return e;
    return hipSuccess;
}

// the Fisher workspace of a chunk handle (grow-only; psoap_chunk_fisher_release frees it)
struct FisherWs {
    Grow<double> Kinv, Kt, Z, TanX, TanGp, Part, GGp, GX, Y, Mu, F;
    Grow<double> V;      // Vt 1 of the marginal form (marg_fisher_kernels.hpp)
    Grow<double> TanTau, GTau;      // the time-scale tangents (T, c) and their contractions (fisher_tv)
    Grow<double> TanGamma, TanPeriod, GGamma, GPeriod;      // those of Gamma and P likewise (fisher_qp)
    Grow<MatAcc> Info;
};

}  // namespace psoap
