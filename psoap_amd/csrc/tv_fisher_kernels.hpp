// tv_fisher_kernels.hpp -- Fisher information under the time-variable kernel of fill_kernels.hpp (not in the reference).
//
//   K_ij = sum_c a_c^2 e_cij + sigma_i^2 delta_ij,   e_cij = exp(p_c d_cij^2 + q_c dt_ij^2),   q_c = -1/2 / tau_c^2
// A tangent is t = (dx_t (c, N), da_tc, dl_tc, dtau_tc), and with d = x_c[n] - x_c[m], dt = t[n] - t[m]
//   K_t[m,n] = sum_c e_cmn (2 a_c da_tc + a_c^2 c_kms^2 / l_c^3 d^2 dl_tc + a_c^2 2 p_c d (dx_tc[n] - dx_tc[m])
//                           + a_c^2 / tau_c^3 dt^2 dtau_tc)
// F_st = 1/2 tr(K^-1 K_s K^-1 K_t) and F_mu = 1^T K^-1 1 as in fisher_kernels.hpp, whose launch sequence this is: [K | I]
// factored under the time-variable fill (Factored::tv), k_fisher_kinv, k_fisher_gemm, k_fisher_w1 and k_fisher_mu as they are,
// and per tangent
//   k_tv_fisher_tangent_fill<C>  k_fisher_tangent_fill with the row times in LDS beside xrow / drow, two column times per lane,
//                                and the fourth coefficient ct[c] = a_c^2 / tau_c^3 dtau_tc
//   k_tv_fisher_contract<C>      k_fisher_contract -- both K-loops of the symmetrised G_t -- with the epilogue of the
//                                time-variable gradient (grad_kernels.hpp): the tile's row and column times in LDS, the
//                                combined argument, one more hyper sum per component, sum w q e dt^2, in a GradTile<true> record
//   k_tv_grad_finish             (the time-variable gradient's, as it is) leaves g_t[tau_c] beside g_t[gp] and g_t[x]
//   k_tv_fisher_dot              F_st = tan_s . g_t over c N + 3 c numbers for s >= t, mirrored
// The argument of every exp() here is formed as k_fill_sym_tv forms it: a = p2 * d * d, then a = a + q2 * dt * dt, without
// contraction, one exp, the wave-uniform <= -746 shortcut on the combined argument.
//
// tau_c = +inf is the static model, bit for bit.  q2 = -0, so q2 * dt * dt = -0 whatever the sign of dt and a + (-0) = a;
// ct = a^2 / inf * dtau = 0 whatever dtau is, and its term is ADDED LAST to the static sum of the fill, s + ct * dt^2 = s
// (fused or not: the product is an exact zero); the contraction's new sum st goes nowhere near sa, sl or the row and column
// sums; k_tv_grad_finish gives g_t[tau_c] = (1/2 a^2 / inf) * st = 0; and the dot adds the tau terms AFTER the static ones,
// r + 0 = r.  So with every tau = inf the entries of F have the bits of psoap_chunk_fisher whatever tan_tau holds, and a
// tangent with nothing but dtau gives K_t = 0 and an exactly-zero row and column.
//
// These are second kernels beside the static ones, as k_fill_sym_tv stands beside k_fill_sym: the static kernels keep their
// instructions (profiles/timevar_fisher.md).  fp64 throughout, no atomics, every sum in an order fixed by (N, c, T); g_t
// depends on tangent t alone.
#pragma once
#include "fisher_kernels.hpp"

namespace psoap {

// K_t under the time-variable kernel, every tile (grid P P): k_fisher_tangent_fill's layout and order of operations.
template <int C>
__global__ __launch_bounds__(256) void k_tv_fisher_tangent_fill(double* __restrict__ Kt, int Npad, int N, int P,
                                                                const double* __restrict__ lwl, const double* __restrict__ times,
                                                                const double* __restrict__ gp, const double* __restrict__ tau,
                                                                const double* __restrict__ tan_x,
                                                                const double* __restrict__ tan_gp,
                                                                const double* __restrict__ tan_tau)
{
    __shared__ double xrow[C][NB];
    __shared__ double drow[C][NB];
    __shared__ double trow[NB];
    const int ti = blockIdx.x / P, tj = blockIdx.x % P;
    const int tid = threadIdx.x;
    const int i0 = ti * NB, j0 = tj * NB;
    GpDev g;
    load_gp(gp, C, g);
    double q2[C];
    double ca[C], cl[C], cx[C], ct[C];      // the coefficients of e, e d^2, e d (dx[n] - dx[m]) and e dt^2
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double a = gp[2 * c], l = gp[2 * c + 1], tc = tau[c];
        q2[c] = tv_q2(tc);
        ca[c] = 2.0 * a * tan_gp[2 * c];
        cl[c] = g.a2[c] * (C_KMS * C_KMS) / (l * l * l) * tan_gp[2 * c + 1];
        cx[c] = g.a2[c] * 2.0 * g.p2[c];
        ct[c] = g.a2[c] / (tc * tc * tc) * tan_tau[c];
    }
    if (tid < NB) {
        const int i = i0 + tid;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            xrow[c][tid] = (i < N) ? lwl[(size_t)c * N + i] : 0.0;
            drow[c][tid] = (i < N) ? tan_x[(size_t)c * N + i] : 0.0;
        }
        trow[tid] = (i < N) ? times[i] : 0.0;
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
    const double ta = (ja < N) ? times[ja] : 0.0, tb = (jb < N) ? times[jb] : 0.0;
    __syncthreads();
#pragma unroll 1
    for (int g4 = 0; g4 < NB / 16; ++g4) {
        double va[4] = {0.0, 0.0, 0.0, 0.0}, vb[4] = {0.0, 0.0, 0.0, 0.0};
        double dta[4], dtb[4];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const double tr = trow[16 * g4 + rg + 4 * s4];
            dta[s4] = ta - tr;
            dtb[s4] = tb - tr;
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
                a[2 * s4] = a[2 * s4] + q2[c] * dta[s4] * dta[s4];
                a[2 * s4 + 1] = g.p2[c] * d[2 * s4 + 1] * d[2 * s4 + 1];
                a[2 * s4 + 1] = a[2 * s4 + 1] + q2[c] * dtb[s4] * dtb[s4];
                live = live || !(a[2 * s4] <= -746.0) || !(a[2 * s4 + 1] <= -746.0);
            }
            if (__builtin_amdgcn_ballot_w64(live) == 0ull) continue;      // exp() = +0 for the whole wave
            exp_nonpos_batch<8>(a, e);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const double di = drow[c][16 * g4 + rg + 4 * s4];
                const double ua = d[2 * s4], ub = d[2 * s4 + 1];
                // the static sum first, as k_fisher_tangent_fill writes it, the temporal term last: at tau = inf it adds an exact
                // zero.  (The opaque statement ends the static expression where the static kernel ends it: what is fused
                // into multiply-adds inside it does not depend on the term that follows.)
                double sa = ca[c] + cl[c] * (ua * ua) + cx[c] * (ua * (da[c] - di));
                double sb = ca[c] + cl[c] * (ub * ub) + cx[c] * (ub * (db[c] - di));
                asm volatile("" : "+v"(sa), "+v"(sb));
                sa = sa + ct[c] * (dta[s4] * dta[s4]);
                sb = sb + ct[c] * (dtb[s4] * dtb[s4]);
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

// One workgroup per upper tile (ti <= tj) of 2 G_t = K^-1 Z + Z^T K^-1, as k_fisher_contract, then the epilogue of
// k_tv_grad_contract with q = G_t[i][j] in place of alpha_i alpha_j - (K^-1)_ij: per component e_c = exp(p_c d^2 + q_c dt^2)
// once per element and the sums
//   hyper-parameters  sum w q e_c, sum w q e_c d^2, sum w q e_c dt^2   (w = 2 off the diagonal, 1 on it)
//   rows of block ti  sum_j q e_c d;     rows of block tj  -sum_i q e_c d
// in the tile's own GradTile<true>::DOUBLES of `part`, in the order k_tv_grad_finish reads them.  The LDS map is GradTile<true>'s
// (its alpha rows stay unused); a diagonal tile takes i <= j only; rows and columns >= N are masked.
template <int C>
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_tv_fisher_contract(const double* __restrict__ Kinv, const double* __restrict__ Z,
                                                                       int N, int Npad, int P, const double* __restrict__ lwl,
                                                                       const double* __restrict__ times,
                                                                       const double* __restrict__ gp,
                                                                       const double* __restrict__ tau, double* __restrict__ part)
{
    using L = GradTile<true>;
    constexpr int XS = L::XS, TS = L::TS, RS = L::RS, CS = L::CS, HS = L::HS, WS = L::WS;
    static_assert(TS >= XS + 6 * NB && RS >= TS + 2 * NB && (HS + 4 * WS) * sizeof(double) <= GEMM_LDS_BYTES,
                  "the epilogue with its two time arrays fits the operand buffers");
    int ti, tj;
    decode_upper(blockIdx.x, P, ti, tj);
    Tile t;
    t.zero();
    tile_gemm_tn(t, Kinv + NB * ti, (size_t)Npad, Z + NB * tj, (size_t)Npad, Npad, ti == tj);
    tile_gemm_tn(t, Z + NB * ti, (size_t)Npad, Kinv + NB * tj, (size_t)Npad, Npad, ti == tj);      // (+ its transpose's tile)

    const int tid = threadIdx.x;
    {
        const int side = tid >> 7, idx = tid & 127;
        const int g = NB * (side ? tj : ti) + idx;
#pragma unroll
        for (int c = 0; c < C; ++c) psoap_smem[XS + (side * 3 + c) * NB + idx] = (g < N) ? lwl[(size_t)c * N + g] : 0.0;
        psoap_smem[TS + side * NB + idx] = (g < N) ? times[g] : 0.0;
    }
    __syncthreads();
    const bool diag_tile = ti == tj;
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        // (the thread id passes through an opaque statement in every turn: the rows, columns, masks and weights derived from
        // it are formed again per component and not kept across the loop -- 64 predicates and weights held live beside the
        // accumulators are registers the kernel does not have)
        int tl = tid;
        asm volatile("" : "+v"(tl));
        const int ln = tl & 63, wave = tl >> 6;
        const int wr = wave >> 1, wc = wave & 1;
        double p2;
        {
#pragma clang fp contract(off)
            const double l = gp[2 * c + 1];      // (as load_gp rounds it)
            p2 = -0.5 * (C_KMS * C_KMS) / (l * l);
        }
        const double q2 = tv_q2(tau[c]);
        double xj[4], colacc[4];
        bool jok[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int col = tile_col(wc, n, ln);
            xj[n] = psoap_smem[XS + (3 + c) * NB + col];
            jok[n] = NB * tj + col < N;
            colacc[n] = 0.0;
        }
        double sa = 0.0, sl = 0.0, st = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            double xi[4], rowacc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                xi[r] = psoap_smem[XS + c * NB + tile_row(wr, m, ln, r)];
                rowacc[r] = 0.0;
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int col = tile_col(wc, n, ln);
                // (the times are read where they are used, as in the gradient's epilogue: kept across the tile they would not
                // fit beside the accumulators)
                const double tcol = psoap_smem[TS + NB + col];
                double d[4], a[4], e[4];
                bool live = false;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma clang fp contract(off)
                    d[r] = xj[n] - xi[r];
                    const double dt = tcol - psoap_smem[TS + tile_row(wr, m, ln, r)];
                    a[r] = p2 * d[r] * d[r];
                    a[r] = a[r] + q2 * dt * dt;
                    live = live || !(a[r] <= -746.0);
                }
                if (__builtin_amdgcn_ballot_w64(live) == 0ull) continue;      // exp() = +0 for the whole wave: nothing to add
                exp_nonpos_batch<4>(a, e);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = tile_row(wr, m, ln, r);
                    const bool ok = jok[n] && NB * ti + row < N && (!diag_tile || row <= col);
                    const double qe = ok ? 0.5 * t.acc[m][n][r] * e[r] : 0.0;
                    const double w = (diag_tile && row == col) ? 1.0 : 2.0;
                    const double qed = qe * d[r];
                    // dt again from LDS, through an index the optimiser cannot match with the one above: four time
                    // differences kept across the exp are registers the kernel does not have
                    int trow = TS + row;
                    asm volatile("" : "+v"(trow));
                    const double dt = tcol - psoap_smem[trow];
                    sa = fma(w, qe, sa);
                    sl = fma(w * qed, d[r], sl);
                    st = fma(w * qe * dt, dt, st);
                    rowacc[r] += qed;
                    colacc[n] -= qed;
                }
            }
            // the row's 16 lanes (lane & 15 = column within the block), then the two wave columns in LDS
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int off = 1; off <= 8; off <<= 1) rowacc[r] += __shfl_xor(rowacc[r], off, 64);
                if ((ln & 15) == 0) psoap_smem[RS + (wc * 3 + c) * NB + tile_row(wr, m, ln, r)] = rowacc[r];
            }
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            colacc[n] += __shfl_xor(colacc[n], 16, 64);
            colacc[n] += __shfl_xor(colacc[n], 32, 64);
            if (ln < 16) psoap_smem[CS + (wr * 3 + c) * NB + tile_col(wc, n, ln)] = colacc[n];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            sa += __shfl_xor(sa, off, 64);
            sl += __shfl_xor(sl, off, 64);
            st += __shfl_xor(st, off, 64);
        }
        if (ln == 0) {
            psoap_smem[HS + wave * WS + L::HYP * c] = sa;
            psoap_smem[HS + wave * WS + L::HYP * c + 1] = sl;
            psoap_smem[HS + wave * WS + L::HYP * c + 2] = st;
        }
    }
    __syncthreads();
    double* out = part + (size_t)blockIdx.x * L::DOUBLES;
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

// F[s][t] = F[t][s] = tan_s . g_t for s >= t.  grid (T, T), 256 threads: k_fisher_dot's c N grid terms and 2c
// hyper-parameter terms in its order, then the c time-scale terms one after the other (g_tau (T, c): k_tv_grad_finish's)
__global__ __launch_bounds__(256) void k_tv_fisher_dot(const double* __restrict__ tan_x, const double* __restrict__ tan_gp,
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
    red[tid] = acc;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        double r = red[0];
        for (int k = 0; k < 2 * C; ++k) r = fma(tan_gp[(size_t)s * 2 * C + k], g_gp[(size_t)t * 2 * C + k], r);
        for (int k = 0; k < C; ++k) r = fma(tan_tau[(size_t)s * C + k], g_tau[(size_t)t * C + k], r);
        F[(size_t)s * T + t] = r;
        F[(size_t)t * T + s] = r;
    }
}

inline hipError_t tv_fisher_configure_kernels()
{
    const void* const kernels[] = {reinterpret_cast<const void*>(k_tv_fisher_contract<1>),
                                   reinterpret_cast<const void*>(k_tv_fisher_contract<2>),
                                   reinterpret_cast<const void*>(k_tv_fisher_contract<3>)};
    for (const void* k : kernels)
        if (hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEMM_LDS_BYTES)) return e;
    return hipSuccess;
}

}  // namespace psoap
