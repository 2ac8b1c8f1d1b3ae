// timevar_kernels.hpp -- time-variable component spectra: a temporal factor in the GP kernel (not in the reference, whose
// paper names it as the next step).
//
//   K_ij = sum_c a_c^2 exp(p_c d_cij^2 + q_c dt_ij^2) + sigma_i^2 delta_ij
//   d_cij = x_c[j] - x_c[i],  p_c = -1/2 c_kms^2 / l_c^2;     dt_ij = t[j] - t[i],  q_c = -1/2 / tau_c^2
// t[i] is the observation time of pixel i (days), tau_c the time scale over which component c's spectrum drifts.
// tau_c = +inf is the static model of fill_kernels.hpp / grad_kernels.hpp.
//
// One exp: the temporal term joins the argument the kernels already form -- a = p2 * d * d, then a = a + q2 * dt * dt, both
// without contraction, in that order -- so the cost is a multiply-add per element and the wave-uniform underflow shortcut
// works on the combined argument.  Bit-identity at tau = inf: q2 = -0.5 / (tau * tau) = -0, the added term (-0 * dt) * dt is
// -0 for every finite dt, and a + (-0) has the bits of a (a = -0 included): k_fill_sym_tv then writes the matrix of
// k_fill_sym, and the value and the gradient below have the bits of grad_kernels.hpp.
//
// With e_cij = exp(p_c d_cij^2 + q_c dt_ij^2), the gradient of grad_kernels.hpp keeps its formulas and gains
//   dlnL/dtau_c = 1/2 a_c^2 / tau_c^3 sum_ij Q_ij e_cij dt_ij^2            (exactly 0 at tau_c = inf)
// The factorisation, alpha and the product W_ti^T W_tj are those of grad_kernels.hpp; only the fill, the epilogue of the
// contraction and the finishing sums are new.  Every sum runs in a fixed order and no kernel uses an atomic.
#pragma once
#include "grad_kernels.hpp"

namespace psoap {

// q_c = -1/2 / tau_c^2 as every kernel here rounds it (tau = inf: -0)
__device__ __forceinline__ double tv_q2(double tau)
{
#pragma clang fp contract(off)
    return -0.5 / (tau * tau);
}

// k_fill_sym (fill_kernels.hpp) with the temporal term: t (N) the pixels' times, tau (B, C).  Everything else -- the
// layout, one exp_nonpos_batch<8> per component and step, the underflow shortcut, the diagonal rule, the identity
// padding, upper_only -- is k_fill_sym's.
template <int C>
__global__ __launch_bounds__(256) void k_fill_sym_tv(double* __restrict__ Kbase, size_t mat_stride, int ld, int N, int P,
                                                     const double* __restrict__ lwl, const double* __restrict__ t,
                                                     const double* __restrict__ gp, const double* __restrict__ tau,
                                                     const double* __restrict__ sigma, int upper_only)
{
    __shared__ double xrow[C][NB];
    __shared__ double trow[NB];
    __shared__ double srow[NB];
    const int b = blockIdx.y;
    int ti, tj;
    if (upper_only) {
        decode_upper(blockIdx.x, P, ti, tj);
    } else {
        ti = blockIdx.x / P;
        tj = blockIdx.x % P;
    }
    const int tid = threadIdx.x;
    const int i0 = ti * NB, j0 = tj * NB;
    const double* lw = lwl + (size_t)b * C * N;
    GpDev g;
    load_gp(gp + (size_t)b * 2 * C, C, g);
    double q2[C];
#pragma unroll
    for (int c = 0; c < C; ++c) q2[c] = tv_q2(tau[(size_t)b * C + c]);
    double dsum = g.a2[0];
    {
#pragma clang fp contract(off)
        for (int c = 1; c < C; ++c) dsum = dsum + g.a2[c];
    }

    if (tid < NB) {
        int i = i0 + tid;
#pragma unroll
        for (int c = 0; c < C; ++c) xrow[c][tid] = (i < N) ? lw[(size_t)c * N + i] : 0.0;
        trow[tid] = (i < N) ? t[i] : 0.0;
        double s = (sigma != nullptr && i < N) ? sigma[i] : 0.0;
        srow[tid] = s * s;
    }
    // (the patch shape of k_fill_sym: wave w owns the 32-column block w, a step covers 16 rows x 32 columns)
    const int w = tid >> 6, rg = (tid >> 4) & 3, cp = tid & 15;
    const int ja = j0 + 32 * w + 2 * cp, jb = ja + 1;
    double xa[C], xb[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        xa[c] = (ja < N) ? lw[(size_t)c * N + ja] : 0.0;
        xb[c] = (jb < N) ? lw[(size_t)c * N + jb] : 0.0;
    }
    const double ta = (ja < N) ? t[ja] : 0.0, tb = (jb < N) ? t[jb] : 0.0;
    __syncthreads();

    double* Km = Kbase + (size_t)b * mat_stride;
#pragma unroll 1
    for (int g4 = 0; g4 < NB / 16; ++g4) {
        double va[4], vb[4];
        double dta[4], dtb[4];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const double tr = trow[16 * g4 + rg + 4 * s4];
            dta[s4] = ta - tr;
            dtb[s4] = tb - tr;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma clang fp contract(off)
            double a[8], e[8];
            bool live = false;
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const double xi = xrow[c][16 * g4 + rg + 4 * s4];
                const double da = xa[c] - xi, db = xb[c] - xi;
                a[2 * s4] = g.p2[c] * da * da;
                a[2 * s4] = a[2 * s4] + q2[c] * dta[s4] * dta[s4];
                a[2 * s4 + 1] = g.p2[c] * db * db;
                a[2 * s4 + 1] = a[2 * s4 + 1] + q2[c] * dtb[s4] * dtb[s4];
                live = live || !(a[2 * s4] <= -746.0) || !(a[2 * s4 + 1] <= -746.0);
            }
            if (__builtin_amdgcn_ballot_w64(live) != 0ull) {
                exp_nonpos_batch<8>(a, e);
#pragma unroll
                for (int k = 0; k < 8; ++k) e[k] = g.a2[c] * e[k];
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) e[k] = 0.0;
            }
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                va[s4] = (c == 0) ? e[2 * s4] : va[s4] + e[2 * s4];
                vb[s4] = (c == 0) ? e[2 * s4 + 1] : vb[s4] + e[2 * s4 + 1];
            }
        }
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int r = 16 * g4 + rg + 4 * s4;
            const int i = i0 + r;
            d2 v;
            if (i < N) {
                double x = (ja < N) ? va[s4] : 0.0;
                double y = (jb < N) ? vb[s4] : 0.0;
                if (ja == i) x = dsum + srow[r];
                if (jb == i) y = dsum + srow[r];
                v.x = x;
                v.y = y;
            } else {
                v.x = (ja == i) ? 1.0 : 0.0;
                v.y = (jb == i) ? 1.0 : 0.0;
            }
            *reinterpret_cast<d2*>(Km + (size_t)i * ld + ja) = v;
        }
    }
}

// doubles per tile in the partial-sum workspace of the time-variable gradient: the row and column sums of
// grad_kernels.hpp, then three hyper-parameter sums per component (sa, sl, st)
constexpr int TV_ROWS_OFF = 0, TV_COLS_OFF = 3 * NB, TV_HYP_OFF = 6 * NB, TV_TILE_DOUBLES = 6 * NB + 9;

// grad_contract_epilogue (grad_kernels.hpp) under the time-variable kernel: e_c = exp(p_c d^2 + q_c dt^2), the tile's row and
// column times beside its abscissae in LDS, and one more sum per component,
//   st = sum w q e_c dt^2
// sa, sl and the row and column sums keep their formulas and their order (the same bits at tau = inf).
template <int C>
__device__ __forceinline__ void tv_contract_epilogue(const Tile& t, int b, int ti, int tj, int tile_index, int N, int Npad,
                                                     int P, const double* __restrict__ lwl, const double* __restrict__ times,
                                                     const double* __restrict__ gp, const double* __restrict__ tau,
                                                     const double* __restrict__ alpha, double* __restrict__ part)
{
    constexpr int XS = 0;                 // [2][3][NB]: abscissae of the tile's rows (side 0) and columns (side 1)
    constexpr int AL = XS + 6 * NB;       // [2][NB]: alpha likewise
    constexpr int TS = AL + 2 * NB;       // [2][NB]: times likewise
    constexpr int RS = TS + 2 * NB;       // [2 wc][3][NB]: row sums of the two wave columns
    constexpr int CS = RS + 6 * NB;       // [2 wr][3][NB]: column sums of the two wave rows
    constexpr int HS = CS + 6 * NB;       // [4 waves][9]
    static_assert((HS + 36) * sizeof(double) <= GEMM_LDS_BYTES, "the epilogue fits the operand buffers");
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
        psoap_smem[TS + side * NB + idx] = (g < N) ? times[g] : 0.0;
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
        const double q2 = tv_q2(tau[(size_t)b * C + c]);
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
        double sa = 0.0, sl = 0.0, st = 0.0;
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
                // (the times are read where they are used: two more values per row and column kept across the tile would
                // not fit beside the accumulators)
                const double tcol = psoap_smem[TS + NB + col];
                double d[4], a[4], e[4];
                bool live = false;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma clang fp contract(off)
                    d[r] = xj[n] - xi[r];
                    const double dt = tcol - psoap_smem[TS + tile_row(wr, m, lane, r)];
                    a[r] = p2 * d[r] * d[r];
                    a[r] = a[r] + q2 * dt * dt;
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
        }
        if (lane == 0) {
            psoap_smem[HS + wave * 9 + 3 * c] = sa;
            psoap_smem[HS + wave * 9 + 3 * c + 1] = sl;
            psoap_smem[HS + wave * 9 + 3 * c + 2] = st;
        }
    }
    __syncthreads();
    double* out = part + ((size_t)b * (P * (P + 1) / 2) + tile_index) * TV_TILE_DOUBLES;
    {
        const int side = tid >> 7, idx = tid & 127;
        const int src = side ? CS : RS;
#pragma unroll
        for (int c = 0; c < C; ++c)
            out[(side ? TV_COLS_OFF : TV_ROWS_OFF) + c * NB + idx] =
                psoap_smem[src + c * NB + idx] + psoap_smem[src + (3 + c) * NB + idx];
    }
    if (tid < 3 * C)
        out[TV_HYP_OFF + tid] = ((psoap_smem[HS + tid] + psoap_smem[HS + 9 + tid]) + psoap_smem[HS + 18 + tid]) +
                                psoap_smem[HS + 27 + tid];
}

// k_grad_contract (grad_kernels.hpp): the same product, the epilogue above.  grid (P (P + 1) / 2, B)
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
    const int b = blockIdx.y;
    int ti, tj;
    decode_upper(blockIdx.x, P, ti, tj);
    const double* W = Abase + (size_t)b * mat_stride + Npad + (size_t)NB * tj * ld;
    Tile t;
    t.zero();
    tile_gemm_tn(t, W + NB * ti, (size_t)ld, W + NB * tj, (size_t)ld, Npad - NB * tj, ti == tj);
    tv_contract_epilogue<C>(t, b, ti, tj, (int)blockIdx.x, N, Npad, P, lwl, times, gp, tau, alpha, part);
}

// k_grad_finish (grad_kernels.hpp) over the records above, in the same tile order.  grid (P + 1, B), 128 threads.
//   blocks x < P:  grad_x[b][c][128 x + i], as k_grad_finish
//   block  x == P: the 3 C hyper-parameter sums and sum_i alpha_i, each as k_grad_finish adds its own:
//                  grad_gp[b][2C], grad_tau[b][c] = 1/2 a_c^2 / tau_c^3 st_c, grad_mu[b]
__global__ __launch_bounds__(128) void k_tv_grad_finish(const double* __restrict__ part, const double* __restrict__ alpha,
                                                        const double* __restrict__ gp, const double* __restrict__ tau, int C,
                                                        int N, int Npad, int P, double* __restrict__ grad_gp,
                                                        double* __restrict__ grad_tau, double* __restrict__ grad_x,
                                                        double* __restrict__ grad_mu)
{
    __shared__ double red[128];
    const int b = blockIdx.y, x = blockIdx.x, tid = threadIdx.x;
    const int ntiles = P * (P + 1) / 2;
    const double* pb = part + (size_t)b * ntiles * TV_TILE_DOUBLES;
    const double* gpb = gp + (size_t)b * 2 * C;
    if (x < P) {
        const int i = NB * x + tid;
        for (int c = 0; c < C; ++c) {
            double s = 0.0;
            for (int ti = 0; ti <= x; ++ti) s += pb[(size_t)upper_index(ti, x, P) * TV_TILE_DOUBLES + TV_COLS_OFF + c * NB + tid];
            for (int tj = x; tj < P; ++tj) s += pb[(size_t)upper_index(x, tj, P) * TV_TILE_DOUBLES + TV_ROWS_OFF + c * NB + tid];
            const double a = gpb[2 * c], l = gpb[2 * c + 1];
            const double p2 = -0.5 * (C_KMS * C_KMS) / (l * l);
            if (i < N) grad_x[((size_t)b * C + c) * N + i] = -2.0 * p2 * (a * a) * s;
        }
        return;
    }
    for (int k = 0; k <= 3 * C; ++k) {
        double s = 0.0;
        if (k < 3 * C) {
            for (int t = tid; t < ntiles; t += 128) s += pb[(size_t)t * TV_TILE_DOUBLES + TV_HYP_OFF + k];
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
            if (k == 3 * C) {
                grad_mu[b] = red[0];
            } else {
                const int c = k / 3, what = k % 3;
                const double a = gpb[2 * c], l = gpb[2 * c + 1];
                if (what == 0) {
                    grad_gp[(size_t)b * 2 * C + 2 * c] = a * red[0];
                } else if (what == 1) {
                    grad_gp[(size_t)b * 2 * C + 2 * c + 1] = 0.5 * (a * a) * (C_KMS * C_KMS) / (l * l * l) * red[0];
                } else {
                    const double tc = tau[(size_t)b * C + c];
                    grad_tau[(size_t)b * C + c] = 0.5 * (a * a) / (tc * tc * tc) * red[0];
                }
            }
        }
    }
}

inline hipError_t tv_configure_kernels()
{
    const int lds = (int)GEMM_LDS_BYTES;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_tv_grad_contract<1>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_tv_grad_contract<2>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_tv_grad_contract<3>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    return e;
}

}  // namespace psoap
