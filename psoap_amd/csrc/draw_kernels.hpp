// draw_kernels.hpp -- draws from the posterior of the component spectra, on the device.
//
// Reference: scripts/psoap_retrieve_SB2_draw.py, psoap_retrieve_ST3_draw.py and psoap_predict_SB2.py / _ST3.py --draws end in
// np.random.multivariate_normal(mu, Sigma, size=n_draws).  Here, with mu and Sigma resident after a predict call
// (PredictWs::Mu, PredictWs::S),
//     X[d, :] = mu + U^T z_d,     U^T U = Sigma + nugget I,     z_d ~ N(0, I_R)
// i.e. draws from N(mu, Sigma + nugget I): Sigma = A - W^T W on a grid finer than the kernel's length scale is numerically
// rank deficient, and a Cholesky factorisation (unlike NumPy's SVD route) needs the nugget.
//
//   k_draw_copy      S' = Sigma + nugget I into the factor buffer [S' | Z] (draw_plan.hpp); identity on the padded
//                    diagonal, as k_fisher_kinv documents for its padding; Sigma itself stays intact
//   (staged_row)     the factorisation of S' by the kernels of chol_kernels.hpp, strip ending at S's last tile column
//   k_draw_normals   Z from the counter-based generator of draw_rng.hpp, or k_draw_load_z: the caller's z
//   k_draw_trmm      X = Z^T U + mu on the fp64 tile engine (gemm_core.hpp)
// No atomics; every sum in an order fixed by (R, D).
#pragma once
#include "chol_kernels.hpp"
#include "draw_plan.hpp"
#include "draw_rng.hpp"

namespace psoap {

// F[i][j] (i, j < Rpad, leading dimension ld) = S[i][j] + nugget [i == j] inside R, the identity outside
__global__ __launch_bounds__(256) void k_draw_copy(const double* __restrict__ S, size_t lds, int R, int Rpad, double nugget,
                                                   double* __restrict__ F, size_t ld)
{
    const int i = blockIdx.y;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < Rpad; j += gridDim.x * 256) {
        double v = (i == j) ? 1.0 : 0.0;
        if (i < R && j < R) {
            v = S[(size_t)i * lds + j];
            if (i == j) v = v + nugget;
        }
        F[(size_t)i * ld + j] = v;
    }
}

// The normals of draws 0 .. D-1, elements 0 .. n-1; element (d, i) goes to out[i * si + d * sd].  One thread per
// (pair of elements, draw).  npad / Dpad: the extent that is written (zeros beyond n and D) -- n, npad even or the odd last
// element handled by its pair alone.  DRAW_FAST: consecutive threads take consecutive draws (the k-major Z of the factor
// buffer, sd == 1); else consecutive pairs (psoap_draw_normals, si == 1).
template <bool DRAW_FAST>
__global__ __launch_bounds__(256) void k_draw_normals(double* __restrict__ out, size_t si, size_t sd, int n, int npad, int D, int Dpad,
                                                      unsigned long long seed)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t npairs = (size_t)(npad + 1) / 2;
    if (idx >= npairs * (size_t)Dpad) return;
    const size_t pair = DRAW_FAST ? idx / (size_t)Dpad : idx % npairs;
    const int d = (int)(DRAW_FAST ? idx % (size_t)Dpad : idx / npairs);
    const int i0 = (int)(2 * pair);
    double z0 = 0.0, z1 = 0.0;
    if (d < D && i0 < n) {
        const PhiloxBlock b = draw_block(seed, (uint32_t)pair, (uint32_t)d);
        const double r = sqrt(-2.0 * log(draw_u_radius(b)));
        double sn, cs;
        sincospi(2.0 * draw_u_angle(b), &sn, &cs);      // (the argument reduction of an exact 2 u2 is exact)
        z0 = r * cs;
        z1 = r * sn;
    }
    out[(size_t)i0 * si + (size_t)d * sd] = z0;
    if (i0 + 1 < npad) out[(size_t)(i0 + 1) * si + (size_t)d * sd] = (i0 + 1 < n) ? z1 : 0.0;
}

// the caller's z (D, R) into Z[i][d], zeros in the padding
__global__ __launch_bounds__(256) void k_draw_load_z(const double* __restrict__ zin, int R, int Rpad, int D, int Dpad,
                                                     double* __restrict__ Z, size_t ld)
{
    const int i = blockIdx.y;
    for (int d = blockIdx.x * 256 + threadIdx.x; d < Dpad; d += gridDim.x * 256)
        Z[(size_t)i * ld + d] = (i < R && d < D) ? zin[(size_t)d * R + i] : 0.0;
}

// X tile (td, tj) = sum_{k < 128 (tj + 1)} Z[k][128 td + .] U[k][128 tj + .]  + mu[128 tj + .]
// F: the factor buffer, U in its upper tiles and Z from column Rpad on, both k-major as the tile engine takes them.  Block
// rows 0 .. tj-1 of U are whole tiles (tile_gemm_tn); the diagonal tile's lower half is not part of U -- the factorisation
// leaves what the copy put there -- and is masked to zero on its way through the staging registers.  In those eight chunks
// the waves of the left column half have nothing to add from k = 64 on.
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_draw_trmm(const double* __restrict__ F, size_t ld, int Rpad, int Rt, int Dt,
                                                              const double* __restrict__ mu, int R, double* __restrict__ X,
                                                              size_t ldx)
{
    const DrawTile g = draw_tile((int)blockIdx.x, Rt, Dt);
    const double* A = F + Rpad + (size_t)NB * g.td;
    const double* B = F + (size_t)NB * g.tj;
    Tile t;
    t.zero();
    tile_gemm_tn(t, A, ld, B, ld, NB * g.tj);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    {
        const int k0 = NB * g.tj;
        const int col2 = tid & 63, row0 = tid >> 6;
        Staging s;
        auto load_masked = [&](int c) {
            stage_load(s, A, ld, B, ld, k0 + c * KB, tid);
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int kr = c * KB + row0 + 4 * it;      // row and columns inside the diagonal tile
                if (kr > 2 * col2) s.b[it].x = 0.0;
                if (kr > 2 * col2 + 1) s.b[it].y = 0.0;
            }
        };
        load_masked(0);
        stage_store(s, 0, tid);
        __syncthreads();
        constexpr int nchunk = NB / KB;
        for (int c = 0; c < nchunk; ++c) {
            const int cur = c & 1;
            if (c + 1 < nchunk) load_masked(c + 1);
            if (!(wc == 0 && c * KB >= NB / 2)) tile_mma_chunk(t, cur, wr, wc, lane);
            if (c + 1 < nchunk) stage_store(s, cur ^ 1, tid);
            __syncthreads();
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int col = NB * g.tj + tile_col(wc, n, lane);
            const double m0 = col < R ? mu[col] : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                X[(size_t)(NB * g.td + tile_row(wr, m, lane, r)) * ldx + col] = t.acc[m][n][r] + m0;
        }
}

inline hipError_t draw_configure_kernels()
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_draw_trmm), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)GEMM_LDS_BYTES);
}

// what a draw needs beyond the predict workspace (psoap_chunk_predict_release frees both)
struct DrawWs {
    Grow<double> F;          // [S' | Z]
    Grow<double> X;          // Dpad x Rpad
    Grow<double> Zin;        // the caller's z
    Grow<double> Rhs;        // the zero right-hand side the staged kernels carry along
    Grow<double> Wt;         // the inverted diagonal tile of the current block row
    Grow<MatAcc> Acc;        // the block rows' records, then their total
    Grow<MatAcc, true> hAcc;
    DrawPlan plan;
};

}  // namespace psoap
