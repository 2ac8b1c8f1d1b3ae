// mix_kernels.hpp -- the component spectra marginalised over the chain: mixture moments on the device.
//
// Not a function of the reference: its retrieve scripts reconstruct at ONE parameter vector.  Over chain samples s = 1 .. S
// with weights w_s, W = sum_s w_s, and the conditional (mu_s, Sigma_s) of each sample left in the predict workspace by a
// predict call (PredictWs::Mu, PredictWs::S, PredictWs::Var), the law of total covariance:
//     mu_mix    = sum_s w_s mu_s / W
//     Sigma_mix = sum_s w_s Sigma_s / W  +  sum_s w_s (mu_s - mu_mix)(mu_s - mu_mix)^T / W
//                 `------ within ------'    `------------------ between ----------------'
//
//   k_mix_fold       Sbar += w_s Sigma_s, every element of the R x R block once (the upper tiles and their mirrors alike),
//                    mu_s into row s of Mu, w_s into the weights; k_mix_fold_var: Vbar += w_s var_s in Sbar's place
//   k_mix_mean       W and mu_mix, both sums in ascending s, one lane per column
//   k_mix_center     D[s][i] = sqrt(w_s / W) (Mu[s][i] - mu_mix[i]); Mu itself stays for the next finish
//   k_mix_syrk       one workgroup per upper tile: one K loop over D on the fp64 tile engine (gemm_core.hpp), Sbar / W added,
//                    the tile and its mirror image written; var_within and var_between from the diagonal tiles
//   k_mix_var        the variance-only finish: var_between[i] = sum_s D[s][i]^2 in ascending s, var_within = Vbar / W
// No atomics, no FMA contraction where a weight multiplies (w = 1 adds exactly); every sum in an order fixed by
// (R, S, the order of the adds).  Rows >= S and columns >= R of Mu and D, and Sbar outside R x R, are exact zeros.
#pragma once
#include "gemm_core.hpp"
#include "mix_plan.hpp"

namespace psoap {

// grid (ceil(Rpad / 512), R): row i = blockIdx.y of Sbar (leading dimension Rpad) takes w S[i][.] (leading dimension lds),
// two columns per lane.  Row 0's workgroups also store mu into row s of Mu (zeros from column R on) and w into wv[s].
__global__ __launch_bounds__(256) void k_mix_fold(const double* __restrict__ S, size_t lds, const double* __restrict__ mu, int R,
                                                  int Rpad, double w, int s, double* __restrict__ Sbar, double* __restrict__ Mu,
                                                  double* __restrict__ wv)
{
#pragma clang fp contract(off)
    const int i = blockIdx.y;
    const int j = 2 * (blockIdx.x * 256 + threadIdx.x);
    if (j >= Rpad) return;
    if (j < R) {
        const d2 a = *reinterpret_cast<const d2*>(S + (size_t)i * lds + j);
        d2* out = reinterpret_cast<d2*>(Sbar + (size_t)i * Rpad + j);
        d2 b = *out;
        b.x = b.x + w * a.x;
        if (j + 1 < R) b.y = b.y + w * a.y;
        *out = b;
    }
    if (i == 0) {
        d2 m;
        m.x = j < R ? mu[j] : 0.0;
        m.y = j + 1 < R ? mu[j + 1] : 0.0;
        *reinterpret_cast<d2*>(Mu + (size_t)s * Rpad + j) = m;
        if (j == 0) wv[s] = w;
    }
}

// grid ceil(Rpad / 256): Vbar[j] += w var[j] inside R; mu into row s of Mu, w into wv[s]
__global__ __launch_bounds__(256) void k_mix_fold_var(const double* __restrict__ var, const double* __restrict__ mu, int R, int Rpad,
                                                      double w, int s, double* __restrict__ Vbar, double* __restrict__ Mu,
                                                      double* __restrict__ wv)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Rpad) return;
    if (j < R) Vbar[j] = Vbar[j] + w * var[j];
    Mu[(size_t)s * Rpad + j] = j < R ? mu[j] : 0.0;
    if (j == 0) wv[s] = w;
}

// grid ceil(Rpad / 256): W = sum_s w_s, mu_mix[i] = (sum_s w_s Mu[s][i]) / W over the n folded samples, ascending s
__global__ __launch_bounds__(256) void k_mix_mean(const double* __restrict__ Mu, const double* __restrict__ wv, int n, int Rpad,
                                                  double* __restrict__ mu_mix, double* __restrict__ Wout)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Rpad) return;
    double W = 0.0, m = 0.0;
    for (int s = 0; s < n; ++s) {
        const double w = wv[s];
        W = W + w;
        m = m + w * Mu[(size_t)s * Rpad + i];
    }
    mu_mix[i] = m / W;
    if (i == 0) Wout[0] = W;
}

// grid (ceil(Rpad / 256), depth): D[s][i] = sqrt(w_s / W) (Mu[s][i] - mu_mix[i]) for s < n, exact zeros in rows n .. depth - 1
__global__ __launch_bounds__(256) void k_mix_center(const double* __restrict__ Mu, const double* __restrict__ wv,
                                                    const double* __restrict__ Wp, const double* __restrict__ mu_mix, int n,
                                                    int Rpad, double* __restrict__ D)
{
#pragma clang fp contract(off)
    const int s = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Rpad) return;
    double v = 0.0;
    if (s < n) v = sqrt(wv[s] / Wp[0]) * (Mu[(size_t)s * Rpad + i] - mu_mix[i]);
    D[(size_t)s * Rpad + i] = v;
}

// Upper tile blockIdx.x (mix_tile) of Sigma_mix = Sbar / W + D^T D: one K loop of `depth` rows of D, then the tile and its
// transpose into Out -- Sigma_mix comes out symmetric bit for bit, as k_marg_predict_sigma's Sigma.  The diagonal tiles
// hand out var_within[i] = Sbar[i][i] / W and var_between[i] = (D^T D)[i][i].  Sbar, D and Out have leading dimension ld.
__global__ __launch_bounds__(GEMM_THREADS, 2) void k_mix_syrk(const double* __restrict__ D, size_t ld, int depth,
                                                             const double* __restrict__ Sbar, const double* __restrict__ Wp,
                                                             double* __restrict__ Out, int Rt, double* __restrict__ var_within,
                                                             double* __restrict__ var_between)
{
    const MixTile g = mix_tile((int)blockIdx.x, Rt);
    const int ti = g.ti, tj = g.tj;
    Tile t;
    t.zero();
    tile_gemm_tn(t, D + (size_t)NB * ti, ld, D + (size_t)NB * tj, ld, depth);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const double W = Wp[0];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const size_t at = (size_t)(NB * ti + tile_row(wr, m, lane, 0)) * ld + NB * tj + tile_col(wc, 0, lane);
        double c[4][4];
        tile_load16(Sbar + at, (size_t)4 * ld, c);
        double* p0 = Out + at;
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = tile_row(wr, m, lane, r), col = tile_col(wc, n, lane);
                const double within = c[n][r] / W;
                const double v = within + t.acc[m][n][r];
                p0[(size_t)4 * r * ld + 16 * n] = v;
                if (ti != tj) {
                    Out[(size_t)(NB * tj + col) * ld + NB * ti + row] = v;
                } else if (row == col) {
                    var_within[NB * ti + row] = within;
                    var_between[NB * ti + row] = t.acc[m][n][r];
                }
            }
    }
}

// grid ceil(Rpad / 256): the variance-only finish
__global__ __launch_bounds__(256) void k_mix_var(const double* __restrict__ D, int n, int Rpad, const double* __restrict__ Vbar,
                                                 const double* __restrict__ Wp, double* __restrict__ var_within,
                                                 double* __restrict__ var_between)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Rpad) return;
    double b = 0.0;
    for (int s = 0; s < n; ++s) {
        const double d = D[(size_t)s * Rpad + i];
        b = b + d * d;
    }
    var_within[i] = Vbar[i] / Wp[0];
    var_between[i] = b;
}

inline hipError_t mix_configure_kernels()
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_mix_syrk), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)GEMM_LDS_BYTES);
}

// The mixture of a handle: its device buffers (their own owner, beside the predict workspace: growing or releasing that one
// does not touch them) and what psoap_chunk_mix_begin fixed.  psoap_chunk_mix_release frees it.
struct MixWs {
    Grow<double> Sbar;       // Rpad x Rpad, or Vbar (Rpad) in the variance-only mode
    Grow<double> Out;        // Sigma_mix, Rpad x Rpad (full Sigma only)
    Grow<double> Mu, D;      // Spad x Rpad each
    Grow<double> Small;      // wv (Spad) | mu_mix (Rpad) | var_within (Rpad) | var_between (Rpad) | W (1)
    Grow<double, true> hSmall;      // pinned: mu_mix | var_within | var_between | W
    MixPlan plan;
    bool active = false;
    int marg = 0, mode = 0, c = 0, M = 0, n_folded = 0;
    std::vector<double> lwl_pred, mu_c, mu_host, var_host;
    double* wv() const { return Small.p; }
    double* mu_mix() const { return Small.p + plan.Spad; }
    double* var_within() const { return Small.p + plan.Spad + plan.Rpad; }
    double* var_between() const { return Small.p + plan.Spad + 2 * (size_t)plan.Rpad; }
    double* W() const { return Small.p + plan.Spad + 3 * (size_t)plan.Rpad; }
};

}  // namespace psoap
