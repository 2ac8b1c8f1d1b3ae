// predict_plan.hpp -- the pure-host part of the predict family (predict_kernels.hpp, predict_host.hpp): argument
// validation, the shape of [B | Cx^T], the prior means and variances, the abscissa rows of the persistent launch, the layout
// of the pinned staging block and the flop count.  No HIP call and no HIP header: psoap_gp.hip includes it into the library,
// and a host compiler builds the same text into a stand-alone, sanitized program (tests/host/predict_host_check.cpp).
//
// mode 0: components (predict_f_g / predict_f_g_h); 1: sum (predict_f_g_sum / _h_sum); 2: predict_f.
#pragma once
#include <stddef.h>

#include "tile_consts.hpp"

namespace psoap {

struct PredictShape {
    int mode = 0, c = 0, N = 0, M = 0;
    int Npad = 0, P = 0;
    int Rq = 0, Rq_pad = 0;           // columns of W that feed Sigma: c M in mode 0, M otherwise
    int Rx = 0, Rx_pad = 0;           // the extra block holding U^-T V12 for the mean of covariance.py:294
    int Rtot_pad = 0, Mt = 0;         // appended columns, their tile columns
    size_t ld = 0;                    // doubles per row of [B | Cx^T]
    int nslab = 0;                    // slabs of 256 rows of the two-stage column sums
    double offset = 0.0;              // what is taken off fl: 1.0 (:140,:184,:248) or the prior mean (:52,:294)
    bool transposed_mean = false;     // mode 1 with c == 3: covariance.py:294 uses V12.T in the mean
    bool dag_ok = false;              // the shape admits the persistent launch (8-bit tile column indices, no transposed block)
};

// -> nullptr, or why the arguments are refused (arrays: every required pointer is there)
inline const char* predict_check(int mode, int c, int N, int M, bool arrays)
{
    if (mode < 0 || mode > 2 || c < 1 || c > 3 || N <= 0 || M <= 0 || !arrays) return "psoap_predict: bad arguments";
    if (mode == 2 && c != 1) return "psoap_predict: mode 2 (predict_f) needs c == 1";
    return nullptr;
}

// mu0: the first prior mean -> nullptr, or why the shape is refused
inline const char* predict_shape(int mode, int c, int N, int M, double mu0, PredictShape& g)
{
    g = PredictShape();
    g.mode = mode, g.c = c, g.N = N, g.M = M;
    g.transposed_mean = (mode == 1 && c == 3);
    if (g.transposed_mean && M != N)
        return "predict_f_g_h_sum is only defined for len(lwl_predict) == len(lwl) (covariance.py:294)";
    g.Npad = round_up(N, NB);
    g.P = g.Npad / NB;
    g.Rq = (mode == 0) ? c * M : M;
    g.Rq_pad = round_up(g.Rq, NB);
    g.Rx = g.transposed_mean ? N : 0;
    g.Rx_pad = round_up(g.Rx, NB);
    g.Rtot_pad = g.Rq_pad + g.Rx_pad;
    g.Mt = g.Rtot_pad / NB;
    g.ld = (size_t)g.Npad + g.Rtot_pad;
    g.nslab = (g.Npad + 255) / 256;
    g.offset = (mode == 0 || (mode == 1 && c == 2)) ? 1.0 : mu0;
    g.dag_ok = !g.transposed_mean && g.P + g.Mt <= 255;
    return nullptr;
}

// Prior variance of prediction column q: the squared amplitudes of the components that contribute to it (fill_V11_* put
// amp^2 on the diagonal), + the 1e-8 nugget of predict_f_g_sum.  ONE routine for the diagonal of the fused Sigma and for
// psoap_*_predict_var, with FMA contraction off: both round alike (and like the reference's a*a + b*b).
inline double predict_prior_variance(int mode, int c, int M, int q, const double* gp)
{
#pragma clang fp contract(off)
    if (mode == 0) return gp[2 * (q / M)] * gp[2 * (q / M)];
    double a2 = gp[0] * gp[0];
    for (int k = 1; k < c; ++k) a2 = a2 + gp[2 * k] * gp[2 * k];
    if (mode == 1 && c == 2) a2 = a2 + 1e-8;
    return a2;
}

inline void predict_prior_variances(const PredictShape& g, const double* gp, double* out)      // (Rq)
{
    for (int q = 0; q < g.Rq; ++q) out[q] = predict_prior_variance(g.mode, g.c, g.M, q, gp);
}

// prior means of the prediction (added to W^T z)
inline void predict_prior_means(const PredictShape& g, const double* mu_c, double* out)      // (Rq)
{
    for (int q = 0; q < g.Rq; ++q) out[q] = (g.mode == 0) ? mu_c[q / g.M] : mu_c[0];
}

// The persistent launch's rows, (c, Rq_pad) each.  colx: prediction abscissae per component for the appended columns; a
// component that does not contribute to a column block (mode 0: C = vstack(V12_f, V12_g, ..), :136,:246) sits at 1e30.
// rowx: row abscissae of the Sigma tiles, the column ones with the opposite sentinel.  diag (Rq_pad): the prior variances.
inline void predict_abscissae(const PredictShape& g, const double* lwl_pred, double* colx, double* rowx)
{
    for (int cc = 0; cc < g.c; ++cc) {
        double* row = colx + (size_t)cc * g.Rq_pad;
        for (int q = 0; q < g.Rq; ++q) {
            const int blk = (g.mode == 0) ? q / g.M : cc;
            row[q] = (g.mode == 0 && blk != cc) ? 1e30 : lwl_pred[(size_t)cc * g.M + (q % g.M)];
        }
        for (int q = g.Rq; q < g.Rq_pad; ++q) row[q] = 0.0;
        if (rowx)
            for (int q = 0; q < g.Rq_pad; ++q) rowx[(size_t)cc * g.Rq_pad + q] = (row[q] == 1e30) ? -1e30 : row[q];
    }
}

inline void predict_diag(const PredictShape& g, const double* gp, double* diag)
{
    predict_prior_variances(g, gp, diag);
    for (int q = g.Rq; q < g.Rq_pad; ++q) diag[q] = 0.0;
}

// The pinned staging block of a call: the first double of every region.  m0, mu, var, prior and diag hold Rq_pad doubles,
// acc the acc_bytes of the totals of the factorisations' records (n sizeof(MatAcc) -- the plain call: K's; the marginal
// one: K's, then M's -- rounded up to whole doubles: the slot is 8-byte aligned), colx and rowx rows_x rows of Rq_pad (the
// persistent launch's; the marginal call has none of the three).
struct PredictStaging {
    size_t m0 = 0, mu = 0, var = 0, prior = 0, acc = 0, colx = 0, rowx = 0, diag = 0, total = 0;
};

inline PredictStaging predict_staging(int Rq_pad, size_t acc_bytes, int rows_x)
{
    PredictStaging s;
    auto take = [&s](size_t n) { const size_t at = s.total; s.total += n; return at; };
    const size_t r = (size_t)Rq_pad;
    s.m0 = take(r), s.mu = take(r), s.var = take(r), s.prior = take(r);
    s.acc = take((acc_bytes + sizeof(double) - 1) / sizeof(double));
    s.colx = take(rows_x * r), s.rowx = take(rows_x * r), s.diag = take(rows_x ? r : 0);
    return s;
}

// flops of psoap_*_predict_timings on padded sizes n and r (SURVEY 8(d) F_pred): the factorisation, W, the mean, and the
// N R^2 of Sigma (2 N R for the variances alone)
inline double predict_flops(double n, double r, bool sigma, bool var)
{
    return n * n * n / 3.0 + n * n * r + (sigma ? n * r * r : (var ? 2.0 * n * r : 0.0)) + 2.0 * n * r;
}

// ---- predict under the time-variable kernel (psoap_chunk_predict_tv; predict_tv_run) ------------------------------------------
// -> nullptr, or why the call is refused, without a device: the modes built (the transposed mean of the sum of three is not,
// as under the baseline), the handle's state -- times set, no open stream, no baseline --, tau (c; +inf is the static model)
// and t_pred (M).  The caller puts the entry's name in front.
inline const char* predict_tv_check(int mode, int c, int M, bool arrays, bool have_times, bool open_stream, bool have_baseline,
                                    const double* tau, const double* t_pred)
{
    if (mode < 0 || mode > 2 || c < 1 || c > 3 || M < 1 || !arrays || !tau || !t_pred) return "bad arguments";
    if (mode == 2 && c != 1) return "mode 2 (predict_f) needs c == 1";
    if (mode == 1 && c == 3)
        return "mode 1 with three components is not provided (the transposed mean of predict_f_g_h_sum, covariance.py:294)";
    if (mode == 1 && c != 2) return "mode 1 (the sum) needs c == 2";
    if (mode == 0 && c < 2) return "mode 0 (the components) needs c == 2 or 3";
    if (!have_times) return "call psoap_chunk_set_times first";
    if (open_stream) return "the handle has an open stream (psoap_stream_close first)";
    if (have_baseline)
        return "the handle has a baseline (psoap_chunk_set_baseline): the time-variable kernel under the marginalised continuum "
               "is not built yet";
    for (int k = 0; k < c; ++k)
        if (!(tau[k] > 0.0)) return "every tau must be a time scale: positive, +inf for a static component";
    for (int m = 0; m < M; ++m)
        if (!(t_pred[m] - t_pred[m] == 0.0)) return "t_pred must be finite";
    return nullptr;
}

// ---- the analysis paths under the time-variable kernel (psoap_chunk_fisher_tv, psoap_chunk_loo_tv) -----------------------------
// -> nullptr, or why the call is refused, without a device: the handle's state in the order and the words of predict_tv_check
// -- times set, no open stream, no baseline.  A tau that is no time scale is not a refusal here: like a negative
// hyper-parameter it gives NaN (the leave-one-out: -inf), after the call.  The caller puts the entry's name in front.
inline const char* tv_analysis_check(int c, bool arrays, bool have_times, bool open_stream, bool have_baseline)
{
    if (!arrays) return "bad arguments";
    if (c < 1 || c > 3) return "number of components must be 1, 2 or 3";
    if (!have_times) return "call psoap_chunk_set_times first";
    if (open_stream) return "the handle has an open stream (psoap_stream_close first)";
    if (have_baseline)
        return "the handle has a baseline (psoap_chunk_set_baseline): the time-variable kernel under the marginalised continuum "
               "is not built yet";
    return nullptr;
}

// ... and of psoap_chunk_fisher_tv: the number of tangents as well (max_T: FISHER_MAX_T of fisher_kernels.hpp)
inline const char* fisher_tv_check(int c, int T, int max_T, bool arrays, bool have_times, bool open_stream, bool have_baseline)
{
    if (!arrays) return "bad arguments";
    if (c < 1 || c > 3) return "number of components must be 1, 2 or 3";
    if (T < 1 || T > max_T) return "the number of tangents must be between 1 and 32";
    return tv_analysis_check(c, arrays, have_times, open_stream, have_baseline);
}

// the temporal factor adds one multiply-add per filled element and nothing to the sweep: the count is the plain call's
inline double predict_tv_flops(double n, double r, bool sigma, bool var) { return predict_flops(n, r, sigma, var); }

// the time scales of components k0 .. k0 + n - 1 for a region launch (TauHost::v), the rest +inf -- static, like the zero
// amplitudes gp_host leaves there
inline void predict_tv_taus(const double* tau, int k0, int n, double out[3])
{
    for (int k = 0; k < 3; ++k) out[k] = (k < n) ? tau[k0 + k] : __builtin_inf();
}

}  // namespace psoap
