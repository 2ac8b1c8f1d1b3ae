// qp_plan.hpp -- the pure-host part of the quasi-periodic kernel's entries (psoap_chunk_lnlike_qp_grad, psoap_chunk_fisher_qp,
// psoap_chunk_loo_qp; the QP kernels of fill_kernels.hpp, grad_kernels.hpp and fisher_kernels.hpp): the refusals of a call, the
// values of Gamma and P that are no proposal, the sizes of the Fisher workspace's additions.  No HIP call and no HIP header:
// psoap_gp.hip includes it into the library, and a host compiler builds the same text into stand-alone, sanitized programs
// (tests/host/qp_host_check.cpp, tests/host/qp_fisher_host_check.cpp).
#pragma once
#include <math.h>
#include <stddef.h>

namespace psoap {

// What psoap_chunk_lnlike_qp_grad is called with, as far as a refusal can depend on it: no pointer is read.
struct QpCall {
    bool arrays;                                        // h, lwl, gp, tau, gamma, period and lnp are there
    bool grad_gp, grad_tau, grad_gamma, grad_period;    // these outputs are there
    bool grad_rest;                                     // grad_lwl or grad_mu is there
    int B, c;
    bool have_times, open_stream, have_baseline;
};

// -> nullptr, or why the call is refused, in the order and the words of psoap_chunk_lnlike_tv_grad: the arrays; its NULL rules
// with the three temporal gradients in the place of grad_tau (grad_gp == NULL: the value only; with grad_gp all three are
// required); B; c; times set; no open stream; no baseline.  A Gamma, P or tau that is no proposal is not a refusal: like a
// negative hyper-parameter it gives -inf / NaN for that proposal, after the call (qp_refused).  The caller puts the entry's
// name in front.
inline const char* qp_check(const QpCall& a)
{
    if (!a.arrays) return "bad arguments";
    if (!a.grad_gp && (a.grad_tau || a.grad_gamma || a.grad_period || a.grad_rest))
        return "grad_gp == NULL asks for the value only: grad_tau, grad_gamma, grad_period, grad_lwl and grad_mu must be NULL too";
    if (a.grad_gp && !(a.grad_tau && a.grad_gamma && a.grad_period)) return "grad_tau, grad_gamma and grad_period go with grad_gp";
    if (a.B < 1) return "B must be at least 1";
    if (a.c < 1 || a.c > 3) return "number of components must be 1, 2 or 3";
    if (!a.have_times) return "call psoap_chunk_set_times first";
    if (a.open_stream) return "the handle has an open stream (psoap_stream_close first; psoap_chunk_set_times refuses one too)";
    if (a.have_baseline)
        return "the handle has a baseline (psoap_chunk_set_baseline): the quasi-periodic kernel under the marginalised continuum is "
               "not built";
    return nullptr;
}

// ---- the analysis paths under the quasi-periodic kernel (psoap_chunk_fisher_qp, psoap_chunk_loo_qp) ----------------------------
// -> nullptr, or why the call is refused, with the arguments, the order and the words of tv_analysis_check and fisher_tv_check
// (predict_plan.hpp): the arrays (gamma and period among them); c; T within 1 .. max_T (FISHER_MAX_T of fisher_kernels.hpp);
// times set; no open stream; no baseline.  A tau, Gamma or P that is no proposal is not a refusal: NaN (the leave-one-out:
// -inf) after the call.  The caller puts the entry's name in front.
inline const char* loo_qp_check(int c, bool arrays, bool have_times, bool open_stream, bool have_baseline)
{
    if (!arrays) return "bad arguments";
    if (c < 1 || c > 3) return "number of components must be 1, 2 or 3";
    if (!have_times) return "call psoap_chunk_set_times first";
    if (open_stream) return "the handle has an open stream (psoap_stream_close first)";
    if (have_baseline)
        return "the handle has a baseline (psoap_chunk_set_baseline): the quasi-periodic kernel under the marginalised continuum is "
               "not built";
    return nullptr;
}

inline const char* fisher_qp_check(int c, int T, int max_T, bool arrays, bool have_times, bool open_stream, bool have_baseline)
{
    if (!arrays) return "bad arguments";
    if (c < 1 || c > 3) return "number of components must be 1, 2 or 3";
    if (T < 1 || T > max_T) return "the number of tangents must be between 1 and 32";
    return loo_qp_check(c, arrays, have_times, open_stream, have_baseline);
}

// What psoap_chunk_fisher_qp asks of the Fisher workspace beyond the three Npad^2 matrices, in doubles: the tangents and their
// contractions ((T, c N) grid parts, (T, 2c) hyper-parameter parts, (T, c) parts of tau, Gamma and P, each twice) and the
// tiles' records of `tile_doubles` (QpTile::DOUBLES of grad_kernels.hpp) for the P (P + 1) / 2 upper tiles of ONE tangent.
struct FisherQpSizes {
    size_t grid, hyper, temporal, part;
};

inline FisherQpSizes fisher_qp_sizes(int c, int N, int P, int T, int tile_doubles)
{
    return FisherQpSizes{(size_t)T * c * N, (size_t)T * 2 * c, (size_t)T * c, (size_t)P * (P + 1) / 2 * tile_doubles};
}

// Proposal b of gamma, period (B, c) holds a value that is none: Gamma < 0, NaN or inf; P <= 0, NaN or inf, or so small that
// rP = 1 / P, which the kernels multiply dt by, is not finite (P below 2^-1024: 0 * inf would put NaN between the pixels of
// one epoch).  (tau keeps its own rule, tau_refused: tau <= 0 or NaN, +inf being the purely periodic component.  A P that
// passes but is so small that dt * rP overflows for some pair of epochs gives NaN elements there, and the proposal ends as
// -inf through the factorisation.)
inline bool qp_refused(const double* gamma, const double* period, int c, int b)
{
    bool bad = false;
    for (int k = 0; k < c; ++k) {
        const double g = gamma[(size_t)b * c + k], p = period[(size_t)b * c + k];
        bad = bad || !(g >= 0.0 && g < INFINITY) || !(p > 0.0 && p < INFINITY) || !(1.0 / p < INFINITY);
    }
    return bad;
}

}  // namespace psoap
