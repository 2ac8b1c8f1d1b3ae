// qp_plan.hpp -- the pure-host part of the quasi-periodic kernel's entry (psoap_chunk_lnlike_qp_grad; the QP kernels of
// fill_kernels.hpp and grad_kernels.hpp): the refusals of a call and the values of Gamma and P that are no proposal.  No HIP
// call and no HIP header: psoap_gp.hip includes it into the library, and a host compiler builds the same text into a
// stand-alone, sanitized program (tests/host/qp_host_check.cpp).
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
