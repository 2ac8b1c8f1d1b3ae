// orbit_grad_kernels.hpp -- the orbit Jacobian and the chain rule from dlnL/dlwl to dlnL/dp_orb (not in the reference).
//
// The rest-frame grids are lwl[i] - v[c, epoch[i]] / c_kms (k_doppler_shift), so with GradX = dlnL/dlwl (k_grad_finish):
//   g_v[b, c, e]   = -(1 / c_kms) sum over the pixels i of epoch e of GradX[b, c, i]        k_epoch_fold
//   grad_orb[b, k] = sum_c sum_e g_v[b, c, e] jac[b, c, e, k]                               k_orbit_chain
//   jac[b, c, e, k] = dv[c, e] / dp_orb[k], k in utils.registered_params order up to gamma  k_orbit_jacobian
//
// The Jacobian is taken at the converged E of orbit_velocities_at (no second iteration) by implicit differentiation of
// Kepler's equation E - e sin E = M.  With w = omega_deg pi/180 and D = 1 - e cos E:
//   df/dM = sqrt(1 - e^2) / D^2            df/de = sin f (2 + e cos f) / (1 - e^2)
//   dM/dT0 = -2 pi / P                     dM/dP = -2 pi (t - T0) / P^2     (the UNREDUCED t - T0: the whole periods that
//                                          fmod drops are piecewise constant in P)
// and per velocity term K (cos(w + f) + e cos w):
//   d/dK = cos(w + f) + e cos w            d/de = -K sin(w + f) df/de + K cos w
//   d/domega_deg = -K (sin(w + f) + e sin w) pi/180
//   d/dP = -K sin(w + f) df/dM dM/dP       d/dT0 = -K sin(w + f) df/dM dM/dT0         d/dgamma = 1
// A K/q component (omega + 180) has d/dq = -term/q and 1/q in d/dK.  The th + 2 pi branch of true_anomaly is a constant.
// Entries of parameters a component does not depend on are exact zeros.
//
// No kernel here uses an atomic for a sum: the fold adds an epoch's pixels in ascending pixel order per lane (stride 64)
// and meets in a wave-64 butterfly; the chain adds per thread in ascending (c, e) order (stride 256), then the butterfly,
// then the four waves in LDS in wave order.  The order depends on the chunk alone, never on the batch around a proposal.
#pragma once
#include "orbit_kernels.hpp"

namespace psoap {

constexpr int ORB_MAX_PARAMS = 13;

// what the Jacobian needs of one orbit at one date
struct OrbitPartials {
    double sf, cf;      // sin f, cos f
    double f;
    double df_dM, df_de, dM_dP, dM_dT0;
};

__device__ inline OrbitPartials orbit_partials(double t, double T0, double P, double e, double f, double E)
{
    const double two_pi = 6.283185307179586476925286766559;
    OrbitPartials o;
    o.f = f;
    o.sf = sin(f);
    o.cf = cos(f);
    const double D = 1.0 - e * cos(E);
    const double one_e2 = (1.0 - e) * (1.0 + e);
    o.df_dM = sqrt(one_e2) / (D * D);
    o.df_de = o.sf * (2.0 + e * o.cf) / one_e2;
    o.dM_dT0 = -two_pi / P;
    o.dM_dP = -two_pi * (t - T0) / (P * P);
    return o;
}

// derivatives of K (cos(w + f) + e cos w) with respect to (K, e, omega_deg, P, T0) of its orbit
__device__ inline void rv_term_grad(double K, double e, double omega_deg, const OrbitPartials& o, double (&g)[5])
{
    const double deg = 3.14159265358979323846 / 180.0;
    const double w = omega_deg * 3.14159265358979323846 / 180.0;
    const double swf = sin(w + o.f), cwf = cos(w + o.f), sw = sin(w), cw = cos(w);
    g[0] = cwf + e * cw;
    g[1] = -K * swf * o.df_de + K * cw;
    g[2] = -K * (swf + e * sw) * deg;
    const double kf = -K * swf * o.df_dM;
    g[3] = kf * o.dM_dP;
    g[4] = kf * o.dM_dT0;
}

// One thread per (proposal, epoch), as k_orbit_velocities: the same velocities (orbit_velocities_at) and flag rule, plus
// jac (B, c, n_epochs, n_orb).
__global__ void k_orbit_jacobian(int model, int B, int n_epochs, const double* __restrict__ p_orb,
                                 const double* __restrict__ dates, double* __restrict__ vel, double* __restrict__ jac,
                                 int* __restrict__ too_fast)
{
    const int ep = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (ep >= n_epochs || b >= B) return;
    const int np = orbit_n_params(model), c = orbit_n_components(model);
    const double* p = p_orb + (size_t)b * np;
    const double t = dates[ep];
    double v[3], fE[4];
    orbit_velocities_at(model, p, t, v, fE);
    bool fast = false;
    for (int k = 0; k < c; ++k) {
        vel[((size_t)b * c + k) * n_epochs + ep] = v[k];
        fast = fast || (fabs(v[k]) >= C_KMS);
    }
    if (fast && too_fast) atomicOr(&too_fast[b], 1);      // (a flag, not a sum: every writer sets the same bit)

    double row[3][ORB_MAX_PARAMS];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < ORB_MAX_PARAMS; ++j) row[k][j] = 0.0;
    double g[5];
    if (model == ORB_SB1 || model == ORB_SB2) {
        const int o = (model == ORB_SB2) ? 1 : 0;          // offset of K
        const double K = p[o], e = p[o + 1], om = p[o + 2], P = p[o + 3], T0 = p[o + 4];
        const OrbitPartials op = orbit_partials(t, T0, P, e, fE[0], fE[1]);
        rv_term_grad(K, e, om, op, g);
#pragma unroll
        for (int j = 0; j < 5; ++j) row[0][o + j] = g[j];
        row[0][o + 5] = 1.0;
        if (model == ORB_SB2) {
            const double q = p[0], Kq = K / q;
            rv_term_grad(Kq, e, om + 180.0, op, g);
            row[1][1] = g[0] / q;
            row[1][0] = -row[1][1] * Kq;
#pragma unroll
            for (int j = 1; j < 5; ++j) row[1][1 + j] = g[j];
            row[1][6] = 1.0;
        }
    } else {
        const int o = (model == ORB_ST1) ? 0 : 1;          // offset of K_in
        const int oo = o + 5 + (model == ORB_ST3 ? 1 : 0);  // offset of K_out
        const double K_in = p[o], e_in = p[o + 1], w_in = p[o + 2], P_in = p[o + 3], T0_in = p[o + 4];
        const double K_out = p[oo], e_out = p[oo + 1], w_out = p[oo + 2], P_out = p[oo + 3], T0_out = p[oo + 4];
        const OrbitPartials in = orbit_partials(t, T0_in, P_in, e_in, fE[0], fE[1]);
        const OrbitPartials out = orbit_partials(t, T0_out, P_out, e_out, fE[2], fE[3]);
        double go[5];
        rv_term_grad(K_out, e_out, w_out, out, go);         // v3: in the primary and the secondary
        rv_term_grad(K_in, e_in, w_in, in, g);
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            row[0][o + j] = g[j];
            row[0][oo + j] = go[j];
        }
        row[0][oo + 5] = 1.0;
        if (c >= 2) {
            const double q = p[0], Kq = K_in / q;
            rv_term_grad(Kq, e_in, w_in + 180.0, in, g);
            row[1][o] = g[0] / q;
            row[1][0] = -row[1][o] * Kq;
#pragma unroll
            for (int j = 1; j < 5; ++j) row[1][o + j] = g[j];
#pragma unroll
            for (int j = 0; j < 5; ++j) row[1][oo + j] = go[j];
            row[1][oo + 5] = 1.0;
        }
        if (c == 3) {
            const double q = p[o + 5], Kq = K_out / q;
            rv_term_grad(Kq, e_out, w_out + 180.0, out, g);
            row[2][oo] = g[0] / q;
            row[2][o + 5] = -row[2][oo] * Kq;
#pragma unroll
            for (int j = 1; j < 5; ++j) row[2][oo + j] = g[j];
            row[2][oo + 5] = 1.0;
        }
    }
    for (int k = 0; k < c; ++k) {
        double* dst = jac + (((size_t)b * c + k) * n_epochs + ep) * np;
        for (int j = 0; j < np; ++j) dst[j] = row[k][j];
    }
}

// The pixels of every epoch, for the fold: ep_start (n_epochs + 1) and ep_pix (N), the pixels of epoch e in ascending
// order at ep_pix[ep_start[e] .. ep_start[e + 1]) -- a counting sort of the handle's epoch index, made on the host.
// One wave per (proposal, component, epoch): grid (ceil(c n_epochs / 4), B), 256 threads.  An epoch with no pixel gives 0.0.
__global__ __launch_bounds__(256) void k_epoch_fold(const double* __restrict__ grad_x, const int* __restrict__ ep_start,
                                                    const int* __restrict__ ep_pix, int C, int N, int n_epochs,
                                                    double* __restrict__ g_v)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ce = blockIdx.x * 4 + wave, b = blockIdx.y;
    if (ce >= C * n_epochs) return;                        // (whole waves leave: the shuffles below stay full)
    const int c = ce / n_epochs, e = ce - c * n_epochs;
    const int j0 = ep_start[e], j1 = ep_start[e + 1];
    const double* gx = grad_x + ((size_t)b * C + c) * N;
    double s = 0.0;
    for (int j = j0 + lane; j < j1; j += 64) s += gx[ep_pix[j]];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) g_v[(size_t)b * C * n_epochs + ce] = (j1 > j0) ? -s / C_KMS : 0.0;
}

// grad_orb[b, k] = sum over (c, e) of g_v[b, c, e] jac[b, c, e, k].  grid (B), 256 threads.
__global__ __launch_bounds__(256) void k_orbit_chain(const double* __restrict__ g_v, const double* __restrict__ jac, int CE,
                                                     int np, double* __restrict__ grad_orb)
{
    __shared__ double red[4][ORB_MAX_PARAMS];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* gv = g_v + (size_t)b * CE;
    const double* J = jac + (size_t)b * CE * np;
    double acc[ORB_MAX_PARAMS];
#pragma unroll
    for (int k = 0; k < ORB_MAX_PARAMS; ++k) acc[k] = 0.0;
    for (int i = tid; i < CE; i += 256) {
        const double g = gv[i];
        const double* Ji = J + (size_t)i * np;
#pragma unroll
        for (int k = 0; k < ORB_MAX_PARAMS; ++k)
            if (k < np) acc[k] = fma(g, Ji[k], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < ORB_MAX_PARAMS; ++k) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
        if (lane == 0) red[wave][k] = acc[k];
    }
    __syncthreads();
    if (tid < np) grad_orb[(size_t)b * np + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

}  // namespace psoap
