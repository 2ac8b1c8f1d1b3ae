// factor_host.hpp -- what every analysis path stands on.  Part of psoap_gp.hip, included behind predict_host.hpp: it uses that
// file's error macros, the handle, enter_device / set_dev, prof_launch and staged_row; the runs are in analysis_host.hpp, behind
// this file.  Everything lives in the handle's workspaces and runs on the handle's first stream behind whatever the handle has
// in flight: neither the proposal slots nor the workspaces of the likelihood paths are touched.
// What the analysis paths share, and what a new one is expected to reuse ("What the analysis paths share"), in the
// order of this file: tile_units counts tile products; grad_ws_need, launch_grad_fill, launch_alpha and grad_row (the record
// staged_row takes) serve [K | ...] in the gradient workspace; analysis_refused, proposal_refused, tau_refused, values_out and
// poison_gradient are the conventions, release_ws the body of a *_release; orbit_front / orbit_back are the orbit entry; then
// the marginal pieces; Factored says where things are after a factorisation, plain or marginal, factored_ws_need sizes the
// workspaces for it and factor_group runs it.  The time-variable kernel is a flag on the same path, not a path: Factored::tv.
#pragma once

// executed 128^3 products over the upper tiles of K^-1 = W W^T (Kt^-1: Q slots of Vt more): tile column tj has tj + 1 tiles
static double tile_units(int P, int Q)
{
    double units = 0.0;
    for (int tj = 0; tj < P; ++tj) units += (double)(tj + 1) * (P - tj + Q);      // (P - tj + Q products each)
    return units;
}

// The gradient workspace for groups of G matrices of mstride doubles each: what the factorisation needs, always; alpha and
// its partial sums (`alpha`); the contraction's partial tiles and the three gradients (`contract`); with np > 0 the orbit
// entry's buffers for c components and np orbital parameters, and the epoch lists of the fold.  `tv`: the time scales, the
// longer tile record of the time-variable contraction and, with `contract`, dlnL/dtau.  `qp` (with `tv`): Gamma and P, the
// still longer record of the quasi-periodic contraction (QpTile) and dlnL/dGamma, dlnL/dP.
static int grad_ws_need(psoap_chunk* h, GradWs& w, int G, size_t mstride, bool alpha, bool contract, int c = 0, int np = 0,
                        bool tv = false, bool qp = false)
{
    const int N = h->N, Npad = h->Npad, ne = h->n_epochs;
    HIP_TRY(w.A.need((size_t)G * mstride));
    HIP_TRY(w.Wt.need((size_t)G * NB * NB));
    HIP_TRY(w.R.need((size_t)G * Npad));
    HIP_TRY(w.Acc.need((size_t)G * ACC_ROWS));
    HIP_TRY(w.Lwl.need((size_t)G * 3 * N));
    HIP_TRY(w.Gp.need((size_t)G * 6));
    if (alpha) {
        HIP_TRY(w.Alpha.need((size_t)G * Npad));
        HIP_TRY(w.APart.need((size_t)G * ((Npad + 255) / 256) * Npad));
    }
    if (tv) HIP_TRY(w.Tau.need((size_t)G * 3));
    if (qp) {
        HIP_TRY(w.Gamma.need((size_t)G * 3));
        HIP_TRY(w.Period.need((size_t)G * 3));
    }
    if (contract) {
        HIP_TRY(w.Part.need((size_t)G * (h->P * (h->P + 1) / 2) *
                            (qp ? QpTile::DOUBLES : tv ? GradTile<true>::DOUBLES : GradTile<false>::DOUBLES)));
        HIP_TRY(w.GradGp.need((size_t)G * 6));
        HIP_TRY(w.GradX.need((size_t)G * 3 * N));
        HIP_TRY(w.GradMu.need(G));
        if (tv) HIP_TRY(w.GradTau.need((size_t)G * 3));
        if (qp) {
            HIP_TRY(w.GradGamma.need((size_t)G * 3));
            HIP_TRY(w.GradPeriod.need((size_t)G * 3));
        }
    }
    if (np > 0) {
        HIP_TRY(w.Porb.need((size_t)G * np));
        HIP_TRY(w.Vel.need((size_t)G * c * ne));
        HIP_TRY(w.Jac.need((size_t)G * c * ne * np));
        HIP_TRY(w.Gv.need((size_t)G * c * ne));
        HIP_TRY(w.GradOrb.need((size_t)G * np));
        HIP_TRY(w.TooFast.need(G));
    }
    return 0;
}

// K (upper tiles) of the nb matrices whose grids and hyper-parameters are in w.Lwl and w.Gp, into w.A as the caller lays it out
// (`tv`: under the time-variable kernel -- k_fill_sym_tv with the handle's times and w.Tau; `qp` with it: under the
// quasi-periodic one -- k_fill_sym_qp with w.Gamma and w.Period as well)
static void launch_grad_fill(const psoap_chunk* h, GradWs& w, hipStream_t s, int nb, int c, size_t mstride, int ld, bool tv = false,
                             bool qp = false)
{
    with_components(c, [&](auto nc) {
        if (qp) {
            hipLaunchKernelGGL(k_fill_sym_qp<nc()>, dim3(h->P * (h->P + 1) / 2, nb), dim3(256), 0, s, w.A.p, mstride, ld, h->N, h->P,
                               (const double*)w.Lwl.p, (const double*)h->dTimes.p, (const double*)w.Gp.p, (const double*)w.Tau.p,
                               (const double*)w.Gamma.p, (const double*)w.Period.p, (const double*)h->dSigma.p, 1);
            return;
        }
        if (tv) {
            hipLaunchKernelGGL(k_fill_sym_tv<nc()>, dim3(h->P * (h->P + 1) / 2, nb), dim3(256), 0, s, w.A.p, mstride, ld, h->N, h->P,
                               (const double*)w.Lwl.p, (const double*)h->dTimes.p, (const double*)w.Gp.p, (const double*)w.Tau.p,
                               (const double*)h->dSigma.p, 1);
            return;
        }
        hipLaunchKernelGGL(k_fill_sym<nc()>, dim3(h->P * (h->P + 1) / 2, nb), dim3(256), 0, s, w.A.p, mstride, ld, h->N, h->P,
                           (const double*)w.Lwl.p, (const double*)w.Gp.p, (const double*)h->dSigma.p, 1);
    });
}

// w.Alpha = W^T z for nb factored matrices (z: w.R, or what the caller made of it).  Launches only: inside the caller's bracket.
static void launch_alpha(GradWs& w, hipStream_t s, int nb, size_t mstride, int ld, int Npad, int P, const double* z)
{
    const int nslab = (Npad + 255) / 256;
    hipLaunchKernelGGL(k_grad_alpha_partial, dim3(P, nslab, nb), dim3(256), 0, s, (const double*)w.A.p, mstride, ld, Npad, z,
                       w.APart.p, nslab);
    hipLaunchKernelGGL(k_grad_alpha_finish, dim3((Npad + 255) / 256, nb), dim3(256), 0, s, (const double*)w.APart.p, nslab, Npad,
                       w.Alpha.p);
}

// the block-row record of [K | ...] in the gradient workspace, `strip` tiles right of the diagonal tile
static StagedRow grad_row(GradWs& w, size_t mstride, int ld, int Npad, int strip)
{
    return StagedRow{w.A.p, mstride, ld, w.R.p, Npad, w.Acc.p, w.Wt.p, (size_t)NB * NB, strip};
}

// The pair of refusals of an analysis call, in this order: an open stream; with `marg`, what marg_grad_check says of B, c
static int analysis_refused(const psoap_chunk* h, const char* who, bool marg, int B, int c)
{
    if (h->stream.open) FAIL(std::string(who) + ": the handle has an open stream (psoap_stream_close first)");
    if (marg)
        if (const char* why = marg_grad_check(B, c, h->marg.valid, h->marg.stale_weight)) FAIL(std::string(who) + ": " + why);
    return 0;
}

// The conventions of the likelihood (covariance.py:317; sample_parallel.py:186-187): proposal b has a negative hyper-parameter
// or, with `fast` given, an orbit with |v| >= c  ->  lnL = -inf whatever the device computed
static bool proposal_refused(const double* gp, int c, int b, const int* fast = nullptr)
{
    bool neg = fast && fast[b];
    for (int k = 0; k < 2 * c; ++k) neg = neg || gp[(size_t)b * 2 * c + k] < 0.0;
    return neg;
}

// a time scale that is no time scale: tau <= 0 or NaN (+inf is the static model)
static bool tau_refused(const double* tau, int c, int b)
{
    bool bad = false;
    for (int k = 0; k < c; ++k) bad = bad || !(tau[(size_t)b * c + k] > 0.0);
    return bad;
}

// The value record of proposal b (`stride` doubles per proposal: the value and, with stride 5, its four parts) into lnp[b] and,
// where asked for, parts[4 b]: -inf for a refused proposal whatever the device computed, NaN parts beside a -inf.
// -> the proposal has no value, and nothing else is to be said about it
static bool values_out(const double* out, int stride, int b, bool refused, double* lnp, double* parts)
{
    lnp[b] = refused ? -INFINITY : out[(size_t)b * stride];
    const bool bad = lnp[b] == -INFINITY;
    if (parts)
        for (int k = 0; k < 4; ++k) parts[(size_t)b * 4 + k] = bad ? NAN : out[(size_t)b * stride + 1 + k];
    return bad;
}

// NaN into record b of an output of n doubles per record (nullptr: not asked for)
static void fill_nan(double* out, size_t b, size_t n) { if (out) std::fill(out + b * n, out + (b + 1) * n, (double)NAN); }

// ... and no gradient there: NaN into proposal b of grad_gp and of every optional output that was asked for
static void poison_gradient(int b, int c, int N, int ne, int np, double* grad_gp, double* grad_tau, double* grad_lwl,
                            double* grad_mu, double* grad_orb, double* grad_vel)
{
    fill_nan(grad_gp, b, (size_t)2 * c);
    fill_nan(grad_tau, b, c);
    fill_nan(grad_lwl, b, (size_t)c * N);
    fill_nan(grad_mu, b, 1);
    fill_nan(grad_orb, b, np);
    fill_nan(grad_vel, b, (size_t)c * ne);
}

// The body of a *_release: the handle's first stream drained (the workspace may still be read there), then `drop`
template <class F>
static int release_ws(psoap_chunk* h, F&& drop)
{
    if (!h) FAIL("null handle");
    DEVICE_SCOPE(h->device);
    if (set_dev(h)) return 1;
    HIP_TRY(hipStreamSynchronize(h->streams[0]));
    drop();
    return 0;
}

// The pixels of every epoch for k_epoch_fold: a counting sort of the handle's epoch index (stable: ascending pixels within an
// epoch), made once per psoap_chunk_set_grid.
static int grad_epoch_lists(psoap_chunk* h, GradWs& w, hipStream_t s)
{
    if (w.epochs_valid) return 0;
    const int N = h->N, ne = h->n_epochs;
    std::vector<int32_t> ep((size_t)N);
    HIP_TRY(hipMemcpyAsync(ep.data(), h->dEpoch, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<int> start((size_t)ne + 1, 0), pix((size_t)N);
    for (int i = 0; i < N; ++i) start[(size_t)ep[i] + 1]++;
    for (int e = 0; e < ne; ++e) start[(size_t)e + 1] += start[e];
    std::vector<int> at(start.begin(), start.end() - 1);
    for (int i = 0; i < N; ++i) pix[(size_t)at[ep[i]]++] = i;
    HIP_TRY(w.EpStart.need((size_t)ne + 1));
    HIP_TRY(w.EpPix.need((size_t)N));
    HIP_TRY(hipMemcpyAsync(w.EpStart, start.data(), sizeof(int) * ((size_t)ne + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(w.EpPix, pix.data(), sizeof(int) * (size_t)N, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));       // (the vectors leave scope)
    w.epochs_valid = true;
    return 0;
}

// The staged factorisation of [K | I] for the nb matrices whose grids and hyper-parameters are in w.Lwl and w.Gp: afterwards
// the appended block holds W = U^-T, w.R holds z = U^-T (fl - mu_GP) and w.Acc the block records.
static int grad_factor(psoap_chunk* h, GradWs& w, hipStream_t s, int nb, int c, double mu_GP, bool tv = false, bool qp = false)
{
    const int N = h->N, Npad = h->Npad, P = h->P, ld = 2 * h->Npad;
    const size_t mstride = (size_t)Npad * ld;
    if (int rc = prof_launch(h, s, PSOAP_K_FILL, 0.0, (double)nb * 12.0 * N * (N + 1.0), [&] {
            launch_grad_fill(h, w, s, nb, c, mstride, ld, tv, qp);
            hipLaunchKernelGGL(k_grad_init, dim3(P * (P + 1) / 2, nb), dim3(256), 0, s, w.A.p, mstride, ld, Npad, P);
        })) return rc;
    if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
            hipLaunchKernelGGL(k_init_rhs, dim3((Npad + 255) / 256, nb), dim3(256), 0, s, w.R.p, Npad, N, h->dFl, mu_GP, w.Acc.p);
        })) return rc;
    // block row p: tile columns p .. P + p -- the rest of K's row and the appended tiles j <= p
    for (int p = 0; p < P; ++p) {
        const int k0 = p * NB;
        const double units = (double)p * (P - p) + 0.5 * p * (p + 1.0);
        auto update = [&] {
            hipLaunchKernelGGL(k_grad_panel_update, dim3(P + 1, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, w.A.p, mstride, ld, k0, P);
        };
        if (int rc = staged_row(h, s, grad_row(w, mstride, ld, Npad, P), nb, k0, p > 0 ? &update : nullptr, TILE_FLOPS * units * nb))
            return rc;
    }
    return 0;
}

// The orbit entry of a gradient call, front: the group's nb orbits (np parameters each) go up, k_orbit_jacobian makes their
// velocities, Jacobian and |v| >= c flags, k_doppler_shift the grids w.Lwl from the handle's grid and dates.
static int orbit_front(psoap_chunk* h, GradWs& w, hipStream_t s, int nb, int c, int model, int np, const double* p_orb)
{
    const int N = h->N, ne = h->n_epochs;
    HIP_TRY(hipMemcpyAsync(w.Porb, p_orb, sizeof(double) * (size_t)nb * np, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(w.TooFast, 0, sizeof(int) * (size_t)nb, s));
    hipLaunchKernelGGL(k_orbit_jacobian, dim3((ne + 63) / 64, nb), dim3(64), 0, s, model, nb, ne, (const double*)w.Porb.p,
                       (const double*)h->dDates, w.Vel.p, w.Jac.p, w.TooFast.p);
    hipLaunchKernelGGL(k_doppler_shift, dim3((N + 255) / 256, nb * c), dim3(256), 0, s, w.Lwl.p, h->dGrid, h->dEpoch,
                       (const double*)w.Vel.p, N, ne, nb * c);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ... and back: after k_grad_finish the fold and the chain (orbit_grad_kernels.hpp) turn w.GradX into dlnL/dv and dlnL/dp_orb
// on the device; the group's grad_orb, grad_vel (optional) and flags come down.
static int orbit_back(psoap_chunk* h, GradWs& w, hipStream_t s, int nb, int c, int np, double* grad_orb, double* grad_vel, int* fast)
{
    const int N = h->N, ne = h->n_epochs, CE = c * ne;
    hipLaunchKernelGGL(k_epoch_fold, dim3((CE + 3) / 4, nb), dim3(256), 0, s, (const double*)w.GradX.p, (const int*)w.EpStart.p,
                       (const int*)w.EpPix.p, c, N, ne, w.Gv.p);
    hipLaunchKernelGGL(k_orbit_chain, dim3(nb), dim3(256), 0, s, (const double*)w.Gv.p, (const double*)w.Jac.p, CE, np, w.GradOrb.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(grad_orb, w.GradOrb, sizeof(double) * (size_t)nb * np, hipMemcpyDeviceToHost, s));
    if (grad_vel) HIP_TRY(hipMemcpyAsync(grad_vel, w.Gv, sizeof(double) * (size_t)nb * CE, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(fast, w.TooFast, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, s));
    return 0;
}

// The marginal pieces (marg_kernels.hpp).  Ht and the tables of the handle's baseline onto the device (once per
// psoap_chunk_set_baseline or _marg_release)
static int marg_basis(psoap_chunk* h, MargWs& m, hipStream_t s)
{
    if (m.basis_ready) return 0;
    const MargSetup& su = h->marg;
    const MargPlan& pl = su.plan;
    const int N = h->N, Npad = h->Npad, Q = pl.Q, ldh = NB * Q, ne = pl.n_epochs;
    std::vector<int> tab((size_t)3 * Q), ep(su.epoch.begin(), su.epoch.end());
    for (int t = 0; t < Q; ++t) {
        tab[(size_t)marg_tab_first(Q) + t] = pl.first[pl.column[t]];
        tab[(size_t)marg_tab_column(Q) + t] = pl.column[t];
        tab[(size_t)marg_tab_slot(Q) + t] = pl.slot[t];
    }
    HIP_TRY(m.Ht.need((size_t)Npad * ldh));
    HIP_TRY(m.X.need(N));
    HIP_TRY(m.Weight.need(N));
    HIP_TRY(m.Epoch.need(N));
    HIP_TRY(m.EpOff.need(ne));
    HIP_TRY(m.EpScl.need(ne));
    HIP_TRY(m.Sd.need(pl.order + 1));
    HIP_TRY(m.Tab.need(tab.size()));
    HIP_TRY(m.Tiles.need(pl.tiles.size()));
    HIP_TRY(hipMemsetAsync(m.Ht, 0, sizeof(double) * (size_t)Npad * ldh, s));
    HIP_TRY(hipMemcpyAsync(m.X, su.x.data(), sizeof(double) * (size_t)N, hipMemcpyHostToDevice, s));
    if (!su.weight.empty()) HIP_TRY(hipMemcpyAsync(m.Weight, su.weight.data(), sizeof(double) * (size_t)N, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(m.Epoch, ep.data(), sizeof(int) * (size_t)N, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(m.EpOff, pl.off.data(), sizeof(double) * (size_t)ne, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(m.EpScl, pl.scl.data(), sizeof(double) * (size_t)ne, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(m.Sd, su.sd.data(), sizeof(double) * (size_t)(pl.order + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(m.Tab, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(m.Tiles, pl.tiles.data(), sizeof(MargTile) * pl.tiles.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_marg_basis, dim3((N + 255) / 256), dim3(256), 0, s, m.Ht.p, ldh, N, pl.order, Q, (const double*)m.X.p,
                       (const int*)m.Epoch.p, (const double*)m.EpOff.p, (const double*)m.EpScl.p,
                       su.weight.empty() ? (const double*)nullptr : (const double*)m.Weight.p, (const double*)m.Sd.p,
                       (const int*)m.Tab.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));       // (the vectors leave scope)
    m.basis_ready = true;
    return 0;
}

// What marg_run and marg_grad_factor share: their K sweeps differ -- [K | Ht] with no identity to pay for, [K | I | Ht] -- and
// so does where M lives (m.M, mg.Mx); the rest is here.  First the marginal workspace beyond M for groups of G matrices;
// `cov`: the inverse of M and the covariance of beta as well
static int marg_ws_need(psoap_chunk* h, MargWs& m, int G, bool cov)
{
    const MargPlan& pl = h->marg.plan;
    const size_t S = (size_t)NB * pl.Q, q = pl.q, nslab = (h->Npad + 255) / 256;
    HIP_TRY(m.WtM.need((size_t)G * pl.Q * NB * NB));
    HIP_TRY(m.Rhs.need((size_t)G * S));
    HIP_TRY(m.Gam.need((size_t)G * S));
    HIP_TRY(m.RPart.need((size_t)G * nslab * S));
    HIP_TRY(m.AccM.need((size_t)G * ACC_ROWS));
    HIP_TRY(m.Out.need((size_t)G * 5));
    HIP_TRY(m.Beta.need((size_t)G * q));
    HIP_TRY(m.Flc.need((size_t)G * h->N));
    if (cov) {
        HIP_TRY(m.Minv.need((size_t)G * S * S));
        HIP_TRY(m.Cov.need((size_t)G * q * q));
    }
    return 0;
}

// m.Rhs = Wh^T z for nb factored matrices, Ah what the kernels of marg_kernels.hpp take for [K | Ht].  Launches only: inside
// the caller's bracket.
static void launch_marg_rhs(const psoap_chunk* h, MargWs& m, hipStream_t s, int nb, const double* Ah, size_t mstride, int ld,
                            const double* z)
{
    const int Npad = h->Npad, Q = h->marg.plan.Q, nslab = (Npad + 255) / 256;
    hipLaunchKernelGGL(k_marg_rhs_partial, dim3(Q, nslab, nb), dim3(256), 0, s, Ah, mstride, ld, Npad, Q, (const int*)m.Tab.p, z,
                       m.RPart.p, nslab);
    hipLaunchKernelGGL(k_marg_rhs_finish, dim3((NB * Q + 255) / 256, nb), dim3(256), 0, s, (const double*)m.RPart.p, nslab, Npad, Q,
                       (const int*)m.Tab.p, m.Rhs.p);
}

// executed 128^3 products of one Gram matrix M = I + Wh^T Wh: a diagonal tile issues three quarters of its MFMAs
static double gram_units(const MargPlan& pl, int Npad)
{
    double units = 0.0;
    for (const MargTile& t : pl.tiles) units += (t.ti == t.tj ? 0.75 : 1.0) * (Npad - t.k0) / NB;
    return units;
}

// lnL, its parts and g = U_M^-1 y of nb matrices into m.Out and m.Gam from the factored M (m_stride doubles per matrix, ldm
// per row); with want_sol beta and the corrected flux as well.  The only launch site of k_marg_finish; inside the caller's bracket.
static void launch_marg_finish(const psoap_chunk* h, const GradWs& w, MargWs& m, hipStream_t s, int nb, const double* M,
                               size_t m_stride, int ldm, bool want_sol)
{
    const MargPlan& pl = h->marg.plan;
    hipLaunchKernelGGL(k_marg_finish, dim3(nb), dim3(256), 0, s, h->N, h->P, pl.Q, pl.q, pl.order, (const MatAcc*)w.Acc.p,
                       (const MatAcc*)m.AccM.p, M, m_stride, ldm, (const double*)m.WtM.p, (const double*)m.Rhs.p, m.Gam.p,
                       (const double*)m.Sd.p, (const int*)m.Epoch.p, (const int*)m.Tab.p, (const double*)m.Ht.p, NB * pl.Q,
                       (const double*)h->dFl.p, m.Out.p, m.Beta.p, m.Flc.p, want_sol ? 1 : 0);
}

// Where things are once a group of matrices is factored (factor_group) -- [K | I], or under the handle's baseline
// [K | I | Ht] and [M | Xt] (marg_grad_plan.hpp): what grad_run, fisher_run and loo_run read instead of asking which.
struct Factored {
    bool marg;
    bool tv;                     // K under the time-variable kernel (fill_kernels.hpp), plain or marginal: the fill reads w.Tau
    bool qp;                     // ... under the quasi-periodic one (plain only, and tv is set with it): w.Gamma and w.Period too
    int G;                       // matrices per group
    int ld;                      // doubles per row of a matrix in w.A, mstride from one matrix to the next
    size_t mstride;
    const Grow<double>* Out;     // the value record, out_stride doubles per matrix: w.Out, or m.Out with the four parts behind the value
    int out_stride;
    bool parts;
    int Q;                       // slots of Ht, for the flop counts (plain: 0)
    const Grow<double>* Vt;      // [M | Vt] as the marginal kernels take it (mg.Mx): m_stride doubles per matrix, ldm per row, M of
    int ldm, S;                  // side S (plain: null and 0)
    size_t m_stride;
    MargGradPlan gpl;            // the block rows of [K | I | Ht]: marg_grad_factor's
};

// The staged factorisation of [K | I | Ht] (marg_grad_kernels.hpp, marg_grad_plan.hpp) and of [M | Xt] for the nb matrices
// whose grids and hyper-parameters are in w.Lwl and w.Gp.  Afterwards the I block holds Wi = U^-T, the appended block of mg.Mx
// holds Vt = U_M^-T Wh^T Wi, m.Out the value and its parts with the bits of marg_run, mg.Zt = z - Wh g and w.Alpha = alpha_m.
// Under fac.tv K is the time-variable kernel (the fill reads the handle's times and w.Tau); nothing behind the fill knows.
static int marg_grad_factor(psoap_chunk* h, const Factored& fac, hipStream_t s, int nb, int c, double mu_GP)
{
    GradWs& w = *h->gws;
    MargWs& m = *h->mws;
    MargGradWs& mg = *h->mgws;
    const MargPlan& pl = h->marg.plan;
    const MargGradPlan& gpl = fac.gpl;
    const int N = h->N, Npad = h->Npad, P = h->P, Q = pl.Q;
    const int S = fac.S, ld = fac.ld, ldm = fac.ldm, ldh = S, ngram = Q * (Q + 1) / 2, ntiles = P * (P + 1) / 2;
    const size_t mstride = fac.mstride, m_stride = fac.m_stride, wstride = (size_t)Q * NB * NB;
    const int* tab = m.Tab.p;
    double* Ah = w.A.p + Npad;          // what the kernels of marg_kernels.hpp take for [K | Ht]: Ht one block further right
    if (int rc = prof_launch(h, s, PSOAP_K_FILL, 0.0, (double)nb * 12.0 * N * (N + 1.0), [&] {
            launch_grad_fill(h, w, s, nb, c, mstride, ld, fac.tv);
            hipLaunchKernelGGL(k_grad_init, dim3(ntiles, nb), dim3(256), 0, s, w.A.p, mstride, ld, Npad, P);
            hipLaunchKernelGGL(k_marg_load, dim3(Q * P, nb), dim3(256), 0, s, Ah, mstride, ld, Npad, P, (const double*)m.Ht.p, ldh,
                               tab);
        })) return rc;
    if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
            hipLaunchKernelGGL(k_init_rhs, dim3((Npad + 255) / 256, nb), dim3(256), 0, s, w.R.p, Npad, N, h->dFl, mu_GP, w.Acc.p);
        })) return rc;
    // block row p: the rest of K's row with I_0 .. I_p, and the slots of Ht whose first non-zero block row is <= p
    for (int p = 0; p < P; ++p) {
        const int k0 = p * NB;
        const MargGradRow& row = gpl.rows[(size_t)p];
        const double units = (double)p * (P - p) + 0.5 * p * (p + 1.0) + (double)p * row.update_h;
        auto update = [&] {
            hipLaunchKernelGGL(k_marg_grad_panel_update, dim3(row.update_k + row.update_h, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES,
                               s, w.A.p, mstride, ld, k0, P, tab);
        };
        // the slots of Ht are a second strip: its first tile column moved onto tile column 2 P, and no right-hand side
        // (r_rows = 0: every column counts as appended, r is only read)
        StagedRow sr = grad_row(w, mstride, ld, Npad, row.strip_k);
        sr.A2 = w.A.p + (NB * gpl.tile_H - k0 - NB);
        sr.strip2 = row.strip_h;
        if (int rc = staged_row(h, s, sr, nb, k0, row.update_k + row.update_h > 0 ? &update : nullptr, TILE_FLOPS * units * nb))
            return rc;
    }
    if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] { launch_marg_rhs(h, m, s, nb, Ah, mstride, ld, w.R.p); })) return rc;
    double gunits = gram_units(pl, Npad);
    for (int sl = 0; sl < Q; ++sl)
        for (int tj = 0; tj < P; ++tj) gunits += P - std::min(P, std::max(pl.first[(size_t)pl.column[(size_t)sl]], tj));
    if (int rc = prof_launch(h, s, PSOAP_K_GRAD, TILE_FLOPS * gunits * nb, 0.0, [&] {
            hipLaunchKernelGGL(k_marg_gram, dim3(ngram, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, (const double*)Ah, mstride, ld,
                               Npad, (const MargTile*)m.Tiles.p, mg.Mx.p, m_stride, ldm);
            hipLaunchKernelGGL(k_marg_grad_cross, dim3(Q * P, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, (const double*)w.A.p,
                               mstride, ld, Npad, P, Q, tab, mg.Mx.p, m_stride, ldm);
        })) return rc;
    // [M | Xt]: M = U_M^T U_M with bt alongside, and the appended block becomes Vt = U_M^-T Xt
    for (int p = 0; p < Q; ++p) {
        const int k0 = p * NB;
        const StagedRow mrow{mg.Mx.p, m_stride, ldm, m.Rhs.p, S, m.AccM.p, m.WtM.p + (size_t)p * NB * NB, wstride, Q - p - 1 + P};
        auto update = [&] {
            hipLaunchKernelGGL(k_panel_update, dim3(Q - p + P, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, mg.Mx.p, m_stride, ldm, k0);
        };
        if (int rc = staged_row(h, s, mrow, nb, k0, p > 0 ? &update : nullptr, TILE_FLOPS * p * (Q - p + P) * nb)) return rc;
    }
    // lnL and g = U_M^-1 y; z - Wh g; alpha_m
    return prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
        launch_marg_finish(h, w, m, s, nb, mg.Mx.p, m_stride, ldm, true);
        hipLaunchKernelGGL(k_marg_grad_resid, dim3(Npad / 4, nb), dim3(256), 0, s, (const double*)w.A.p, mstride, ld, Npad, Q,
                           tab, (const double*)w.R.p, (const double*)m.Gam.p, mg.Zt.p);
        launch_alpha(w, s, nb, mstride, ld, Npad, P, mg.Zt.p);
    });
}

// `Factored` of a call with B matrices; the workspaces it points into exist afterwards, empty until factored_ws_need
static Factored factored(psoap_chunk* h, bool marg, int B, bool tv = false, bool qp = false)
{
    const int Npad = h->Npad;
    if (!h->gws) h->gws.reset(new GradWs());
    Factored fac{};
    fac.marg = fac.parts = marg;
    fac.tv = tv || qp;
    fac.qp = qp;
    if (!marg) {
        fac.G = grad_group_size(B, Npad);
        fac.ld = 2 * Npad;
        fac.mstride = (size_t)Npad * fac.ld;
        fac.Out = &h->gws->Out;
        fac.out_stride = 1;
        return fac;
    }
    if (!h->mws) h->mws.reset(new MargWs());
    if (!h->mgws) h->mgws.reset(new MargGradWs());
    const MargPlan& pl = h->marg.plan;
    marg_grad_plan(pl, fac.gpl);
    fac.G = marg_grad_group_size(B, Npad, pl.Q);
    fac.ld = fac.gpl.ld;
    fac.mstride = marg_grad_matrix_doubles(Npad, pl.Q);
    fac.Out = &h->mws->Out;
    fac.out_stride = 5;
    fac.Q = pl.Q;
    fac.Vt = &h->mgws->Mx;
    fac.S = NB * pl.Q;
    fac.ldm = fac.S + Npad;
    fac.m_stride = (size_t)fac.S * fac.ldm;
    return fac;
}

// The handle's workspaces sized for groups of fac.G matrices: what the factorisation needs, always; alpha and the plain value
// record (`values`: the marginal factorisation makes both whatever is asked); `contract`, c, np as grad_ws_need.  Under the
// baseline Ht goes onto the device as well.
static int factored_ws_need(psoap_chunk* h, const Factored& fac, hipStream_t s, bool values, bool contract, int c = 0, int np = 0)
{
    GradWs& w = *h->gws;
    if (int rc = grad_ws_need(h, w, fac.G, fac.mstride, values || fac.marg, contract, c, np, fac.tv, fac.qp)) return rc;
    if (!fac.marg) {
        if (values) HIP_TRY(w.Out.need(fac.G));
        return 0;
    }
    HIP_TRY(h->mgws->Mx.need((size_t)fac.G * fac.m_stride));
    HIP_TRY(h->mgws->Zt.need((size_t)fac.G * h->Npad));
    if (int rc = marg_ws_need(h, *h->mws, fac.G, false)) return rc;
    return marg_basis(h, *h->mws, s);
}

// The factorisation of the nb matrices whose grids and hyper-parameters are in w.Lwl and w.Gp.  With `values`, w.Alpha and
// the value record are ready afterwards: marg_grad_factor makes both anyway, the plain side in a bracket of their own, which
// fisher_run does without.  `extra` (nullptr: none) is a launch of the caller's that shares that bracket on the plain side
// and has one to itself under the baseline: the bookkeeping of loo_run.
template <class X = void (*)()>
static int factor_group(psoap_chunk* h, const Factored& fac, hipStream_t s, int nb, int c, double mu_GP, bool values,
                        const X* extra = nullptr)
{
    GradWs& w = *h->gws;
    if (int rc = fac.marg ? marg_grad_factor(h, fac, s, nb, c, mu_GP) : grad_factor(h, w, s, nb, c, mu_GP, fac.tv, fac.qp)) return rc;
    const bool finish = values && !fac.marg;
    if (!finish && !extra) return 0;
    return prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
        if (finish) {
            hipLaunchKernelGGL(k_finalize, dim3((nb + 63) / 64), dim3(64), 0, s, (const MatAcc*)w.Acc.p, w.Out.p, nb,
                               (const int*)nullptr, h->P);
            launch_alpha(w, s, nb, fac.mstride, fac.ld, h->Npad, h->P, w.R.p);
        }
        if (extra) (*extra)();
    });
}
