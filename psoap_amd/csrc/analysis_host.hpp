// analysis_host.hpp -- the runs of the analysis paths.  Part of psoap_gp.hip, included behind factor_host.hpp, on whose steps
// every run stands; the entries of the C ABI stay in psoap_gp.hip, each its argument checks and one call of a run.  A run is
// straight-line code: workspaces, uploads, the factorisation, its own brackets, downloads, one synchronisation, the conventions.
#pragma once

// The gradient of the likelihood (grad_kernels.hpp).  Group after group of matrices through factor_group, then the contraction
// and the finishing sums -- plain, or with `marg` under the handle's baseline (marg_grad_kernels.hpp).  The ln-wavelengths come
// from the host (lwl) or, with lwl == nullptr, from the orbits p_orb of `model` (orbit_front, orbit_back).  With `tau` (B, c)
// K is the time-variable kernel over the handle's times: the TV fill, contraction and finishing sums, and grad_tau beside
// grad_gp -- plain, or with `marg` on Kt = K_tv + Ht Ht^T (k_marg_tv_grad_contract).  `contract` false is the value only: no
// contraction, no finishing sums, no gradient touched.  With `qp` (plain, host grids, with `tau`) K is the quasi-periodic
// kernel: Gamma and P (B, c) go up beside tau, the QP fill, contraction and finishing sums run, and grad_gamma and grad_period
// come down beside grad_tau.
struct QpArgs {
    const double *gamma, *period;
    double *grad_gamma, *grad_period;
};

// ... and of fisher_run: Gamma and P (c), and the tangents' parts in them (T, c; nullptr: zeros)
struct QpFisherArgs {
    const double *gamma, *period;
    const double *tan_gamma, *tan_period;
};

static int grad_run(psoap_chunk* h, bool marg, int B, int c, const double* lwl, int model, const double* p_orb,
                    const double* gp, const double* tau, double mu_GP, double* lnp, double* parts, double* grad_gp,
                    double* grad_tau, double* grad_lwl, double* grad_mu, double* grad_orb, double* grad_vel, bool contract,
                    const QpArgs* qp = nullptr)
{
    const bool orbits = lwl == nullptr, tv = tau != nullptr;
    DEVICE_SCOPE(h->device);
    if (int rc = enter_device(h->device)) return rc;
    const Factored fac = factored(h, marg, B, tv, qp != nullptr);
    const int N = h->N, Npad = h->Npad, P = h->P, G = fac.G, ld = fac.ld, ntiles = P * (P + 1) / 2;
    const size_t mstride = fac.mstride;
    const int ne = h->n_epochs, np = orbits ? orbit_n_params(model) : 0;
    hipStream_t s = h->streams[0];
    if (int rc = factored_ws_need(h, fac, s, true, contract, c, np)) return rc;
    GradWs& w = *h->gws;
    std::vector<int> fast(orbits ? (size_t)B : 0, 0);
    if (orbits && grad_epoch_lists(h, w, s)) return 1;
    h->recs.clear();
    std::vector<double> out((size_t)B * fac.out_stride);
    for (int b0 = 0; b0 < B; b0 += G) {
        const int nb = (B - b0 < G) ? B - b0 : G;
        if (!orbits)
            HIP_TRY(hipMemcpyAsync(w.Lwl, lwl + (size_t)b0 * c * N, sizeof(double) * (size_t)nb * c * N, hipMemcpyHostToDevice, s));
        else if (int rc = orbit_front(h, w, s, nb, c, model, np, p_orb + (size_t)b0 * np)) return rc;
        HIP_TRY(hipMemcpyAsync(w.Gp, gp + (size_t)b0 * 2 * c, sizeof(double) * (size_t)nb * 2 * c, hipMemcpyHostToDevice, s));
        if (tv) HIP_TRY(hipMemcpyAsync(w.Tau, tau + (size_t)b0 * c, sizeof(double) * (size_t)nb * c, hipMemcpyHostToDevice, s));
        if (qp) {
            HIP_TRY(hipMemcpyAsync(w.Gamma, qp->gamma + (size_t)b0 * c, sizeof(double) * (size_t)nb * c, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(w.Period, qp->period + (size_t)b0 * c, sizeof(double) * (size_t)nb * c, hipMemcpyHostToDevice, s));
        }
        if (int rc = factor_group(h, fac, s, nb, c, mu_GP, true)) return rc;
        if (contract) {
            if (int rc = prof_launch(h, s, PSOAP_K_GRAD, TILE_FLOPS * tile_units(P, fac.Q) * nb, 0.0, [&] {
                    with_components(c, [&](auto nc) {
                        if (qp)
                            hipLaunchKernelGGL(k_qp_grad_contract<nc()>, dim3(ntiles, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s,
                                               (const double*)w.A.p, mstride, ld, N, Npad, P, (const double*)w.Lwl.p,
                                               (const double*)h->dTimes.p, (const double*)w.Gp.p, (const double*)w.Tau.p,
                                               (const double*)w.Gamma.p, (const double*)w.Period.p, (const double*)w.Alpha.p,
                                               w.Part.p);
                        else if (marg && tv)
                            hipLaunchKernelGGL(k_marg_tv_grad_contract<nc()>, dim3(ntiles, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES,
                                               s, (const double*)w.A.p, mstride, ld, N, Npad, P, (const double*)w.Lwl.p,
                                               (const double*)h->dTimes.p, (const double*)w.Gp.p, (const double*)w.Tau.p,
                                               (const double*)w.Alpha.p, w.Part.p, (const double*)fac.Vt->p, fac.m_stride, fac.ldm,
                                               fac.S);
                        else if (marg)
                            hipLaunchKernelGGL(k_marg_grad_contract<nc()>, dim3(ntiles, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s,
                                               (const double*)w.A.p, mstride, ld, N, Npad, P, (const double*)w.Lwl.p,
                                               (const double*)w.Gp.p, (const double*)w.Alpha.p, w.Part.p, (const double*)fac.Vt->p,
                                               fac.m_stride, fac.ldm, fac.S);
                        else if (tv)
                            hipLaunchKernelGGL(k_tv_grad_contract<nc()>, dim3(ntiles, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s,
                                               (const double*)w.A.p, mstride, ld, N, Npad, P, (const double*)w.Lwl.p,
                                               (const double*)h->dTimes.p, (const double*)w.Gp.p, (const double*)w.Tau.p,
                                               (const double*)w.Alpha.p, w.Part.p);
                        else
                            hipLaunchKernelGGL(k_grad_contract<nc()>, dim3(ntiles, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s,
                                               (const double*)w.A.p, mstride, ld, N, Npad, P, (const double*)w.Lwl.p,
                                               (const double*)w.Gp.p, (const double*)w.Alpha.p, w.Part.p);
                    });
                })) return rc;
            if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
                    if (qp)
                        hipLaunchKernelGGL(k_qp_grad_finish, dim3(P + 1, nb), dim3(128), 0, s, (const double*)w.Part.p,
                                           (const double*)w.Alpha.p, (const double*)w.Gp.p, (const double*)w.Tau.p,
                                           (const double*)w.Gamma.p, (const double*)w.Period.p, c, N, Npad, P, w.GradGp.p,
                                           w.GradTau.p, w.GradGamma.p, w.GradPeriod.p, w.GradX.p, w.GradMu.p);
                    else if (tv)
                        hipLaunchKernelGGL(k_tv_grad_finish, dim3(P + 1, nb), dim3(128), 0, s, (const double*)w.Part.p,
                                           (const double*)w.Alpha.p, (const double*)w.Gp.p, (const double*)w.Tau.p, c, N, Npad, P,
                                           w.GradGp.p, w.GradTau.p, w.GradX.p, w.GradMu.p);
                    else
                        hipLaunchKernelGGL(k_grad_finish, dim3(P + 1, nb), dim3(128), 0, s, (const double*)w.Part.p,
                                           (const double*)w.Alpha.p, (const double*)w.Gp.p, c, N, Npad, P, w.GradGp.p, w.GradX.p,
                                           w.GradMu.p);
                })) return rc;
        }
        HIP_TRY(hipMemcpyAsync(out.data() + (size_t)b0 * fac.out_stride, fac.Out->p, sizeof(double) * (size_t)nb * fac.out_stride,
                               hipMemcpyDeviceToHost, s));
        if (contract) {
            HIP_TRY(hipMemcpyAsync(grad_gp + (size_t)b0 * 2 * c, w.GradGp, sizeof(double) * (size_t)nb * 2 * c, hipMemcpyDeviceToHost, s));
            if (tv) HIP_TRY(hipMemcpyAsync(grad_tau + (size_t)b0 * c, w.GradTau, sizeof(double) * (size_t)nb * c, hipMemcpyDeviceToHost, s));
            if (qp) {
                HIP_TRY(hipMemcpyAsync(qp->grad_gamma + (size_t)b0 * c, w.GradGamma, sizeof(double) * (size_t)nb * c, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipMemcpyAsync(qp->grad_period + (size_t)b0 * c, w.GradPeriod, sizeof(double) * (size_t)nb * c, hipMemcpyDeviceToHost, s));
            }
            if (grad_lwl)
                HIP_TRY(hipMemcpyAsync(grad_lwl + (size_t)b0 * c * N, w.GradX, sizeof(double) * (size_t)nb * c * N, hipMemcpyDeviceToHost, s));
            if (grad_mu) HIP_TRY(hipMemcpyAsync(grad_mu + b0, w.GradMu, sizeof(double) * nb, hipMemcpyDeviceToHost, s));
            if (orbits)
                if (int rc = orbit_back(h, w, s, nb, c, np, grad_orb + (size_t)b0 * np,
                                        grad_vel ? grad_vel + (size_t)b0 * c * ne : nullptr, fast.data() + b0))
                    return rc;
        } else if (orbits) {      // (the value only: the faster-than-light flags still decide it)
            HIP_TRY(hipMemcpyAsync(fast.data() + b0, w.TooFast, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipStreamSynchronize(s));       // the next group reuses the workspace and the caller's arrays are pageable
    }
    if (collect_timings(h)) return 1;
    // a negative hyper-parameter, a faster-than-light orbit, a tau that is no time scale, a Gamma or P that is none (qp_refused),
    // a K (or under the baseline an M) that does not factor -> -inf, and no gradient there
    for (int b = 0; b < B; ++b)
        if (values_out(out.data(), fac.out_stride, b,
                       proposal_refused(gp, c, b, orbits ? fast.data() : nullptr) || (tv && tau_refused(tau, c, b)) ||
                           (qp && qp_refused(qp->gamma, qp->period, c, b)),
                       lnp, fac.parts ? parts : nullptr) &&
            contract) {
            poison_gradient(b, c, N, ne, np, grad_gp, grad_tau, grad_lwl, grad_mu, grad_orb, grad_vel);
            if (qp) {
                fill_nan(qp->grad_gamma, b, c);
                fill_nan(qp->grad_period, b, c);
            }
        }
    return 0;
}

// The front of fisher_run, vel_fisher_launches and loo_run: new profiling records, the one grid and hyper-parameter vector up
static int single_front(psoap_chunk* h, hipStream_t s, int c, const double* lwl, const double* gp)
{
    h->recs.clear();
    HIP_TRY(hipMemcpyAsync(h->gws->Lwl, lwl, sizeof(double) * (size_t)c * h->N, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->gws->Gp, gp, sizeof(double) * 2 * c, hipMemcpyHostToDevice, s));
    return 0;
}

// The bracket that forms the inverse in f.Kinv: K^-1 by k_fisher_kinv or, under the baseline, Kt^-1 by k_marg_fisher_kinv
static int inverse_bracket(psoap_chunk* h, hipStream_t s, const Factored& fac, FisherWs& f)
{
    const double* A = h->gws->A.p;
    const int Npad = h->Npad, P = h->P;
    const dim3 tiles(P * (P + 1) / 2), threads(GEMM_THREADS);
    return prof_launch(h, s, PSOAP_K_GRAD, TILE_FLOPS * tile_units(P, fac.Q), 0.0, [&] {
        if (fac.marg)
            hipLaunchKernelGGL(k_marg_fisher_kinv, tiles, threads, GEMM_LDS_BYTES, s, A, fac.ld, Npad, P, (const double*)fac.Vt->p,
                               fac.ldm, fac.S, f.Kinv.p);
        else
            hipLaunchKernelGGL(k_fisher_kinv, tiles, threads, GEMM_LDS_BYTES, s, A, fac.ld, Npad, P, f.Kinv.p);
    });
}

// The Fisher information of the likelihood (fisher_kernels.hpp).  One matrix through the gradient's workspace and
// factorisation, then K^-1 and, tangent after tangent, K_t, Z = K_t K^-1 and the contraction of G_t = 1/2 (K^-1 Z + Z^T K^-1).
// `marg`: under Kt = K + Ht Ht^T (marg_fisher_kernels.hpp) -- the marginal gradient's factorisation, Kt^-1, the same tangents.
// With `tau` (c, as grad_run's; also with `marg`) K is the time-variable kernel over the handle's times and a tangent has a
// time-scale part, tan_tau (T, c; nullptr: zeros): the TV fill, tangent fill, contraction and finishing sums, and the dot
// with its time-scale terms.  The caller has made the checks of fisher_tv_check (with `marg`: of marg_tv_check).
// With `qp` (plain, with `tau`; the checks of fisher_qp_check) K is the quasi-periodic kernel: Gamma and P go up beside tau, a
// tangent has a Gamma and a period part as well, and the QP fill, tangent fill, contraction, finishing sums and dot run in the
// places of the time-variable ones.  With `qp` null the launches are those of the call without it.
static int fisher_run(psoap_chunk* h, const char* who, bool marg, int c, const double* lwl, const double* gp, const double* tau,
                      int T, const double* tan_lwl, const double* tan_gp, const double* tan_tau, double* fisher,
                      double* fisher_mu, const QpFisherArgs* qp = nullptr)
{
    const bool tv = tau != nullptr;
    if (!h || !lwl || !gp || !tan_gp || !fisher) FAIL(std::string(who) + ": bad arguments");
    if (c < 1 || c > 3) FAIL("number of components must be 1, 2 or 3");
    if (T < 1 || T > FISHER_MAX_T) FAIL(std::string(who) + ": the number of tangents must be between 1 and 32");
    if (int rc = analysis_refused(h, who, marg, 1, c)) return rc;
    DEVICE_SCOPE(h->device);
    if (int rc = enter_device(h->device)) return rc;
    hipStream_t s = h->streams[0];
    const Factored fac = factored(h, marg, 1, tv, qp != nullptr);
    const int N = h->N, Npad = h->Npad, P = h->P, ld = fac.ld, ntiles = P * (P + 1) / 2;
    const size_t sq = (size_t)Npad * Npad, CN = (size_t)c * N;
    if (!h->fws) h->fws.reset(new FisherWs());
    if (int rc = factored_ws_need(h, fac, s, false, false)) return rc;
    GradWs& w = *h->gws;
    FisherWs& f = *h->fws;
    if (marg) HIP_TRY(f.V.need(fac.S));
    HIP_TRY(f.Kinv.need(sq));
    HIP_TRY(f.Kt.need(sq));
    HIP_TRY(f.Z.need(sq));
    HIP_TRY(f.TanX.need((size_t)T * CN));
    HIP_TRY(f.TanGp.need((size_t)T * 2 * c));
    HIP_TRY(f.Part.need(qp ? fisher_qp_sizes(c, N, P, T, QpTile::DOUBLES).part
                           : (size_t)ntiles * (tv ? GradTile<true>::DOUBLES : GradTile<false>::DOUBLES)));
    HIP_TRY(f.GGp.need((size_t)T * 2 * c));
    if (tv) {
        HIP_TRY(f.TanTau.need((size_t)T * c));
        HIP_TRY(f.GTau.need((size_t)T * c));
    }
    if (qp)
        for (Grow<double>* g : {&f.TanGamma, &f.TanPeriod, &f.GGamma, &f.GPeriod})
            HIP_TRY(g->need(fisher_qp_sizes(c, N, P, T, QpTile::DOUBLES).temporal));
    HIP_TRY(f.GX.need((size_t)T * CN));
    HIP_TRY(f.Y.need(Npad));
    HIP_TRY(f.Mu.need(2));
    HIP_TRY(f.F.need((size_t)T * T));
    HIP_TRY(f.Info.need(1));
    if (int rc = single_front(h, s, c, lwl, gp)) return rc;
    if (tan_lwl) HIP_TRY(hipMemcpyAsync(f.TanX, tan_lwl, sizeof(double) * (size_t)T * CN, hipMemcpyHostToDevice, s));
    else HIP_TRY(hipMemsetAsync(f.TanX, 0, sizeof(double) * (size_t)T * CN, s));
    HIP_TRY(hipMemcpyAsync(f.TanGp, tan_gp, sizeof(double) * (size_t)T * 2 * c, hipMemcpyHostToDevice, s));
    if (tv) {
        HIP_TRY(hipMemcpyAsync(w.Tau, tau, sizeof(double) * c, hipMemcpyHostToDevice, s));
        if (tan_tau) HIP_TRY(hipMemcpyAsync(f.TanTau, tan_tau, sizeof(double) * (size_t)T * c, hipMemcpyHostToDevice, s));
        else HIP_TRY(hipMemsetAsync(f.TanTau, 0, sizeof(double) * (size_t)T * c, s));
    }
    if (qp) {
        HIP_TRY(hipMemcpyAsync(w.Gamma, qp->gamma, sizeof(double) * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(w.Period, qp->period, sizeof(double) * c, hipMemcpyHostToDevice, s));
        const std::pair<Grow<double>*, const double*> parts[] = {{&f.TanGamma, qp->tan_gamma}, {&f.TanPeriod, qp->tan_period}};
        for (const auto& [dst, src] : parts) {
            if (src) HIP_TRY(hipMemcpyAsync(dst->p, src, sizeof(double) * (size_t)T * c, hipMemcpyHostToDevice, s));
            else HIP_TRY(hipMemsetAsync(dst->p, 0, sizeof(double) * (size_t)T * c, s));
        }
    }
    // (F does not depend on the data: any mu_GP)
    if (int rc = factor_group(h, fac, s, 1, c, 0.0, false)) return rc;
    if (int rc = inverse_bracket(h, s, fac, f)) return rc;
    if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
            hipLaunchKernelGGL(k_acc_total, dim3(1), dim3(1), 0, s, (const MatAcc*)w.Acc.p, P, f.Info.p);
            hipLaunchKernelGGL(k_fisher_w1, dim3(N), dim3(256), 0, s, (const double*)w.A.p, ld, Npad, N, f.Y.p);
            if (marg) {
                hipLaunchKernelGGL(k_marg_fisher_v1, dim3(fac.S), dim3(256), 0, s, (const double*)fac.Vt->p, fac.ldm, fac.S, N,
                                   f.V.p);
                hipLaunchKernelGGL(k_marg_fisher_mu, dim3(1), dim3(256), 0, s, (const double*)f.Y.p, N, (const double*)f.V.p, fac.S,
                                   f.Mu.p);
            } else
                hipLaunchKernelGGL(k_fisher_mu, dim3(1), dim3(256), 0, s, (const double*)f.Y.p, N, f.Mu.p);
        })) return rc;
    // (static: the handle's times, w.Tau, f.TanTau and f.GTau may be null pointers; the static kernels do not read them)
    const double *times = h->dTimes.p, *dtau = w.Tau.p;
    for (int t = 0; t < T; ++t) {
        const double* tan_tau_t = tv ? f.TanTau.p + (size_t)t * c : nullptr;
        if (int rc = prof_launch(h, s, PSOAP_K_FILL, 0.0, 8.0 * (double)sq, [&] {
                with_components(c, [&](auto nc) {
                    if (qp) {
                        hipLaunchKernelGGL(k_qp_fisher_tangent_fill<nc()>, dim3(P * P), dim3(256), 0, s, f.Kt.p, Npad, N, P,
                                           (const double*)w.Lwl.p, times, (const double*)w.Gp.p, dtau, (const double*)w.Gamma.p,
                                           (const double*)w.Period.p, (const double*)(f.TanX.p + (size_t)t * CN),
                                           (const double*)(f.TanGp.p + (size_t)t * 2 * c), tan_tau_t,
                                           (const double*)(f.TanGamma.p + (size_t)t * c),
                                           (const double*)(f.TanPeriod.p + (size_t)t * c));
                        return;
                    }
                    hipLaunchKernelGGL(tv ? k_tv_fisher_tangent_fill<nc()> : k_fisher_tangent_fill<nc()>, dim3(P * P), dim3(256),
                                       0, s, f.Kt.p, Npad, N, P, (const double*)w.Lwl.p, times, (const double*)w.Gp.p, dtau,
                                       (const double*)(f.TanX.p + (size_t)t * CN),
                                       (const double*)(f.TanGp.p + (size_t)t * 2 * c), tan_tau_t);
                });
            })) return rc;
        if (int rc = prof_launch(h, s, PSOAP_K_GRAD, TILE_FLOPS * P * ((double)P * P + 2.0 * ntiles), 0.0, [&] {
                hipLaunchKernelGGL(k_fisher_gemm, dim3(P * P), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, (const double*)f.Kt.p,
                                   (const double*)f.Kinv.p, Npad, P, f.Z.p);
                with_components(c, [&](auto nc) {
                    if (qp) {
                        hipLaunchKernelGGL(k_qp_fisher_contract<nc()>, dim3(ntiles), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s,
                                           (const double*)f.Kinv.p, (const double*)f.Z.p, N, Npad, P, (const double*)w.Lwl.p, times,
                                           (const double*)w.Gp.p, dtau, (const double*)w.Gamma.p, (const double*)w.Period.p,
                                           f.Part.p);
                        return;
                    }
                    hipLaunchKernelGGL(tv ? k_tv_fisher_contract<nc()> : k_fisher_contract<nc()>, dim3(ntiles),
                                       dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, (const double*)f.Kinv.p, (const double*)f.Z.p, N,
                                       Npad, P, (const double*)w.Lwl.p, times, (const double*)w.Gp.p, dtau, f.Part.p);
                });
            })) return rc;
        // the gradient's finishing sums as they are: its alpha is W 1 here, and its sum over alpha goes nowhere (Mu[1])
        if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
                if (qp)
                    hipLaunchKernelGGL(k_qp_grad_finish, dim3(P + 1, 1), dim3(128), 0, s, (const double*)f.Part.p,
                                       (const double*)f.Y.p, (const double*)w.Gp.p, dtau, (const double*)w.Gamma.p,
                                       (const double*)w.Period.p, c, N, Npad, P, f.GGp.p + (size_t)t * 2 * c,
                                       f.GTau.p + (size_t)t * c, f.GGamma.p + (size_t)t * c, f.GPeriod.p + (size_t)t * c,
                                       f.GX.p + (size_t)t * CN, f.Mu.p + 1);
                else if (tv)
                    hipLaunchKernelGGL(k_tv_grad_finish, dim3(P + 1, 1), dim3(128), 0, s, (const double*)f.Part.p,
                                       (const double*)f.Y.p, (const double*)w.Gp.p, dtau, c, N, Npad, P,
                                       f.GGp.p + (size_t)t * 2 * c, f.GTau.p + (size_t)t * c, f.GX.p + (size_t)t * CN, f.Mu.p + 1);
                else
                    hipLaunchKernelGGL(k_grad_finish, dim3(P + 1, 1), dim3(128), 0, s, (const double*)f.Part.p,
                                       (const double*)f.Y.p, (const double*)w.Gp.p, c, N, Npad, P, f.GGp.p + (size_t)t * 2 * c,
                                       f.GX.p + (size_t)t * CN, f.Mu.p + 1);
            })) return rc;
    }
    // (static: no time-scale terms in the dot)
    if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
            if (qp) {
                hipLaunchKernelGGL(k_qp_fisher_dot, dim3(T, T), dim3(256), 0, s, (const double*)f.TanX.p, (const double*)f.TanGp.p,
                                   (const double*)f.TanTau.p, (const double*)f.TanGamma.p, (const double*)f.TanPeriod.p,
                                   (const double*)f.GX.p, (const double*)f.GGp.p, (const double*)f.GTau.p,
                                   (const double*)f.GGamma.p, (const double*)f.GPeriod.p, c, N, T, f.F.p);
                return;
            }
            hipLaunchKernelGGL(k_fisher_dot, dim3(T, T), dim3(256), 0, s, (const double*)f.TanX.p, (const double*)f.TanGp.p,
                               (const double*)(tv ? f.TanTau.p : nullptr), (const double*)f.GX.p, (const double*)f.GGp.p,
                               (const double*)(tv ? f.GTau.p : nullptr), c, N, T, f.F.p);
        })) return rc;
    MatAcc info;
    double value = 0.0;      // (marg: -inf also when M does not factor)
    if (marg) HIP_TRY(hipMemcpyAsync(&value, fac.Out->p, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(fisher, f.F, sizeof(double) * (size_t)T * T, hipMemcpyDeviceToHost, s));
    if (fisher_mu) HIP_TRY(hipMemcpyAsync(fisher_mu, f.Mu, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&info, f.Info, sizeof info, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (collect_timings(h)) return 1;
    // the conventions of the likelihood: a negative hyper-parameter, a tau that is no time scale, a Gamma or P that is none
    // (qp_refused) or a matrix that is not positive definite -> no information
    if (info.info != 0.0 || value == -INFINITY || proposal_refused(gp, c, 0) || (tv && tau_refused(tau, c, 0)) ||
        (qp && qp_refused(qp->gamma, qp->period, c, 0))) {
        fill_nan(fisher, 0, (size_t)T * T);
        fill_nan(fisher_mu, 0, 1);
    }
    return 0;
}

// The Fisher information of the per-epoch velocities (vel_fisher_kernels.hpp).  The launches of fisher_vel_run up to
// k_vel_finish, for it and for info_vel_run (inside the caller's device scope): afterwards F is in h->vws->F, K^-1 (fac.marg:
// Kt^-1, as fisher_run forms it) in the Fisher workspace, the plan in h->vws->Plan and the epoch of every pixel in
// h->vws->Epoch.  `values`: the value record and alpha (alpha_m) of the data at mu_GP as well (factor_group).
static int vel_fisher_launches(psoap_chunk* h, hipStream_t s, const Factored& fac, bool values, int c, const double* lwl,
                               const double* gp, double mu_GP, int n_epochs, const int32_t* epoch, VelFisherPlan& pl,
                               std::vector<int>& packed /* the caller keeps it until its stream is drained */)
{
    const int N = h->N, Npad = h->Npad, P = h->P, ntiles = P * (P + 1) / 2;
    const size_t sq = (size_t)Npad * Npad, T = (size_t)c * n_epochs;
    vel_fisher_plan(c, N, n_epochs, epoch, pl);
    vel_plan_pack(pl, packed);
    const VelPlanOffsets off = vel_plan_offsets(Npad, P, pl.S, n_epochs);
    if (!h->fws) h->fws.reset(new FisherWs());
    if (!h->vws) h->vws.reset(new VelFisherWs());
    if (int rc = factored_ws_need(h, fac, s, values, false)) return rc;
    GradWs& w = *h->gws;
    FisherWs& f = *h->fws;
    VelFisherWs& v = *h->vws;
    HIP_TRY(f.Kinv.need(sq));
    HIP_TRY(f.Info.need(1));
    HIP_TRY(v.Dv.need((size_t)c * sq));
    HIP_TRY(v.Z.need((size_t)c * sq));
    HIP_TRY(v.Part.need((size_t)pl.part_doubles));
    HIP_TRY(v.F.need(T * T));
    HIP_TRY(v.Plan.need(packed.size()));
    HIP_TRY(v.Epoch.need((size_t)N));
    if (int rc = single_front(h, s, c, lwl, gp)) return rc;
    HIP_TRY(hipMemcpyAsync(v.Plan, packed.data(), sizeof(int) * packed.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(v.Epoch, epoch, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, s));
    if (int rc = factor_group(h, fac, s, 1, c, mu_GP, values)) return rc;
    if (int rc = inverse_bracket(h, s, fac, f)) return rc;
    if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
            hipLaunchKernelGGL(k_acc_total, dim3(1), dim3(1), 0, s, (const MatAcc*)w.Acc.p, P, f.Info.p);
        })) return rc;
    const int* plan = v.Plan.p;
    if (int rc = prof_launch(h, s, PSOAP_K_FILL, 0.0, 8.0 * (double)sq * c, [&] {
            hipLaunchKernelGGL(k_vel_dv_fill, dim3(P * P, c), dim3(256), 0, s, v.Dv.p, sq, Npad, N, P, (const double*)w.Lwl.p,
                               (const double*)w.Gp.p, (const int*)v.Epoch.p);
        })) return rc;
    if (int rc = prof_launch(h, s, PSOAP_K_GRAD, TILE_FLOPS * pl.tile_units, 0.0, [&] {
            hipLaunchKernelGGL(k_vel_z, dim3(P * P, c), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, (const double*)f.Kinv.p,
                               (const double*)v.Dv.p, sq, Npad, plan + off.tiles_all, v.Z.p);
            for (int k = 0; k < c; ++k)
                for (int j = 0; j <= k; ++j) {
                    const double *Zk = v.Z.p + (size_t)k * sq, *Zj = v.Z.p + (size_t)j * sq;
                    const double *Dk = v.Dv.p + (size_t)k * sq, *Dj = v.Dv.p + (size_t)j * sq;
                    double* part = v.Part.p + (size_t)(k * (k + 1) / 2 + j) * pl.S * pl.S;
                    if (k == j)
                        hipLaunchKernelGGL(k_vel_contract<true>, dim3(ntiles), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s,
                                           (const double*)f.Kinv.p, Zk, Zj, Dk, Dj, Npad, pl.S, plan + off.tiles_upper,
                                           plan + off.slot_of, plan + off.slot_first, part);
                    else
                        hipLaunchKernelGGL(k_vel_contract<false>, dim3(P * P), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s,
                                           (const double*)f.Kinv.p, Zk, Zj, Dk, Dj, Npad, pl.S, plan + off.tiles_all,
                                           plan + off.slot_of, plan + off.slot_first, part);
                }
        })) return rc;
    return prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
        hipLaunchKernelGGL(k_vel_finish, dim3((unsigned)((T * T + 63) / 64)), dim3(64), 0, s, (const double*)v.Part.p, pl.S, c,
                           n_epochs, plan + off.epoch_ptr, plan + off.epoch_slots, plan + off.slot_block, v.F.p);
    });
}

// K^-1 as fisher_run; then Dv_k, Z_k = K^-1 Dv_k per component, the c (c + 1) / 2 products X_kj with their binning, the finishing sums
static int fisher_vel_run(psoap_chunk* h, int c, const double* lwl, const double* gp, int n_epochs, const int32_t* epoch, double* fisher)
{
    DEVICE_SCOPE(h->device);
    if (int rc = enter_device(h->device)) return rc;
    hipStream_t s = h->streams[0];
    const Factored fac = factored(h, false, 1);
    const size_t T = (size_t)c * n_epochs;
    VelFisherPlan pl;
    std::vector<int> packed;
    if (int rc = vel_fisher_launches(h, s, fac, false, c, lwl, gp, 0.0, n_epochs, epoch, pl, packed)) return rc;
    MatAcc info;
    HIP_TRY(hipMemcpyAsync(fisher, h->vws->F, sizeof(double) * T * T, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&info, h->fws->Info, sizeof info, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (collect_timings(h)) return 1;
    // the conventions of the likelihood: a negative hyper-parameter or a matrix that is not positive definite -> no information
    if (info.info != 0.0 || proposal_refused(gp, c, 0)) fill_nan(fisher, 0, T * T);
    return 0;
}

// The observed information of the per-epoch velocities (vel_newton_kernels.hpp).  Value, gradient, F and J from ONE factorisation:
// fisher_vel_run's launches with the value record and alpha, then the pair pass over K^-1, U, V = K^-1 U, U^T V and the finish.
static int info_vel_run(psoap_chunk* h, bool marg, int c, const double* lwl, const double* gp, double mu_GP, int n_epochs,
                        const int32_t* epoch, double* lnp, double* grad, double* fisher, double* observed)
{
    DEVICE_SCOPE(h->device);
    if (int rc = enter_device(h->device)) return rc;
    hipStream_t s = h->streams[0];
    const Factored fac = factored(h, marg, 1);
    const int N = h->N, Npad = h->Npad, P = h->P;
    const size_t T = (size_t)c * n_epochs;
    const int Tpad = round_up((int)T, NB), Tp = Tpad / NB;
    VelFisherPlan pl;
    std::vector<int> packed;
    if (int rc = vel_fisher_launches(h, s, fac, true, c, lwl, gp, mu_GP, n_epochs, epoch, pl, packed)) return rc;
    const VelPlanOffsets off = vel_plan_offsets(Npad, P, pl.S, n_epochs);
    const size_t S = (size_t)pl.S;
    if (!h->nws) h->nws.reset(new VelNewtonWs());
    GradWs& w = *h->gws;
    FisherWs& f = *h->fws;
    VelFisherWs& v = *h->vws;
    VelNewtonWs& nw = *h->nws;
    HIP_TRY(nw.Y.need((size_t)c * S * Npad));
    HIP_TRY(nw.A.need((size_t)c * S * S));
    HIP_TRY(nw.B.need((size_t)c * S * S));
    HIP_TRY(nw.U.need((size_t)Npad * Tpad));
    HIP_TRY(nw.V.need((size_t)Npad * Tpad));
    HIP_TRY(nw.M.need((size_t)Tpad * Tpad));
    HIP_TRY(nw.J.need(T * T));
    HIP_TRY(nw.Grad.need(T));
    const int* plan = v.Plan.p;
    if (int rc = prof_launch(h, s, PSOAP_K_FILL, 0.0, 8.0 * (double)Npad * Npad * c, [&] {
            hipLaunchKernelGGL(k_vel_pair, dim3(P * P, c), dim3(VEL_PAIR_THREADS), 0, s, (const double*)f.Kinv.p,
                               (const double*)w.Alpha.p, Npad, N, P, pl.S, (const double*)w.Lwl.p, (const double*)w.Gp.p,
                               (const int*)v.Epoch.p, plan + off.slot_of, plan + off.slot_first, nw.Y.p, nw.A.p, nw.B.p);
        })) return rc;
    if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
            hipLaunchKernelGGL(k_vel_u, dim3((Npad + 255) / 256, Tpad), dim3(256), 0, s, (const double*)nw.Y.p, Npad, N, pl.S, c,
                               n_epochs, Tpad, (const int*)v.Epoch.p, plan + off.epoch_ptr, plan + off.epoch_slots, nw.U.p);
        })) return rc;
    if (int rc = prof_launch(h, s, PSOAP_K_GRAD, TILE_FLOPS * ((double)P * P * Tp + 0.5 * P * Tp * (Tp + 1.0)), 0.0, [&] {
            hipLaunchKernelGGL(k_vel_v, dim3(P, Tp), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, (const double*)f.Kinv.p,
                               (const double*)nw.U.p, Npad, Tpad, nw.V.p);
            hipLaunchKernelGGL(k_vel_gram, dim3(Tp, Tp), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, (const double*)nw.U.p,
                               (const double*)nw.V.p, Npad, Tpad, nw.M.p);
        })) return rc;
    if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
            hipLaunchKernelGGL(k_vel_newton_finish, dim3((unsigned)((T * T + 63) / 64)), dim3(64), 0, s, (const double*)nw.A.p,
                               (const double*)nw.B.p, (const double*)nw.M.p, (const double*)v.F.p, pl.S, c, n_epochs, Tpad,
                               plan + off.epoch_ptr, plan + off.epoch_slots, nw.J.p, nw.Grad.p);
        })) return rc;
    MatAcc info;
    std::vector<double> out((size_t)fac.out_stride);
    HIP_TRY(hipMemcpyAsync(out.data(), fac.Out->p, sizeof(double) * (size_t)fac.out_stride, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(fisher, v.F, sizeof(double) * T * T, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(observed, nw.J, sizeof(double) * T * T, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(grad, nw.Grad, sizeof(double) * T, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&info, f.Info, sizeof info, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (collect_timings(h)) return 1;
    // the conventions: a negative hyper-parameter or a matrix that is not positive definite -> -inf, no gradient, no information
    if (values_out(out.data(), fac.out_stride, 0, proposal_refused(gp, c, 0) || info.info != 0.0, lnp, nullptr)) {
        for (double* v : {fisher, observed}) fill_nan(v, 0, T * T);
        fill_nan(grad, 0, T);
    }
    return 0;
}

// Leave-one-out cross-validation of the likelihood (loo_kernels.hpp).  One matrix through the gradient's factorisation, alpha
// as the gradient makes it, the band of K^-1 into the packed epoch blocks, their staged factorisation, the finishing kernel.
// `marg`: under Kt = K + Ht Ht^T (marg_fisher_kernels.hpp) -- the factorisation, the value and alpha_m are the marginal
// gradient's for one matrix and k_marg_loo_band scatters the band of Kt^-1 where k_loo_band scatters that of K^-1.
// With `tau` (c; plain only, as grad_run's) K is the time-variable kernel over the handle's times: the factorisation alone
// knows -- everything behind it reads K through W and alpha.  With `qp` (its gamma and period, c; plain, with `tau`) it is the
// quasi-periodic kernel, and again the factorisation alone knows; with `qp` null the launches are those of the call without it.
static int loo_run(psoap_chunk* h, const char* who, bool marg, int c, const double* lwl, const double* gp, const double* tau,
                   double mu_GP, const int32_t* epoch, int n_epochs, double* lnp, double* loo_logp, double* pix_mean, double* pix_var,
                   double* pix_logp, double* ep_resid, double* ep_chi2, double* ep_logp, int32_t* ep_npix,
                   const QpArgs* qp = nullptr)
{
    if (!h || !lwl || !gp) FAIL(std::string(who) + ": bad arguments");
    if (c < 1 || c > 3) FAIL("number of components must be 1, 2 or 3");
    if (epoch && n_epochs < 1) FAIL(std::string(who) + ": n_epochs must be at least 1");
    if (int rc = analysis_refused(h, who, marg, 1, c)) return rc;
    const int N = h->N, Npad = h->Npad, P = h->P;
    LooLayout lay;
    if (const char* why = loo_layout(epoch, N, n_epochs, lay)) FAIL(std::string(who) + ": " + why);
    const int ne = epoch ? n_epochs : 0, nblk = (int)lay.blocks.size(), ntile = (int)lay.tiles.size();
    if (!epoch) ep_resid = ep_chi2 = ep_logp = nullptr, ep_npix = nullptr;
    DEVICE_SCOPE(h->device);
    if (int rc = enter_device(h->device)) return rc;
    const bool tv = tau != nullptr;
    const Factored fac = factored(h, marg, 1, tv, qp != nullptr);
    hipStream_t s = h->streams[0];
    if (!h->lws) h->lws.reset(new LooWs());
    if (int rc = factored_ws_need(h, fac, s, true, false)) return rc;
    GradWs& w = *h->gws;
    LooWs& l = *h->lws;
    HIP_TRY(l.Blk.need((size_t)lay.block_doubles));
    HIP_TRY(l.Rhs.need((size_t)lay.rhs_doubles));
    HIP_TRY(l.Sol.need((size_t)lay.rhs_doubles));
    HIP_TRY(l.Wt.need((size_t)lay.wt_doubles));
    HIP_TRY(l.Acc.need((size_t)nblk * ACC_ROWS));
    HIP_TRY(l.Diag.need(N));
    HIP_TRY(l.Pix.need((size_t)3 * N));
    HIP_TRY(l.EpResid.need(N));
    HIP_TRY(l.EpOut.need((size_t)2 * (ne + 1)));
    HIP_TRY(l.EpNpix.need((size_t)ne + 1));
    HIP_TRY(l.Logp.need(1));
    HIP_TRY(l.Blocks.need(nblk));
    HIP_TRY(l.Tiles.need(ntile));
    HIP_TRY(l.PixBlock.need(N));
    HIP_TRY(l.EpBlock.need(lay.epoch_block.size()));
    if (int rc = single_front(h, s, c, lwl, gp)) return rc;
    if (tv) HIP_TRY(hipMemcpyAsync(w.Tau, tau, sizeof(double) * c, hipMemcpyHostToDevice, s));
    if (qp) {
        HIP_TRY(hipMemcpyAsync(w.Gamma, qp->gamma, sizeof(double) * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(w.Period, qp->period, sizeof(double) * c, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(l.Blocks, lay.blocks.data(), sizeof(LooBlock) * (size_t)nblk, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(l.Tiles, lay.tiles.data(), sizeof(LooTile) * (size_t)ntile, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(l.PixBlock, lay.pixel_block.data(), sizeof(int) * (size_t)N, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(l.EpBlock, lay.epoch_block.data(), sizeof(int) * lay.epoch_block.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(l.Blk, 0, sizeof(double) * (size_t)lay.block_doubles, s));
    // the value and alpha exactly as psoap_chunk_lnlike_grad (marg: psoap_chunk_lnlike_marg_grad) makes them for one matrix
    auto pad = [&] { hipLaunchKernelGGL(k_loo_pad, dim3(nblk), dim3(128), 0, s, (const LooBlock*)l.Blocks.p, l.Blk.p); };
    if (int rc = factor_group(h, fac, s, 1, c, mu_GP, true, &pad)) return rc;
    double bunits = 0.0;      // executed 128^3 products of the band: a diagonal tile issues three quarters of its MFMAs
    for (const LooTile& t : lay.tiles) bunits += (t.ti == t.tj ? 0.75 : 1.0) * (P - t.tj + fac.Q);
    if (int rc = prof_launch(h, s, PSOAP_K_GRAD, TILE_FLOPS * bunits, 0.0, [&] {
            if (marg)
                hipLaunchKernelGGL(k_marg_loo_band, dim3(ntile), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, (const double*)w.A.p, fac.ld, N,
                                   Npad, (const double*)fac.Vt->p, fac.ldm, fac.S, (const LooTile*)l.Tiles.p,
                                   (const int*)l.PixBlock.p, (const LooBlock*)l.Blocks.p, l.Blk.p);
            else
                hipLaunchKernelGGL(k_loo_band, dim3(ntile), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, (const double*)w.A.p, fac.ld, N, Npad,
                                   (const LooTile*)l.Tiles.p, (const int*)l.PixBlock.p, (const LooBlock*)l.Blocks.p, l.Blk.p);
        })) return rc;
    if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
            hipLaunchKernelGGL(k_loo_rhs, dim3(nblk), dim3(256), 0, s, (const LooBlock*)l.Blocks.p, (const double*)l.Blk.p,
                               (const double*)w.Alpha.p, l.Rhs.p, l.Diag.p, l.Acc.p);
        })) return rc;
    // the packed blocks through the staged factorisation, one matrix of the batch per block, group after group of equal side
    if (epoch)
        for (const LooGroup& g : lay.groups) {
            const LooBlock& b0 = lay.blocks[(size_t)g.first];
            const int S = g.side, Pb = S / NB, nb = g.count;
            const size_t bstride = (size_t)S * S, wstride = (size_t)Pb * NB * NB;
            for (int p = 0; p < Pb; ++p) {
                const int k0 = p * NB, nt = Pb - p;
                const StagedRow row{l.Blk.p + b0.offset, bstride, S, l.Rhs.p + b0.rhs, S, l.Acc.p + (size_t)g.first * ACC_ROWS,
                                    l.Wt.p + b0.wt + (size_t)p * NB * NB, wstride, nt - 1};
                auto update = [&] {
                    hipLaunchKernelGGL(k_panel_update, dim3(nt, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, row.A, bstride, S, k0);
                };
                if (int rc = staged_row(h, s, row, nb, k0, p > 0 ? &update : nullptr, TILE_FLOPS * p * nt * nb)) return rc;
            }
        }
    if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
            hipLaunchKernelGGL(k_loo_finish, dim3(ne + 1), dim3(256), 0, s, N, ne, (const int*)l.EpBlock.p, (const LooBlock*)l.Blocks.p,
                               (const double*)l.Blk.p, (const double*)l.Wt.p, (const double*)l.Rhs.p, l.Sol.p, (const MatAcc*)l.Acc.p,
                               (const double*)w.Alpha.p, (const double*)l.Diag.p, (const double*)h->dFl.p, l.Pix.p, l.Pix.p + N,
                               l.Pix.p + 2 * (size_t)N, l.EpResid.p, l.EpOut.p, l.EpOut.p + (ne + 1), l.EpNpix.p, l.Logp.p);
        })) return rc;
    double value = 0.0;
    HIP_TRY(hipMemcpyAsync(&value, fac.Out->p, sizeof(double), hipMemcpyDeviceToHost, s));
    if (loo_logp) HIP_TRY(hipMemcpyAsync(loo_logp, l.Logp, sizeof(double), hipMemcpyDeviceToHost, s));
    if (pix_mean) HIP_TRY(hipMemcpyAsync(pix_mean, l.Pix, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, s));
    if (pix_var) HIP_TRY(hipMemcpyAsync(pix_var, l.Pix.p + N, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, s));
    if (pix_logp) HIP_TRY(hipMemcpyAsync(pix_logp, l.Pix.p + 2 * (size_t)N, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, s));
    if (ep_resid) HIP_TRY(hipMemcpyAsync(ep_resid, l.EpResid, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, s));
    if (ep_chi2) HIP_TRY(hipMemcpyAsync(ep_chi2, l.EpOut, sizeof(double) * (size_t)ne, hipMemcpyDeviceToHost, s));
    if (ep_logp) HIP_TRY(hipMemcpyAsync(ep_logp, l.EpOut.p + (ne + 1), sizeof(double) * (size_t)ne, hipMemcpyDeviceToHost, s));
    if (ep_npix) HIP_TRY(hipMemcpyAsync(ep_npix, l.EpNpix, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));       // (the layout's vectors and the caller's pageable arrays)
    if (collect_timings(h)) return 1;
    // the conventions: a negative hyper-parameter, a tau that is no time scale, a Gamma or P that is none (qp_refused) or a
    // matrix that is not positive definite -> -inf, and nothing else to say
    if (proposal_refused(gp, c, 0) || (tv && tau_refused(tau, c, 0)) || (qp && qp_refused(qp->gamma, qp->period, c, 0)))
        value = -INFINITY;
    if (lnp) *lnp = value;
    if (value == -INFINITY) {
        fill_nan(loo_logp, 0, 1);
        for (double* v : {pix_mean, pix_var, pix_logp, ep_resid}) fill_nan(v, 0, N);
        for (double* v : {ep_chi2, ep_logp}) fill_nan(v, 0, ne);
    }
    return 0;
}

// The likelihood with a per-epoch continuum polynomial integrated out (marg_kernels.hpp).  Group after group of matrices
// through the gradient's workspace as [K | Ht] (ld = Npad + 128 Q), then the Gram matrices through the staged kernels once
// more.  This K sweep stays apart from marg_grad_factor's [K | I | Ht]: the value alone has no appended identity to pay for.
// With `tau` (B, c) K is the time-variable kernel over the handle's times: the fill alone knows.
static int marg_run(psoap_chunk* h, int B, int c, const double* lwl, const double* gp, const double* tau, double mu_GP, double* lnp,
                    double* parts, double* beta, double* beta_cov, double* fl_cor)
{
    const bool tv = tau != nullptr;
    DEVICE_SCOPE(h->device);
    if (int rc = enter_device(h->device)) return rc;
    const MargPlan& pl = h->marg.plan;
    const int N = h->N, Npad = h->Npad, P = h->P, Q = pl.Q, q = pl.q, order = pl.order;
    const int S = NB * Q, ld = Npad + S, ldm = 2 * S, ldh = S;
    const size_t mstride = (size_t)Npad * ld, m_stride = (size_t)S * ldm, wstride = (size_t)Q * NB * NB;
    const int G = marg_group_size(B, Npad, Q), ngram = Q * (Q + 1) / 2;
    const bool want_cov = beta_cov != nullptr, want_sol = beta != nullptr || fl_cor != nullptr;
    if (!h->gws) h->gws.reset(new GradWs());
    if (!h->mws) h->mws.reset(new MargWs());
    GradWs& w = *h->gws;
    MargWs& m = *h->mws;
    if (int rc = grad_ws_need(h, w, G, mstride, false, false, 0, 0, tv)) return rc;
    HIP_TRY(m.M.need((size_t)G * m_stride));
    if (int rc = marg_ws_need(h, m, G, want_cov)) return rc;
    hipStream_t s = h->streams[0];
    if (int rc = marg_basis(h, m, s)) return rc;
    const int* tab = m.Tab.p;
    h->recs.clear();
    std::vector<double> out((size_t)B * 5);
    for (int b0 = 0; b0 < B; b0 += G) {
        const int nb = (B - b0 < G) ? B - b0 : G;
        HIP_TRY(hipMemcpyAsync(w.Lwl, lwl + (size_t)b0 * c * N, sizeof(double) * (size_t)nb * c * N, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(w.Gp, gp + (size_t)b0 * 2 * c, sizeof(double) * (size_t)nb * 2 * c, hipMemcpyHostToDevice, s));
        if (tv) HIP_TRY(hipMemcpyAsync(w.Tau, tau + (size_t)b0 * c, sizeof(double) * (size_t)nb * c, hipMemcpyHostToDevice, s));
        if (int rc = prof_launch(h, s, PSOAP_K_FILL, 0.0, (double)nb * 12.0 * N * (N + 1.0), [&] {
                launch_grad_fill(h, w, s, nb, c, mstride, ld, tv);
                hipLaunchKernelGGL(k_marg_load, dim3(Q * P, nb), dim3(256), 0, s, w.A.p, mstride, ld, Npad, P, (const double*)m.Ht.p,
                                   ldh, tab);
            })) return rc;
        if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
                hipLaunchKernelGGL(k_init_rhs, dim3((Npad + 255) / 256, nb), dim3(256), 0, s, w.R.p, Npad, N, h->dFl, mu_GP, w.Acc.p);
            })) return rc;
        // block row p: the rest of K's row and the appended slots whose first non-zero block row is <= p
        for (int p = 0; p < P; ++p) {
            const int k0 = p * NB, act = pl.active[(size_t)p];
            auto update = [&] {
                hipLaunchKernelGGL(k_marg_panel_update, dim3(P - p + act, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, w.A.p, mstride, ld,
                                   k0, P, tab);
            };
            if (int rc = staged_row(h, s, grad_row(w, mstride, ld, Npad, P - p - 1 + act), nb, k0, p > 0 ? &update : nullptr,
                                    TILE_FLOPS * p * (P - p + act) * nb))
                return rc;
        }
        if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] { launch_marg_rhs(h, m, s, nb, w.A.p, mstride, ld, w.R.p); })) return rc;
        if (int rc = prof_launch(h, s, PSOAP_K_GRAD, TILE_FLOPS * gram_units(pl, Npad) * nb, 0.0, [&] {
                hipLaunchKernelGGL(k_marg_gram, dim3(ngram, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, (const double*)w.A.p, mstride, ld,
                                   Npad, (const MargTile*)m.Tiles.p, m.M.p, m_stride, ldm);
                if (want_cov) hipLaunchKernelGGL(k_grad_init, dim3(ngram, nb), dim3(256), 0, s, m.M.p, m_stride, ldm, S, Q);
            })) return rc;
        // M = U_M^T U_M with bt alongside; with the covariance asked for, [M | I] as the gradient factors [K | I]
        for (int p = 0; p < Q; ++p) {
            const int k0 = p * NB;
            const StagedRow row{m.M.p, m_stride, ldm, m.Rhs.p, S, m.AccM.p, m.WtM.p + (size_t)p * NB * NB, wstride,
                                want_cov ? Q : Q - p - 1};
            auto update = [&] {
                if (want_cov)
                    hipLaunchKernelGGL(k_grad_panel_update, dim3(Q + 1, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, m.M.p, m_stride, ldm,
                                       k0, Q);
                else
                    hipLaunchKernelGGL(k_panel_update, dim3(Q - p, nb), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, m.M.p, m_stride, ldm, k0);
            };
            if (int rc = staged_row(h, s, row, nb, k0, p > 0 ? &update : nullptr, TILE_FLOPS * p * (want_cov ? Q : Q - p) * nb))
                return rc;
        }
        if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] { launch_marg_finish(h, w, m, s, nb, m.M.p, m_stride, ldm, want_sol); }))
            return rc;
        if (want_cov)
            if (int rc = prof_launch(h, s, PSOAP_K_GRAD, 0.0, 0.0, [&] {
                    for (int b = 0; b < nb; ++b)
                        hipLaunchKernelGGL(k_fisher_kinv, dim3(ngram), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s,
                                           (const double*)(m.M.p + (size_t)b * m_stride), ldm, S, Q, m.Minv.p + (size_t)b * S * S);
                    hipLaunchKernelGGL(k_marg_cov, dim3(q, nb), dim3(256), 0, s, (const double*)m.Minv.p, S, q, order,
                                       (const double*)m.Sd.p, m.Cov.p);
                })) return rc;
        HIP_TRY(hipMemcpyAsync(out.data() + (size_t)b0 * 5, m.Out, sizeof(double) * (size_t)nb * 5, hipMemcpyDeviceToHost, s));
        if (beta) HIP_TRY(hipMemcpyAsync(beta + (size_t)b0 * q, m.Beta, sizeof(double) * (size_t)nb * q, hipMemcpyDeviceToHost, s));
        if (fl_cor) HIP_TRY(hipMemcpyAsync(fl_cor + (size_t)b0 * N, m.Flc, sizeof(double) * (size_t)nb * N, hipMemcpyDeviceToHost, s));
        if (want_cov)
            HIP_TRY(hipMemcpyAsync(beta_cov + (size_t)b0 * q * q, m.Cov, sizeof(double) * (size_t)nb * q * q, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));       // the next group reuses the workspace and the caller's arrays are pageable
    }
    if (collect_timings(h)) return 1;
    // the conventions: a negative hyper-parameter, a tau that is no time scale, a K that is not positive definite or an M that
    // fails to factor -> -inf only
    for (int b = 0; b < B; ++b) {
        if (!values_out(out.data(), 5, b, proposal_refused(gp, c, b) || (tv && tau_refused(tau, c, b)), lnp, parts)) continue;
        fill_nan(beta, b, q);
        fill_nan(beta_cov, b, (size_t)q * q);
        fill_nan(fl_cor, b, N);
    }
    return 0;
}
