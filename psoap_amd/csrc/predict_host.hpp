// predict_host.hpp -- the host side of the predict family: the workspace, the Sigma download, the steps that the plain
// call (predict_run), the one under the marginalised continuum (marg_predict_run) and the draws share, and predict_run
// itself.  Part of psoap_gp.hip, included behind staged_row: it uses that file's error macros, prof_launch and staged_row.
// The arithmetic of a call is predict_plan.hpp's, the kernels are predict_kernels.hpp's.  (factor_host.hpp comes behind it.)
//
// Every step queues on the stream it is given and books nothing: marg_predict_run calls them inside its prof_launch
// brackets, predict_run has no handle to book into.
#pragma once
#include <atomic>
#include <chrono>
#include <thread>

#include "predict_kernels.hpp"
#include "predict_plan.hpp"

namespace psoap {

// timings of the last predict call (ms): everything on the device up to mu / Sigma complete, the Sigma
// download, and the whole call (host wall clock)
struct PredictTimes {
    double device_ms = 0.0, factor_ms = 0.0, sigma_ms = 0.0, download_ms = 0.0, total_ms = 0.0;
    double flops = 0.0;
};

struct PredictWs {
    Grow<double> K, W, R, Lwl, Pred, Fl, Sig, Gp, S, Mu, M0, Part, Colx;
    Grow<MatAcc> Acc;
    DagWorkspace dag;
    Grow<unsigned long long> Tlog;   // per-task stamps of the launch (PSOAP_PREDICT_TLOG=<file>: tools/predict_timeline.py)
    Grow<DagMat> Mat;
    Grow<double, true> hSmall;   // pinned staging, laid out by predict_staging (predict_plan.hpp)
    // what the task list in `dag` was built for
    int plan_P = -1, plan_Mt = -1, plan_workers = -1, plan_scheme = -2, plan_Ms = -1;
    int workers = 0, n_cus = 0;   // persistent workgroups the device admits; compute units
    Stream stream;
    Event ev[5];                  // (timed)
    Grow<double> Var, Prior, Rowx, Diag;
    Grow<double> Tpred, Tau;      // the prediction dates (M) and the components' time scales (predict_tv_run)
    PredictTimes times;
};

// Host side of the Sigma download.  The caller's array is pageable and, coming from numpy, freshly mapped; a plain D2H
// into it is staged by the runtime at 6-25 GB/s with a large spread (3-12 ms for the 75 MB of the retrieve shape).  The
// array is therefore page-locked IN PLACE (hipHostRegister: 2.6-3.1 ms, first-touch faults included) by a helper
// thread while the GPU is still factoring, the copy then runs at the link rate (1.4 ms) straight into it, and the
// registration is dropped afterwards (10 us).  (Round 3 first built a pinned bounce buffer emptied by 16 host threads:
// 1.7 ms on one box, 3.7 ms on another -- NUMA placement of buffer and threads.)  Small outputs skip all that.
struct SigmaPin {
    double* ptr = nullptr;
    size_t bytes = 0;
    int device = 0;
    std::thread th;
    std::atomic<int> ok{0};
    bool started = false;
    hipStream_t copy_stream = nullptr;      // an asynchronous copy INTO the array was queued on this stream
    bool copy_queued = false;
    static constexpr size_t MIN_BYTES = (size_t)4 << 20;

    void start(double* out, size_t n_bytes, int dev)
    {
        if (n_bytes < MIN_BYTES) return;
        ptr = out;
        bytes = n_bytes;
        device = dev;
        started = true;
        th = std::thread([this] {
            if (hipSetDevice(device) == hipSuccess && hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess)
                ok.store(1, std::memory_order_release);
        });
    }
    // -> true when the array is page-locked (the copy may then be asynchronous on any stream)
    bool wait()
    {
        if (started && th.joinable()) th.join();
        return ok.load(std::memory_order_acquire) != 0;
    }
    void queued_on(hipStream_t s)
    {
        copy_stream = s;
        copy_queued = true;
    }
    void release()
    {
        if (started && th.joinable()) th.join();
        // (an early return may come here with the DMA into the array still in flight: the registration outlives it)
        if (copy_queued) (void)hipStreamSynchronize(copy_stream);
        copy_queued = false;
        if (ok.load()) (void)hipHostUnregister(ptr);
        ok.store(0);
        started = false;
    }
    ~SigmaPin() { release(); }
};

}  // namespace psoap

// ---- the steps ---------------------------------------------------------------------------------------------------------
// the handle's predict workspace, made on first use: the workgroups the handle found, at most two per compute unit (as
// predict_ws_init)
static PredictWs& predict_ws_of(psoap_chunk* h)
{
    if (!h->pws) {
        h->pws.reset(new PredictWs());
        h->pws->workers = dag_two_per_cu(h->dag_grid, h->n_cus);
        h->pws->n_cus = h->n_cus;
    }
    return *h->pws;
}

// the workspace's stream and events, made on first use
static int predict_stream(PredictWs& ws)
{
    if (!ws.stream) {
        HIP_TRY(ws.stream.create());
        for (Event& e : ws.ev) HIP_TRY(e.create(hipEventDefault));
    }
    return 0;
}

// the buffers every call needs, for rows of ld doubles and n_small doubles of staging
static int predict_need(PredictWs& ws, const PredictShape& g, size_t ld, size_t n_small)
{
    HIP_TRY(ws.K.need((size_t)g.Npad * ld));
    HIP_TRY(ws.W.need(WT_STRIDE));
    HIP_TRY(ws.R.need(g.Npad));
    HIP_TRY(ws.Acc.need(ACC_ROWS + 1));      // the records of the block rows + their total (k_acc_total)
    HIP_TRY(ws.Lwl.need((size_t)g.c * g.N));
    HIP_TRY(ws.Pred.need((size_t)g.c * g.M));
    HIP_TRY(ws.Gp.need(6));
    HIP_TRY(ws.Mu.need(g.Rq_pad));
    HIP_TRY(ws.M0.need(g.Rq_pad));
    HIP_TRY(ws.Part.need((size_t)g.nslab * g.Rtot_pad));
    HIP_TRY(ws.hSmall.need(n_small));
    return 0;
}

// grids and hyper-parameters, fl / sigma where they are not resident on the device (nullptr: they are), the prior means
static int predict_upload(PredictWs& ws, const PredictShape& g, hipStream_t s, const double* lwl, const double* lwl_pred,
                          const double* gp, const double* mu_c, const double* fl, const double* sigma, double* h_m0)
{
    HIP_TRY(hipMemcpyAsync(ws.Lwl, lwl, sizeof(double) * (size_t)g.c * g.N, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ws.Pred, lwl_pred, sizeof(double) * (size_t)g.c * g.M, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ws.Gp, gp, sizeof(double) * 2 * g.c, hipMemcpyHostToDevice, s));
    if (fl) {
        HIP_TRY(ws.Fl.need(g.N));
        HIP_TRY(ws.Sig.need(g.N));
        HIP_TRY(hipMemcpyAsync(ws.Fl, fl, sizeof(double) * g.N, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(ws.Sig, sigma, sizeof(double) * g.N, hipMemcpyHostToDevice, s));
    }
    predict_prior_means(g, mu_c, h_m0);
    HIP_TRY(hipMemcpyAsync(ws.M0, h_m0, sizeof(double) * g.Rq, hipMemcpyHostToDevice, s));
    return 0;
}

static GpHost gp_host(const double* gp, int k0, int n)      // components k0 .. k0 + n - 1, the rest zero
{
    GpHost g;
    for (int k = 0; k < 6; ++k) g.v[k] = (k < 2 * n) ? gp[2 * k0 + k] : 0.0;
    return g;
}

// [K | Cx^T] in rows of ld doubles: cleared (padding rows and columns must be exact zeros), K's upper tiles, Cx^T
static void predict_fill(PredictWs& ws, const PredictShape& g, hipStream_t s, size_t ld, const double* gp, const double* dSig)
{
    const int c = g.c, N = g.N, M = g.M;
    double *dK = ws.K, *dLwl = ws.Lwl, *dPred = ws.Pred;
    hipLaunchKernelGGL(k_zero, dim3(2048), dim3(256), 0, s, dK, (size_t)g.Npad * ld);
    with_components(c, [&](auto nc) {
        hipLaunchKernelGGL(k_fill_sym<nc()>, dim3(g.P * (g.P + 1) / 2, 1), dim3(256), 0, s, dK, (size_t)0, (int)ld, N, g.P,
                           (const double*)dLwl, (const double*)ws.Gp.p, dSig, 1);
    });
    if (g.mode == 0) {
        // C = vstack(V12_f, V12_g, ..) (:136,:246): column block k of Cx^T is component k alone
        for (int k = 0; k < c; ++k)
            launch_region_c(s, 1, dK, ld, g.Npad + k * M, N, M, dLwl + (size_t)k * N, 0, dPred + (size_t)k * M, 0, gp_host(gp, k, 1), 0, 0.0);
    } else {
        // V12 = V12_f + V12_g (+ V12_h) (:171,:279); predict_f's single V12 (:39-40) is the C = 1 case
        launch_region_c(s, c, dK, ld, g.Npad, N, M, dLwl, (size_t)N, dPred, (size_t)M, gp_host(gp, 0, c), 0, 0.0);
    }
}

// the prior covariance of the prediction into S, upper tiles only (the product mirrors the result): mode 0
// A = blockdiag(V11_f_predict, V11_g_predict, ..) (:124-125,:234-236), otherwise V11 = the sum of the component priors with
// the caller's nugget on the diagonal (1e-8 only in the two-component sum, :165 vs :271)
static void predict_fill_prior(PredictWs& ws, const PredictShape& g, hipStream_t s, const double* gp, double nugget)
{
    const int c = g.c, M = g.M, Rq_pad = g.Rq_pad;
    double *dS = ws.S, *dPred = ws.Pred;
    if (g.mode == 0) {
        hipLaunchKernelGGL(k_zero, dim3(1024), dim3(256), 0, s, dS, (size_t)Rq_pad * Rq_pad);
        for (int k = 0; k < c; ++k)
            launch_region_c(s, 1, dS + (size_t)k * M * Rq_pad, (size_t)Rq_pad, k * M, M, M, dPred + (size_t)k * M, 0, dPred + (size_t)k * M, 0,
                            gp_host(gp, k, 1), 1, 0.0);
    } else {
        if (Rq_pad != g.Rq) hipLaunchKernelGGL(k_zero, dim3(1024), dim3(256), 0, s, dS, (size_t)Rq_pad * Rq_pad);
        launch_region_c(s, c, dS, (size_t)Rq_pad, 0, M, M, dPred, (size_t)M, dPred, (size_t)M, gp_host(gp, 0, c), 1, nugget);
    }
}

// predict_fill under the time-variable kernel, launch for launch: K by k_fill_sym_tv over the handle's times dT with ws.Tau,
// the blocks of Cx^T by k_fill_region_tv -- rows at the pixels' times, columns at the prediction dates ws.Tpred (M, shared by
// the components)
static void predict_fill_tv(PredictWs& ws, const PredictShape& g, hipStream_t s, size_t ld, const double* gp, const double* tau,
                            const double* dT, const double* dSig)
{
    const int c = g.c, N = g.N, M = g.M;
    double *dK = ws.K, *dLwl = ws.Lwl, *dPred = ws.Pred;
    const double* dTp = ws.Tpred;
    TauHost th;
    hipLaunchKernelGGL(k_zero, dim3(2048), dim3(256), 0, s, dK, (size_t)g.Npad * ld);
    with_components(c, [&](auto nc) {
        hipLaunchKernelGGL(k_fill_sym_tv<nc()>, dim3(g.P * (g.P + 1) / 2, 1), dim3(256), 0, s, dK, (size_t)0, (int)ld, N, g.P,
                           (const double*)dLwl, dT, (const double*)ws.Gp.p, (const double*)ws.Tau.p, dSig, 1);
    });
    if (g.mode == 0) {
        for (int k = 0; k < c; ++k) {
            predict_tv_taus(tau, k, 1, th.v);
            launch_region_tv_c(s, 1, dK, ld, g.Npad + k * M, N, M, dLwl + (size_t)k * N, 0, dPred + (size_t)k * M, 0, dT, dTp,
                               gp_host(gp, k, 1), th, 0, 0.0);
        }
    } else {
        predict_tv_taus(tau, 0, c, th.v);
        launch_region_tv_c(s, c, dK, ld, g.Npad, N, M, dLwl, (size_t)N, dPred, (size_t)M, dT, dTp, gp_host(gp, 0, c), th, 0, 0.0);
    }
}

// predict_fill_prior under the time-variable kernel: rows and columns both at the prediction dates
static void predict_fill_prior_tv(PredictWs& ws, const PredictShape& g, hipStream_t s, const double* gp, const double* tau, double nugget)
{
    const int c = g.c, M = g.M, Rq_pad = g.Rq_pad;
    double *dS = ws.S, *dPred = ws.Pred;
    const double* dTp = ws.Tpred;
    TauHost th;
    if (g.mode == 0) {
        hipLaunchKernelGGL(k_zero, dim3(1024), dim3(256), 0, s, dS, (size_t)Rq_pad * Rq_pad);
        for (int k = 0; k < c; ++k) {
            predict_tv_taus(tau, k, 1, th.v);
            launch_region_tv_c(s, 1, dS + (size_t)k * M * Rq_pad, (size_t)Rq_pad, k * M, M, M, dPred + (size_t)k * M, 0,
                               dPred + (size_t)k * M, 0, dTp, dTp, gp_host(gp, k, 1), th, 1, 0.0);
        }
    } else {
        if (Rq_pad != g.Rq) hipLaunchKernelGGL(k_zero, dim3(1024), dim3(256), 0, s, dS, (size_t)Rq_pad * Rq_pad);
        predict_tv_taus(tau, 0, c, th.v);
        launch_region_tv_c(s, c, dS, (size_t)Rq_pad, 0, M, M, dPred, (size_t)M, dPred, (size_t)M, dTp, dTp, gp_host(gp, 0, c), th, 1, nugget);
    }
}

// The Sigma download, queued right behind the product on the same stream: into the page-locked caller's array when the
// registration went through (it did its work under the factorisation) -> *direct; otherwise predict_sigma_staged, after
// the stream has drained, goes through the runtime's staging
static int predict_sigma_direct(SigmaPin& pin, PredictWs& ws, const PredictShape& g, hipStream_t s, double* Sigma_out, bool* direct)
{
    *direct = pin.wait();
    if (!*direct) return 0;
    pin.queued_on(s);
    HIP_TRY(hipMemcpy2DAsync(Sigma_out, sizeof(double) * g.Rq, ws.S, sizeof(double) * g.Rq_pad, sizeof(double) * g.Rq, (size_t)g.Rq,
                             hipMemcpyDeviceToHost, s));
    return 0;
}

static int predict_sigma_staged(PredictWs& ws, const PredictShape& g, double* Sigma_out)
{
    HIP_TRY(hipMemcpy2D(Sigma_out, sizeof(double) * g.Rq, ws.S, sizeof(double) * g.Rq_pad, sizeof(double) * g.Rq, g.Rq,
                        hipMemcpyDeviceToHost));
    return 0;
}

// diag(Sigma) = diag(A) - column norms: the prior variances (predict_prior_variance) to the device
static int predict_upload_prior(PredictWs& ws, const PredictShape& g, hipStream_t s, const double* gp, double* h_prior)
{
    HIP_TRY(ws.Var.need(g.Rq_pad));
    HIP_TRY(ws.Prior.need(g.Rq_pad));
    predict_prior_variances(g, gp, h_prior);
    HIP_TRY(hipMemcpyAsync(ws.Prior, h_prior, sizeof(double) * g.Rq, hipMemcpyHostToDevice, s));
    return 0;
}

// events 0 .. 3 of the workspace (call begins, factorisation begins and ends, device work ends) and the host's clock
static void predict_times(PredictWs& ws, std::chrono::steady_clock::time_point t_begin, std::chrono::steady_clock::time_point t_ev0,
                          double flops)
{
    const auto t_end = std::chrono::steady_clock::now();
    float a = 0.f, b = 0.f, cms = 0.f;
    (void)hipEventElapsedTime(&a, ws.ev[0], ws.ev[3]);
    (void)hipEventElapsedTime(&b, ws.ev[1], ws.ev[2]);
    (void)hipEventElapsedTime(&cms, ws.ev[2], ws.ev[3]);
    PredictTimes& t = ws.times;
    t.device_ms = a;
    t.factor_ms = b;
    t.sigma_ms = cms;
    t.total_ms = std::chrono::duration<double, std::milli>(t_end - t_begin).count();
    // what the download adds to the call beyond the device work (the groups travel while later ones are computed)
    const double pre_ms = std::chrono::duration<double, std::milli>(t_ev0 - t_begin).count();
    t.download_ms = t.total_ms - pre_ms - (double)a > 0.0 ? t.total_ms - pre_ms - (double)a : 0.0;
    t.flops = flops;
}

// the panel update of a staged sweep whose block row has nothing but its own `blocks` tile columns to update
static auto plain_update(hipStream_t s, double* A, int ld, int k0, int blocks)
{
    return [=] { hipLaunchKernelGGL(k_panel_update, dim3(blocks, 1), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, A, (size_t)0, ld, k0); };
}

// The left-looking staged sweep of an Npad x (Npad + 128 Mt) augmented matrix [B | appended columns], nothing booked (the
// plain predict and the calibration have no handle): afterwards the appended columns hold U^-T (appended) and dR holds
// z = U^-T r.  (What the sweep reports is in g_err, the error string every caller hands on.)
static int staged_augmented(hipStream_t st, double* dK, int ld, int P, int Mt, double* dW, double* dR, int Npad, MatAcc* dAcc)
{
    for (int p = 0; p < P; ++p) {
        const int k0 = p * NB, ntile = P - p + Mt;
        const auto update = plain_update(st, dK, ld, k0, ntile);
        const StagedRow row{dK, 0, ld, dR, Npad, dAcc, dW, (size_t)NB * NB, ntile - 1};
        if (int rc = staged_row(nullptr, st, row, 1, k0, p > 0 ? &update : nullptr, 0.0)) return rc;
    }
    return 0;
}

// ---- the plain call ------------------------------------------------------------------------------------------------------
// The factorisation of [B | Cx^T] as ONE launch of the persistent dependency-graph kernel with the appended columns as
// extra column tiles (k_chol_dag<C, true>: the cross-covariances are evaluated on the fly like B itself).  With fused_sigma
// the tiles of Sigma = A - W^T W, the Schur complement of the appended columns, are tasks of the same launch (DAG_SCHUR):
// left-looking updates that need no critical path and fill the workgroups the factorisation's row-to-row chain leaves idle.
static int predict_factor_dag(PredictWs& ws, const PredictShape& g, const PredictStaging& hs, hipStream_t st, const double* lwl_pred,
                              const double* gp, const double* dFl, const double* dSig, bool fused_sigma)
{
    const int c = g.c, P = g.P, Mt = g.Mt, Rq_pad = g.Rq_pad, Ms = fused_sigma ? Rq_pad / NB : 0;
    double *h_colx = ws.hSmall.p + hs.colx, *h_rowx = ws.hSmall.p + hs.rowx, *h_diag = ws.hSmall.p + hs.diag;
    predict_abscissae(g, lwl_pred, h_colx, fused_sigma ? h_rowx : nullptr);
    const int scheme = dag_env_scheme();
    const int workers = dag_batch_workers(std::vector<int>(1, P), Mt, ws.n_cus > 0 ? ws.n_cus : ws.workers, ws.workers);
    if (ws.plan_P != P || ws.plan_Mt != Mt || ws.plan_workers != workers || ws.plan_scheme != scheme || ws.plan_Ms != Ms) {
        const DagPlan plan = dag_build_tasks(1, P, workers, scheme, Mt, Ms);
        HIP_TRY(hipStreamSynchronize(st));
        ws.plan_P = -1;      // (until the workspace holds the new list)
        HIP_TRY(ws.dag.load(plan, 1));
        ws.plan_P = P;
        ws.plan_Mt = Mt;
        ws.plan_workers = workers;
        ws.plan_scheme = scheme;
        ws.plan_Ms = Ms;
    }
    const DagWorkspace& dag = ws.dag;
    HIP_TRY(ws.Colx.need((size_t)c * Rq_pad));
    HIP_TRY(ws.Mat.need(1));
    HIP_TRY(hipMemcpyAsync(ws.Colx, h_colx, sizeof(double) * (size_t)c * Rq_pad, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(dag.ctl, 0, dag.ctl_bytes, st));
    HIP_TRY(hipMemsetAsync(ws.W, 0, sizeof(double) * 2 * NB * NB, st));  // the strictly upper part of W stays zero
    HIP_TRY(hipMemsetAsync(ws.W.p + WT_THIRD, 0, sizeof(double) * NB * NB, st));   // (scheme 0's third tile)
    hipLaunchKernelGGL(k_init_rhs, dim3((g.Npad + 255) / 256, 1), dim3(256), 0, st, ws.R.p, g.Npad, g.N, dFl, g.offset, ws.Acc.p);
    DagAug aug{P + Mt, g.Rq, Rq_pad, ws.Colx, nullptr, nullptr, nullptr, 0};
    if (fused_sigma) {
        predict_diag(g, gp, h_diag);
        HIP_TRY(ws.Rowx.need((size_t)c * Rq_pad));
        HIP_TRY(ws.Diag.need(Rq_pad));
        HIP_TRY(ws.S.need((size_t)Rq_pad * Rq_pad));
        HIP_TRY(hipMemcpyAsync(ws.Rowx, h_rowx, sizeof(double) * (size_t)c * Rq_pad, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ws.Diag, h_diag, sizeof(double) * Rq_pad, hipMemcpyHostToDevice, st));
        aug = DagAug{P + Mt, g.Rq, Rq_pad, ws.Colx, ws.Rowx, ws.Diag, ws.S, (size_t)Rq_pad};
    }
    DagMat hm{};
    hm.K = ws.K; hm.R = ws.R; hm.Wt = ws.W; hm.lw = ws.Lwl; hm.gp = ws.Gp; hm.sigma = dSig; hm.acc = ws.Acc;
    hm.N = g.N; hm.Npad = g.Npad; hm.P = P; hm.ld = (int)g.ld;
    // a kernel argument would do, but the records of the likelihood path live in memory: same code path
    HIP_TRY(hipMemcpyAsync(ws.Mat, &hm, sizeof(DagMat), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // hm is a stack object; the staging copies are tiny
    HIP_TRY(hipEventRecord(ws.ev[1], st));
    // debug: per-task stamps of this launch, written with the task list to the file PSOAP_PREDICT_TLOG names
    unsigned long long* tlog_ = nullptr;
    if (getenv("PSOAP_PREDICT_TLOG")) {
        HIP_TRY(ws.Tlog.need((size_t)dag.n_tasks * 8));
        HIP_TRY(hipMemsetAsync(ws.Tlog, 0, sizeof(unsigned long long) * dag.n_tasks * 8, st));
        tlog_ = ws.Tlog.p;
    }
    // (the workers are clamped to two per compute unit already: predict_ws_init)
    const DagShape sh = dag_shape(dag, workers, ws.n_cus);
    dag_launch<true, false>(c, sh.lat, sh.wide, sh.grid, st, ws.Mat, dag.tasks, dag.queues, dag.flags(), dag.arrive(),
                            dag.ws, dag.dag_ctl(), tlog_, aug, StreamArgs{});
    HIP_TRY(hipGetLastError());
    return 0;
}

// The same by the staged sweep, one block row after the other: [B | Cx^T] filled first.  The transposed-mean variant
// (covariance.py:294) needs a block whose ROW abscissae are the prediction grid and always comes here.
static int predict_factor_staged(PredictWs& ws, const PredictShape& g, hipStream_t st, const double* gp, const double* dFl,
                                 const double* dSig)
{
    HIP_TRY(hipEventRecord(ws.ev[1], st));
    predict_fill(ws, g, st, g.ld, gp, dSig);
    if (g.transposed_mean)  // rows indexed by the prediction grid, columns by the data grid (M == N)
        launch_region_c(st, g.c, ws.K, g.ld, g.Npad + g.Rq_pad, g.N, g.N, ws.Pred, (size_t)g.M, ws.Lwl, (size_t)g.N, gp_host(gp, 0, g.c), 0, 0.0);
    hipLaunchKernelGGL(k_init_rhs, dim3((g.Npad + 255) / 256, 1), dim3(256), 0, st, ws.R.p, g.Npad, g.N, dFl, g.offset, ws.Acc.p);
    HIP_TRY(hipGetLastError());
    return staged_augmented(st, ws.K, (int)g.ld, g.P, g.Mt, ws.W, ws.R, g.Npad, ws.Acc);
}

// when the persistent launch has drained: a timed-out wait is an error; PSOAP_PREDICT_TLOG's file; 3 when a workgroup moved
// between compute units under one of the launch's tasks (dag_where) -- the outputs are not handed out, the caller runs the
// call again
static int predict_dag_verdict(PredictWs& ws, const PredictShape& g)
{
    unsigned int dag_err[6] = {0, 0, 0, 0, 0, 0};      // DagCtl::error, pad[0..4]
    HIP_TRY(hipMemcpy(dag_err, ws.dag.ctl.p + offsetof(DagCtl, error), sizeof(dag_err), hipMemcpyDeviceToHost));
    if (dag_err[0] != 0) {
        g_err = "predict: dependency wait timed out inside the persistent kernel";
        return 1;
    }
    if (const char* tpath = getenv("PSOAP_PREDICT_TLOG")) {
        const size_t nt = ws.dag.n_tasks;
        std::vector<unsigned long long> hl(nt * 8);
        std::vector<DagTask> tasks(nt);
        HIP_TRY(hipMemcpy(hl.data(), ws.Tlog.p, sizeof(unsigned long long) * hl.size(), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(tasks.data(), ws.dag.tasks.p, sizeof(DagTask) * nt, hipMemcpyDeviceToHost));
        if (FILE* fh = fopen(tpath, "wb")) {
            const unsigned long long hdr[4] = {(unsigned long long)nt, (unsigned long long)g.P, (unsigned long long)g.Mt,
                                               (unsigned long long)ws.dag.scheme};
            fwrite(hdr, sizeof hdr, 1, fh);
            fwrite(tasks.data(), sizeof(DagTask), nt, fh);
            fwrite(hl.data(), sizeof(unsigned long long), hl.size(), fh);
            fclose(fh);
        }
    }
    if (dag_err[4] != 0) {
        g_err = "predict: the persistent launch was disturbed by the device's scheduler";
        return 3;
    }
    return 0;
}

// dFl_res / dSig_res: the data and noise vectors already resident on the device (a chunk handle's), or nullptr -> fl /
// sigma are uploaded into the workspace.  var_out (optional): diag(Sigma) alone -- R doubles instead of R^2, and no N R^2
// product.  force_staged: several processes share the device and the persistent launch is not to be used, or was disturbed
// (predict_settled).  keep_sigma: Sigma is formed in the workspace as with Sigma_out, by the same launches, and stays there --
// no download (the mixture moments fold it on the device).  A matrix that is not positive definite: *status = 1 and the values
// as they came out.
static int predict_run(PredictWs& ws, int mode, int c, int N, int M, const double* lwl, const double* fl, const double* sigma,
                       const double* dFl_res, const double* dSig_res, const double* lwl_pred, const double* mu_c, const double* gp,
                       double* mu_out, double* Sigma_out, int* status, double* var_out = nullptr, bool force_staged = false,
                       bool keep_sigma = false)
{
    const auto t_begin = std::chrono::steady_clock::now();
    SigmaPin pin;         // declared first: its destructor joins the helper thread and drops the registration on every return path
    PredictShape g;
    if (const char* why = predict_shape(mode, c, N, M, mu_c[0], g)) FAIL(why);
    const bool use_dag = !force_staged && g.dag_ok;
    const bool want_S = Sigma_out || keep_sigma;
    // PSOAP_PREDICT_FUSED=0: Sigma by the separate product (k_syrk_sub_sym) also behind the persistent launch
    const char* env_fused = getenv("PSOAP_PREDICT_FUSED");
    const bool fused_sigma = use_dag && want_S && !(env_fused && atoi(env_fused) == 0);
    const int Npad = g.Npad, Rq = g.Rq, Rq_pad = g.Rq_pad, nslab = g.nslab;
    const PredictStaging hs = predict_staging(Rq_pad, sizeof(MatAcc), c);
    if (int rc = predict_stream(ws)) return rc;
    if (Sigma_out) {
        int dev_now = 0;
        HIP_TRY(hipGetDevice(&dev_now));
        pin.start(Sigma_out, sizeof(double) * (size_t)Rq * Rq, dev_now);
    }
    hipStream_t st = ws.stream;
    if (int rc = predict_need(ws, g, g.ld, hs.total)) return rc;
    double *h_mu = ws.hSmall.p + hs.mu, *h_var = ws.hSmall.p + hs.var;
    MatAcc* h_acc = reinterpret_cast<MatAcc*>(ws.hSmall.p + hs.acc);
    double *dK = ws.K, *dPart = ws.Part;
    MatAcc* dAcc = ws.Acc;
    const auto t_ev0 = std::chrono::steady_clock::now();
    HIP_TRY(hipEventRecord(ws.ev[0], st));
    if (int rc = predict_upload(ws, g, st, lwl, lwl_pred, gp, mu_c, dFl_res ? nullptr : fl, sigma, ws.hSmall.p + hs.m0)) return rc;
    const double *dFl = dFl_res ? dFl_res : ws.Fl.p, *dSig = dSig_res ? dSig_res : ws.Sig.p;
    if (int rc = use_dag ? predict_factor_dag(ws, g, hs, st, lwl_pred, gp, dFl, dSig, fused_sigma)
                         : predict_factor_staged(ws, g, st, gp, dFl, dSig)) return rc;
    HIP_TRY(hipEventRecord(ws.ev[2], st));

    // mean: m0 + W^T z  (W is the block that matches the reference's orientation for this mode); the records' total
    const double* Wmean = dK + Npad + (g.transposed_mean ? Rq_pad : 0);
    hipLaunchKernelGGL(k_gemv_t_partial, dim3((Rq + 127) / 128, nslab), dim3(256), 0, st, Wmean, g.ld, Npad, Rq, ws.R.p, dPart);
    hipLaunchKernelGGL(k_gemv_finish, dim3((Rq + 255) / 256), dim3(256), 0, st, dPart, nslab, Rq, ws.M0.p, ws.Mu.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_mu, ws.Mu, sizeof(double) * Rq, hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(k_acc_total, dim3(1), dim3(1), 0, st, dAcc, g.P, dAcc + ACC_ROWS);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_acc, dAcc + ACC_ROWS, sizeof(MatAcc), hipMemcpyDeviceToHost, st));

    bool sigma_direct = false;
    if (want_S) {
        const int St = Rq_pad / NB;
        HIP_TRY(ws.S.need((size_t)Rq_pad * Rq_pad));
        if (!fused_sigma) {
            predict_fill_prior(ws, g, st, gp, (mode == 1 && c == 2) ? 1e-8 : 0.0);
            HIP_TRY(hipGetLastError());
            // Sigma = A - W^T W: one launch -- every tile is one K = Npad loop and all of them fit the device at once, so they
            // all finish together (launching tile rows one after the other serialises them: measured 2.2 -> 10.5 ms)
            hipLaunchKernelGGL(k_syrk_sub_sym, dim3(St * (St + 1) / 2), dim3(GEMM_THREADS), GEMM_LDS_BYTES, st, dK + Npad, g.ld,
                               Npad, ws.S.p, (size_t)Rq_pad, St, 0);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(ws.ev[3], st));           // the device work of the call ends here
        if (Sigma_out)
            if (int rc = predict_sigma_direct(pin, ws, g, st, Sigma_out, &sigma_direct)) return rc;
    }
    if (var_out) {
        if (int rc = predict_upload_prior(ws, g, st, gp, ws.hSmall.p + hs.prior)) return rc;
        hipLaunchKernelGGL(k_colnorm_partial, dim3((Rq + 127) / 128, nslab), dim3(256), 0, st, dK + Npad, g.ld, Npad, Rq, dPart);
        hipLaunchKernelGGL(k_var_finish, dim3((Rq + 255) / 256), dim3(256), 0, st, dPart, nslab, Rq, ws.Prior.p, ws.Var.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_var, ws.Var, sizeof(double) * Rq, hipMemcpyDeviceToHost, st));
    }
    if (!want_S) HIP_TRY(hipEventRecord(ws.ev[3], st));
    HIP_TRY(hipStreamSynchronize(st));
    if (use_dag)
        if (int rc = predict_dag_verdict(ws, g)) return rc;      // (pin's destructor drops the registration)
    if (Sigma_out && !sigma_direct)
        if (int rc = predict_sigma_staged(ws, g, Sigma_out)) return rc;
    pin.release();
    *status = (h_acc->info != 0.0) ? 1 : 0;
    memcpy(mu_out, h_mu, sizeof(double) * Rq);
    if (var_out) memcpy(var_out, h_var, sizeof(double) * Rq);
    predict_times(ws, t_begin, t_ev0, predict_flops(Npad, Rq_pad, want_S, var_out != nullptr));
    return 0;
}

// ---- the call under the time-variable kernel ---------------------------------------------------------------------------------
// psoap_chunk_predict_tv / _var: the staged route of predict_run with the time-variable fills, on the handle's first stream
// and booked like the other analysis paths (marg_predict_run's shape without its Gram half).  The launches behind the fill
// are predict_factor_staged's and predict_run's, kernel for kernel and grid for grid: with every tau = +inf the outputs have
// the bits of the plain call on the staged route.  The persistent launch evaluates the static covariance in its epilogue and
// is not used.  (The caller has run predict_tv_check.)
static int predict_tv_run(psoap_chunk* h, int mode, int c, int M, const double* lwl, const double* lwl_pred, const double* t_pred,
                          const double* mu_c, const double* gp, const double* tau, double* mu_out, double* Sigma_out, double* var_out,
                          int* status_out)
{
    const auto t_begin = std::chrono::steady_clock::now();
    SigmaPin pin;         // declared first, as in predict_run: its destructor drops the registration on every return path
    h->sigma.valid = false;
    DEVICE_SCOPE(h->device);
    if (int rc = enter_device(h->device)) return rc;
    PredictWs& ws = predict_ws_of(h);
    PredictShape g;
    if (const char* why = predict_shape(mode, c, h->N, M, mu_c[0], g)) FAIL(why);
    const int N = h->N, Npad = g.Npad, P = g.P, Mt = g.Mt, Rq = g.Rq, Rq_pad = g.Rq_pad, nslab = g.nslab, ld = (int)g.ld;
    const PredictStaging hs = predict_staging(Rq_pad, sizeof(MatAcc), 0);
    if (int rc = predict_stream(ws)) return rc;
    if (Sigma_out) pin.start(Sigma_out, sizeof(double) * (size_t)Rq * Rq, h->device);
    hipStream_t s = h->streams[0];
    if (int rc = predict_need(ws, g, g.ld, hs.total)) return rc;
    HIP_TRY(ws.Tpred.need(M));
    HIP_TRY(ws.Tau.need(3));
    double *h_mu = ws.hSmall.p + hs.mu, *h_var = ws.hSmall.p + hs.var;
    MatAcc* h_acc = reinterpret_cast<MatAcc*>(ws.hSmall.p + hs.acc);
    double* dK = ws.K;
    const double* W = dK + Npad;
    h->recs.clear();
    const auto t_ev0 = std::chrono::steady_clock::now();
    HIP_TRY(hipEventRecord(ws.ev[0], s));
    if (int rc = predict_upload(ws, g, s, lwl, lwl_pred, gp, mu_c, nullptr, nullptr, ws.hSmall.p + hs.m0)) return rc;
    HIP_TRY(hipMemcpyAsync(ws.Tpred, t_pred, sizeof(double) * M, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ws.Tau, tau, sizeof(double) * c, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(ws.ev[1], s));
    if (int rc = prof_launch(h, s, PSOAP_K_FILL, 0.0, 8.0 * Npad * (double)g.ld,
                             [&] { predict_fill_tv(ws, g, s, g.ld, gp, tau, h->dTimes.p, h->dSigma.p); })) return rc;
    if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
            hipLaunchKernelGGL(k_init_rhs, dim3((Npad + 255) / 256, 1), dim3(256), 0, s, ws.R.p, Npad, N, h->dFl.p, g.offset, ws.Acc.p);
        })) return rc;
    for (int p = 0; p < P; ++p) {      // (staged_augmented's rows, booked)
        const int k0 = p * NB, ntile = P - p + Mt;
        const auto update = plain_update(s, dK, ld, k0, ntile);
        const StagedRow row{dK, 0, ld, ws.R.p, Npad, ws.Acc.p, ws.W.p, (size_t)NB * NB, ntile - 1};
        if (int rc = staged_row(h, s, row, 1, k0, p > 0 ? &update : nullptr, TILE_FLOPS * p * ntile)) return rc;
    }
    HIP_TRY(hipEventRecord(ws.ev[2], s));
    // mean: m0 + W^T z; the records' total
    if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
            hipLaunchKernelGGL(k_gemv_t_partial, dim3((Rq + 127) / 128, nslab), dim3(256), 0, s, W, g.ld, Npad, Rq, (const double*)ws.R.p,
                               ws.Part.p);
            hipLaunchKernelGGL(k_gemv_finish, dim3((Rq + 255) / 256), dim3(256), 0, s, (const double*)ws.Part.p, nslab, Rq,
                               (const double*)ws.M0.p, ws.Mu.p);
            hipLaunchKernelGGL(k_acc_total, dim3(1), dim3(1), 0, s, (const MatAcc*)ws.Acc.p, P, ws.Acc.p + ACC_ROWS);
        })) return rc;
    HIP_TRY(hipMemcpyAsync(h_mu, ws.Mu, sizeof(double) * Rq, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_acc, ws.Acc.p + ACC_ROWS, sizeof(MatAcc), hipMemcpyDeviceToHost, s));
    bool sigma_direct = false;
    if (Sigma_out) {
        const int St = Rq_pad / NB;
        HIP_TRY(ws.S.need((size_t)Rq_pad * Rq_pad));
        // Sigma = A - W^T W over the prior at the prediction dates: every upper tile in one launch, as predict_run
        if (int rc = prof_launch(h, s, PSOAP_K_GRAD, TILE_FLOPS * (St * (St + 1) / 2) * P, 0.0, [&] {
                predict_fill_prior_tv(ws, g, s, gp, tau, (mode == 1) ? 1e-8 : 0.0);
                hipLaunchKernelGGL(k_syrk_sub_sym, dim3(St * (St + 1) / 2), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, W, g.ld, Npad, ws.S.p,
                                   (size_t)Rq_pad, St, 0);
            })) return rc;
        HIP_TRY(hipEventRecord(ws.ev[3], s));
        if (int rc = predict_sigma_direct(pin, ws, g, s, Sigma_out, &sigma_direct)) return rc;
    }
    if (var_out) {
        // (the prior variances are the static ones: dt = 0 on the diagonal)
        if (int rc = predict_upload_prior(ws, g, s, gp, ws.hSmall.p + hs.prior)) return rc;
        if (int rc = prof_launch(h, s, PSOAP_K_MISC, 0.0, 0.0, [&] {
                hipLaunchKernelGGL(k_colnorm_partial, dim3((Rq + 127) / 128, nslab), dim3(256), 0, s, W, g.ld, Npad, Rq, ws.Part.p);
                hipLaunchKernelGGL(k_var_finish, dim3((Rq + 255) / 256), dim3(256), 0, s, (const double*)ws.Part.p, nslab, Rq,
                                   (const double*)ws.Prior.p, ws.Var.p);
            })) return rc;
        HIP_TRY(hipMemcpyAsync(h_var, ws.Var, sizeof(double) * Rq, hipMemcpyDeviceToHost, s));
    }
    if (!Sigma_out) HIP_TRY(hipEventRecord(ws.ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    if (Sigma_out && !sigma_direct)
        if (int rc = predict_sigma_staged(ws, g, Sigma_out)) return rc;
    pin.release();
    if (collect_timings(h)) return 1;
    // K not positive definite: status 1 and NaN in every output (the marginal call's convention)
    const bool bad = h_acc->info != 0.0;
    if (status_out) *status_out = bad ? 1 : 0;
    for (int q = 0; q < Rq; ++q) mu_out[q] = bad ? NAN : h_mu[q];
    if (var_out)
        for (int q = 0; q < Rq; ++q) var_out[q] = bad ? NAN : h_var[q];
    if (Sigma_out && bad)
        for (size_t k = 0; k < (size_t)Rq * Rq; ++k) Sigma_out[k] = NAN;
    if (Sigma_out && !bad) h->sigma = psoap_chunk::SigmaRecord{true, Rq, mode};
    predict_times(ws, t_begin, t_ev0, predict_tv_flops(Npad, Rq_pad, Sigma_out != nullptr, var_out != nullptr));
    return 0;
}
