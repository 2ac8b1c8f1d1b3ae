// dag_launch.hpp -- host side of the persistent kernel's launches (k_chol_dag, dag_kernel.hpp): the device copy of a task
// list (dag_plan.hpp builds it) with its control region (DagWorkspace), the launch shape, and the one list of built
// instantiations that the launcher dispatches over and the LDS-attribute pass walks.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <vector>

#include "dag_kernel.hpp"
#include "dag_plan.hpp"

namespace psoap {

// ---- one task list on the device ------------------------------------------------------------------
// The plan's tasks, the split-K partial tiles, and the control region: DagCtl, MatFlags[n_mats] and the arrival counters --
// all of it zeroed by one memset of ctl_bytes before every launch.  Grow-only; load() only while no launch reads it.
struct DagWorkspace {
    Grow<DagTask> tasks;
    Grow<double> ws;
    Grow<unsigned char> ctl;
    size_t arrive_off = 0, ctl_bytes = 0;
    DagQueues queues{};
    int scheme = 0;
    unsigned int n_tasks = 0, n_slots = 0;

    // (resident: the same list in device memory already -- a cached one; it is copied on `s`, behind the launches queued
    // there, and the host waits for them only where a buffer has to grow)
    hipError_t load(const DagPlan& plan, size_t n_mats, const DagTask* resident = nullptr, hipStream_t s = nullptr)
    {
        const size_t nt = plan.tasks.size();
        // (the throughput kernels read bits 24.. of a final's ctr as its block row's shortfall: dag_build_tasks)
        if (plan.n_ctrs > DAG_CTR_MASK) return hipErrorInvalidValue;
        arrive_off = sizeof(DagCtl) + sizeof(MatFlags) * n_mats;
        ctl_bytes = arrive_off + sizeof(int) * ((size_t)plan.n_ctrs + 4);
        hipError_t e = hipSuccess;
        const size_t ws_count = (size_t)NB * NB * ((size_t)plan.n_slots + 1);
        if (resident && (ctl_bytes > ctl.cap || nt > tasks.cap || ws_count > ws.cap || !ctl.p || !tasks.p || !ws.p))
            e = hipStreamSynchronize(s);
        if (e == hipSuccess) e = ctl.need(ctl_bytes);
        if (e == hipSuccess) e = tasks.need(nt);
        if (e == hipSuccess) e = ws.need((size_t)NB * NB * ((size_t)plan.n_slots + 1));
        if (e == hipSuccess)
            e = resident ? hipMemcpyAsync(tasks, resident, sizeof(DagTask) * nt, hipMemcpyDeviceToDevice, s)
                         : hipMemcpy(tasks, plan.tasks.data(), sizeof(DagTask) * nt, hipMemcpyHostToDevice);
        queues = plan.queues;
        scheme = plan.scheme;
        n_tasks = (unsigned int)nt;
        n_slots = plan.n_slots;
        return e;
    }
    DagCtl* dag_ctl() const { return reinterpret_cast<DagCtl*>(ctl.p); }
    MatFlags* flags() const { return reinterpret_cast<MatFlags*>(ctl.p + sizeof(DagCtl)); }
    int* arrive() const { return reinterpret_cast<int*>(ctl.p + arrive_off); }
};

// Grid and form of a launch of a task list: at most one workgroup per task, `workers` of them, the LAT kernels at most two
// per compute unit.  Where that leaves at most one workgroup per compute unit (single evaluations, predict:
// dag_pick_workers) the LAT kernels compiled for one wave per SIMD -- 512 registers per lane, nothing of the chain phases in
// scratch memory; PSOAP_DAG_WIDE=0 forbids them (read at every launch).
struct DagShape {
    int grid;
    bool lat, wide;
};
inline DagShape dag_shape(const DagWorkspace& w, int workers, int n_cus)
{
    DagShape s;
    s.lat = w.scheme >= 1;
    s.grid = (long long)w.n_tasks < workers ? (int)w.n_tasks : workers;
    if (s.lat && n_cus > 0) s.grid = dag_two_per_cu(s.grid, n_cus);
    s.wide = s.lat && n_cus > 0 && s.grid <= n_cus && !(getenv("PSOAP_DAG_WIDE") && getenv("PSOAP_DAG_WIDE")[0] == '0');
    return s;
}

// ---- the built instantiations -----------------------------------------------------------------------
// Every k_chol_dag the library launches comes from this list: dag_launch dispatches over it and dag_set_lds gives each
// member its LDS attribute, so no form is launched without one.  C in 1..3 x {throughput, LAT, LAT wide}, for the
// likelihood (AUG = false) and predict (AUG = true); the stream (STREAM = true) has no wide form.
// Waves per SIMD, the one rule: wide 1, every other form 2.
enum DagForm { DAG_TP, DAG_LAT, DAG_WIDE };

template <int C_, bool AUG, bool STREAM, int FORM>
struct DagKernel {
    static constexpr int C = C_;
    static constexpr bool LAT = FORM != DAG_TP;
    static constexpr int WPE = FORM == DAG_WIDE ? 1 : 2;
    // the member's place in the list (include/psoap_gp.h: psoap_dag_form_launches)
    static constexpr int INDEX = STREAM ? 18 + 2 * (C - 1) + (LAT ? 1 : 0) : 9 * (AUG ? 1 : 0) + 3 * (C - 1) + FORM;
    static const void* fn() { return reinterpret_cast<const void*>(k_chol_dag<C, AUG, LAT, STREAM, WPE>); }
};

template <int C, bool AUG, bool STREAM, class F>
inline void dag_visit_form(DagForm form, F& f)
{
    if constexpr (!STREAM) {
        if (form == DAG_WIDE) return f(DagKernel<C, AUG, STREAM, DAG_WIDE>{});
    }
    if (form != DAG_TP) f(DagKernel<C, AUG, STREAM, DAG_LAT>{});
    else f(DagKernel<C, AUG, STREAM, DAG_TP>{});
}
// f(DagKernel<C, AUG, STREAM, form>{}) -- the list's member for the runtime choice (C, form)
template <bool AUG, bool STREAM, class F>
inline void dag_visit(int C, DagForm form, F&& f)
{
    if (C == 1) dag_visit_form<1, AUG, STREAM>(form, f);
    else if (C == 2) dag_visit_form<2, AUG, STREAM>(form, f);
    else dag_visit_form<3, AUG, STREAM>(form, f);
}

// the LDS attribute of every member (per device: hipFuncSetAttribute applies to the current one)
template <bool AUG, bool STREAM>
inline hipError_t dag_set_lds()
{
    hipError_t e = hipSuccess;
    for (int C = 1; C <= 3; ++C)
        for (int form = DAG_TP; form <= (STREAM ? DAG_LAT : DAG_WIDE); ++form)
            dag_visit<AUG, STREAM>(C, (DagForm)form, [&](auto k) {
                if (e == hipSuccess)
                    e = hipFuncSetAttribute(k.fn(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEMM_LDS_BYTES);
            });
    return e;
}

// launches of every member so far, process-wide, by DagKernel::INDEX (psoap_dag_form_launches: the tests read which form ran)
constexpr int DAG_N_FORMS = 24;
static_assert(DAG_N_FORMS == 2 * 3 * (DAG_WIDE + 1) + 3 * (DAG_LAT + 1), "a form was added to the list: give it an index");
inline std::atomic<long long>* dag_form_launches()
{
    static std::atomic<long long> n[DAG_N_FORMS];
    return n;
}

// One launch of the persistent kernel: the member for (C, lat, wide) on `grid` workgroups
template <bool AUG, bool STREAM>
inline void dag_launch(int C, bool lat, bool wide, int grid, hipStream_t s, const DagMat* mats, const DagTask* tasks,
                       DagQueues queues, MatFlags* flags, int* arrive, double* wspace, DagCtl* ctl,
                       unsigned long long* tlog, DagAug aug, StreamArgs st)
{
    dag_visit<AUG, STREAM>(C, wide ? DAG_WIDE : lat ? DAG_LAT : DAG_TP, [&](auto k) {
        using K = decltype(k);
        hipLaunchKernelGGL((k_chol_dag<K::C, AUG, K::LAT, STREAM, K::WPE>), dim3(grid), dim3(GEMM_THREADS), GEMM_LDS_BYTES,
                           s, mats, tasks, queues, flags, arrive, wspace, ctl, tlog, aug, st);
        dag_form_launches()[K::INDEX] += 1;
    });
}

}  // namespace psoap
