// timevar_sampling_host_check.cpp -- the pure-host refusals of the time scales on the batch route and of lnprob(p) under the
// time-variable kernel (psoap_amd/csrc/marg_grad_plan.hpp: batch_tau_check, what psoap_batch_set_tau asks before any work, and
// lnprob_tv_check, what psoap_chunk_lnprob_tv_grad and psoap_chunk_lnprob_marg_tv_grad ask before the orbits are looked at)
// built by a host compiler alone, with sanitizers (tests/test_timevar_sampling_host.py).  One line per case on stdout -- the
// refusal, or "ok" -- for the test to compare with what it expects, and a non-zero exit status when an invariant does not hold.
#include <stdio.h>
#include <string.h>

#include "../../psoap_amd/csrc/marg_grad_plan.hpp"
#include "../../psoap_amd/csrc/predict_plan.hpp"

using namespace psoap;

static int failures = 0;

#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// psoap_batch_set_tau as it is accepted: the array there, B = 9 and c = 2 as the pending upload has them, times set, no open
// stream, no baseline
struct TauCall {
    bool array;
    int B, c;
    bool pending;
    int pend_B, pend_c;
    bool have_times, open_stream, have_baseline;
};
static TauCall good() { return TauCall{true, 9, 2, true, 9, 2, true, false, false}; }
static const char* check(const TauCall& a)
{
    return batch_tau_check(a.array, a.B, a.c, a.pending, a.pend_B, a.pend_c, a.have_times, a.open_stream, a.have_baseline);
}
static void show(const char* name, const TauCall& a)
{
    const char* why = check(a);
    printf("set_tau %s : %s\n", name, why ? why : "ok");
}

// the lnprob entries as they are accepted: the arrays and the whole gradient, B = 3, grid, dates and times set, no open stream
struct LnprobCall {
    bool arrays, grad_gp, grad_orb, grad_tau, grad_rest;
    int B;
    bool have_grid, have_times, open_stream;
};
static LnprobCall lgood() { return LnprobCall{true, true, true, true, true, 3, true, true, false}; }
static const char* lcheck(const LnprobCall& a)
{
    return lnprob_tv_check(a.arrays, a.grad_gp, a.grad_orb, a.grad_tau, a.grad_rest, a.B, a.have_grid, a.have_times, a.open_stream);
}
static void lshow(const char* name, const LnprobCall& a)
{
    const char* why = lcheck(a);
    printf("lnprob %s : %s\n", name, why ? why : "ok");
}

int main()
{
    TauCall a = good();
    show("ok", a);
    a = good(), a.B = a.pend_B = 1, a.c = a.pend_c = 1;
    show("ok-B1-c1", a);
    a = good(), a.c = a.pend_c = 3;
    show("ok-c3", a);
    a = good(), a.array = false;
    show("no-array", a);
    a = good(), a.c = 0;
    show("c0", a);
    a = good(), a.c = 4;
    show("c4", a);
    a = good(), a.B = 0;
    show("B0", a);
    a = good(), a.pending = false, a.pend_B = a.pend_c = 0;
    show("no-pending", a);
    a = good(), a.B = 8;
    show("B-mismatch", a);
    a = good(), a.c = 3;
    show("c-mismatch", a);
    a = good(), a.have_times = false;
    show("no-times", a);
    a = good(), a.open_stream = true;
    show("open-stream", a);
    a = good(), a.have_baseline = true;
    show("baseline", a);

    // the order of the refusals: everything wrong at once, then mended one by one
    TauCall w{false, 0, 0, false, 0, 0, false, true, true};
    EXPECT(!strcmp(check(w), "bad arguments"));
    w.array = true;
    EXPECT(strstr(check(w), "number of components"));
    w.c = 2;
    EXPECT(strstr(check(w), "B must be at least 1"));
    w.B = 9;
    EXPECT(strstr(check(w), "set_times"));
    w.have_times = true;
    EXPECT(strstr(check(w), "open stream"));
    w.open_stream = false;
    EXPECT(strstr(check(w), "psoap_chunk_lnlike_marg_tv"));
    w.have_baseline = false;
    EXPECT(strstr(check(w), "no upload is pending"));
    w.pending = true, w.pend_B = 8, w.pend_c = 2;
    EXPECT(strstr(check(w), "those of the pending upload"));
    w.pend_B = 9, w.pend_c = 3;
    EXPECT(strstr(check(w), "those of the pending upload"));
    w.pend_c = 2;
    EXPECT(check(w) == nullptr);
    // the words: times and stream as the time-variable entries say them (predict_plan.hpp)
    TauCall s = good();
    s.have_times = false;
    EXPECT(!strcmp(check(s), tv_analysis_check(2, true, false, false, false)));
    s = good(), s.open_stream = true;
    EXPECT(!strcmp(check(s), tv_analysis_check(2, true, true, true, false)));
    s = good(), s.c = 0;
    EXPECT(!strcmp(check(s), tv_analysis_check(0, true, true, false, false)));
    // a baseline is refused, in words of its own: where the value under one is to be had
    s = good(), s.have_baseline = true;
    EXPECT(strcmp(check(s), tv_analysis_check(2, true, true, false, true)) != 0 && strstr(check(s), "psoap_chunk_set_baseline"));

    LnprobCall l = lgood();
    lshow("ok", l);
    l = lgood(), l.grad_rest = false;
    lshow("ok-no-rest", l);
    l = lgood(), l.grad_gp = l.grad_orb = l.grad_tau = l.grad_rest = false;
    lshow("value-only", l);
    l = lgood(), l.arrays = false;
    lshow("no-arrays", l);
    l = lgood(), l.grad_gp = false;
    lshow("orb-and-tau-without-gp", l);
    l = lgood(), l.grad_gp = l.grad_orb = l.grad_tau = false;
    lshow("rest-without-gp", l);
    l = lgood(), l.grad_tau = false;
    lshow("gp-without-tau", l);
    l = lgood(), l.grad_orb = false;
    lshow("gp-without-orb", l);
    l = lgood(), l.B = 0;
    lshow("B0", l);
    l = lgood(), l.have_grid = false;
    lshow("no-grid", l);
    l = lgood(), l.have_times = false;
    lshow("no-times", l);
    l = lgood(), l.open_stream = true;
    lshow("open-stream", l);
    LnprobCall lw{false, false, true, false, true, 0, false, false, true};
    EXPECT(!strcmp(lcheck(lw), "bad arguments"));
    lw.arrays = true;
    EXPECT(strstr(lcheck(lw), "grad_gp == NULL"));
    lw.grad_gp = true;
    EXPECT(strstr(lcheck(lw), "go with grad_gp"));
    lw.grad_tau = true;
    EXPECT(strstr(lcheck(lw), "B must be at least 1"));
    lw.B = 1;
    EXPECT(strstr(lcheck(lw), "set_grid"));
    lw.have_grid = true;
    EXPECT(strstr(lcheck(lw), "set_times"));
    lw.have_times = true;
    EXPECT(strstr(lcheck(lw), "open stream"));
    lw.open_stream = false;
    EXPECT(lcheck(lw) == nullptr);
    if (failures) {
        fprintf(stderr, "%d invariant(s) failed\n", failures);
        return 1;
    }
    return 0;
}
