// marg_tv_host_check.cpp -- the pure-host refusals of the time-variable kernel under the marginalised continuum
// (psoap_amd/csrc/marg_grad_plan.hpp: marg_tv_check, what psoap_chunk_lnlike_marg_tv, psoap_chunk_lnlike_marg_tv_grad and
// psoap_chunk_fisher_marg_tv ask before any work) built by a host compiler alone, with sanitizers
// (tests/test_marg_tv_host.py).  One line per case on stdout -- the refusal, or "ok" -- for the test to compare with what it
// expects, and a non-zero exit status when an invariant does not hold.
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

// a call every entry accepts: the arrays there, the whole gradient asked for, B = 3 of max_batch 4, c = 2, T = 9 of 32, times
// set, no open stream, a baseline that is not stale
static MargTvCall good()
{
    return MargTvCall{true, true, true, true, 3, 2, 9, 4, 32, true, false, true, false};
}

static const char* name_of(MargTvEntry e)
{
    return e == MargTvEntry::Value ? "value" : e == MargTvEntry::Grad ? "grad" : "fisher";
}

static void show(MargTvEntry e, const char* name, const MargTvCall& a)
{
    const char* why = marg_tv_check(e, a);
    printf("%s %s : %s\n", name_of(e), name, why ? why : "ok");
}

int main()
{
    const MargTvEntry entries[] = {MargTvEntry::Value, MargTvEntry::Grad, MargTvEntry::Fisher};
    for (MargTvEntry e : entries) {
        MargTvCall a = good();
        show(e, "ok", a);
        a = good(), a.arrays = false;
        show(e, "no-arrays", a);
        a = good(), a.c = 0;
        show(e, "c0", a);
        a = good(), a.c = 4;
        show(e, "c4", a);
        a = good(), a.c = 1;
        show(e, "c1", a);
        a = good(), a.c = 3;
        show(e, "c3", a);
        a = good(), a.have_times = false;
        show(e, "no-times", a);
        a = good(), a.open_stream = true;
        show(e, "open-stream", a);
        a = good(), a.have_baseline = false;
        show(e, "no-baseline", a);
        a = good(), a.stale_weight = true;
        show(e, "stale", a);
    }
    MargTvCall a = good();
    // B: the value entry walks a batch of the handle's slots' size at most, the gradient any B >= 1; the Fisher entry has none
    a = good(), a.B = 0;
    show(MargTvEntry::Value, "B0", a);
    show(MargTvEntry::Grad, "B0", a);
    show(MargTvEntry::Fisher, "B0", a);
    a = good(), a.B = 4;
    show(MargTvEntry::Value, "Bmax", a);
    a = good(), a.B = 5;
    show(MargTvEntry::Value, "Bmax+1", a);
    show(MargTvEntry::Grad, "Bmax+1", a);
    a = good(), a.B = 1;
    show(MargTvEntry::Value, "B1", a);
    // T: the Fisher entry alone looks at it
    a = good(), a.T = 0;
    show(MargTvEntry::Fisher, "T0", a);
    show(MargTvEntry::Value, "T0", a);
    a = good(), a.T = 1;
    show(MargTvEntry::Fisher, "T1", a);
    a = good(), a.T = 32;
    show(MargTvEntry::Fisher, "T32", a);
    a = good(), a.T = 33;
    show(MargTvEntry::Fisher, "T33", a);
    // the NULL rules of the gradient entry: grad_gp == NULL is the value only; grad_tau goes with grad_gp
    a = good(), a.grad_gp = a.grad_tau = a.grad_rest = false;
    show(MargTvEntry::Grad, "value-only", a);
    a = good(), a.grad_gp = false;
    show(MargTvEntry::Grad, "tau-without-gp", a);
    a = good(), a.grad_gp = a.grad_tau = false;
    show(MargTvEntry::Grad, "rest-without-gp", a);
    a = good(), a.grad_tau = false;
    show(MargTvEntry::Grad, "gp-without-tau", a);
    a = good(), a.grad_rest = false;
    show(MargTvEntry::Grad, "gp-and-tau", a);
    a = good(), a.grad_gp = false;
    show(MargTvEntry::Value, "grad-flags-ignored", a);

    // the order of the refusals: everything wrong at once, then mended one by one
    for (MargTvEntry e : entries) {
        MargTvCall w{false, false, true, true, 0, 0, 0, 4, 32, false, true, false, true};
        EXPECT(!strcmp(marg_tv_check(e, w), "bad arguments"));
        w.arrays = true;
        if (e == MargTvEntry::Grad) {
            EXPECT(strstr(marg_tv_check(e, w), "grad_gp == NULL"));
            w.grad_gp = true, w.grad_tau = false;
            EXPECT(strstr(marg_tv_check(e, w), "grad_tau goes with grad_gp"));
            w.grad_tau = true;
        }
        EXPECT(strstr(marg_tv_check(e, w), "number of components"));
        w.c = 2;
        EXPECT(strstr(marg_tv_check(e, w), e == MargTvEntry::Value  ? "batch size outside"
                                           : e == MargTvEntry::Grad ? "B must be at least 1"
                                                                    : "number of tangents"));
        w.B = 1, w.T = 1;
        EXPECT(strstr(marg_tv_check(e, w), "set_times"));
        w.have_times = true;
        EXPECT(strstr(marg_tv_check(e, w), "open stream"));
        w.open_stream = false;
        EXPECT(strstr(marg_tv_check(e, w), "psoap_chunk_set_baseline first"));
        w.have_baseline = true;
        EXPECT(strstr(marg_tv_check(e, w), "psoap_chunk_set_baseline again"));
        w.stale_weight = false;
        EXPECT(marg_tv_check(e, w) == nullptr);
    }
    // the words: the handle's state as the time-variable entries say it (predict_plan.hpp), the baseline as the marginal ones
    MargTvCall s = good();
    s.have_times = false;
    EXPECT(!strcmp(marg_tv_check(MargTvEntry::Fisher, s), fisher_tv_check(2, 9, 32, true, false, false, false)));
    s = good(), s.open_stream = true;
    EXPECT(!strcmp(marg_tv_check(MargTvEntry::Fisher, s), fisher_tv_check(2, 9, 32, true, true, true, false)));
    s = good(), s.T = 40;
    EXPECT(!strcmp(marg_tv_check(MargTvEntry::Fisher, s), fisher_tv_check(2, 40, 32, true, true, false, false)));
    s = good(), s.have_baseline = false;
    EXPECT(!strcmp(marg_tv_check(MargTvEntry::Grad, s), marg_grad_check(3, 2, false, false)));
    s = good(), s.stale_weight = true;
    EXPECT(!strcmp(marg_tv_check(MargTvEntry::Value, s), marg_grad_check(3, 2, true, true)));
    // what the time-variable entries refuse, a handle WITH a baseline, is what these ask for
    EXPECT(fisher_tv_check(2, 9, 32, true, true, false, true) != nullptr && marg_tv_check(MargTvEntry::Fisher, good()) == nullptr);
    if (failures) {
        fprintf(stderr, "%d invariant(s) failed\n", failures);
        return 1;
    }
    return 0;
}
