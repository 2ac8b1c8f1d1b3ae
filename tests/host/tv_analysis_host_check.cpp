// tv_analysis_host_check.cpp -- the pure-host refusals of the analysis paths under the time-variable kernel
// (psoap_amd/csrc/predict_plan.hpp: tv_analysis_check, fisher_tv_check) built by a host compiler alone
// (tests/test_timevar_fisher_reference.py).  One line per case on stdout -- the refusal, or "ok" -- for the test to compare
// with what it expects, and a non-zero exit status when an invariant does not hold.
#include <stdio.h>
#include <string.h>

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

static void fisher(const char* name, int c, int T, bool arrays, bool times, bool stream, bool baseline)
{
    const char* why = fisher_tv_check(c, T, 32, arrays, times, stream, baseline);
    printf("fisher %s : %s\n", name, why ? why : "ok");
}

static void loo(const char* name, int c, bool arrays, bool times, bool stream, bool baseline)
{
    const char* why = tv_analysis_check(c, arrays, times, stream, baseline);
    printf("loo %s : %s\n", name, why ? why : "ok");
}

int main()
{
    fisher("ok", 2, 9, true, true, false, false);
    fisher("T1", 1, 1, true, true, false, false);
    fisher("T32", 3, 32, true, true, false, false);
    fisher("T0", 2, 0, true, true, false, false);
    fisher("T33", 2, 33, true, true, false, false);
    fisher("no-arrays", 2, 9, false, true, false, false);
    fisher("c0", 0, 9, true, true, false, false);
    fisher("c4", 4, 9, true, true, false, false);
    fisher("no-times", 2, 9, true, false, false, false);
    fisher("open-stream", 2, 9, true, true, true, false);
    fisher("baseline", 2, 9, true, true, false, true);
    loo("ok", 2, true, true, false, false);
    loo("no-arrays", 2, false, true, false, false);
    loo("c4", 4, true, true, false, false);
    loo("no-times", 2, true, false, false, false);
    loo("open-stream", 2, true, true, true, false);
    loo("baseline", 2, true, true, false, true);
    // the order of the refusals: arguments, then the number of tangents, then the handle's state -- times, stream, baseline
    EXPECT(strstr(fisher_tv_check(2, 0, 32, false, false, true, true), "bad arguments"));
    EXPECT(strstr(fisher_tv_check(2, 0, 32, true, false, true, true), "tangents"));
    EXPECT(strstr(fisher_tv_check(2, 4, 32, true, false, true, true), "set_times"));
    EXPECT(strstr(fisher_tv_check(2, 4, 32, true, true, true, true), "open stream"));
    EXPECT(strstr(fisher_tv_check(2, 4, 32, true, true, false, true), "baseline"));
    EXPECT(strstr(tv_analysis_check(2, true, false, true, true), "set_times"));
    // the words are predict_tv_check's
    const double tau[2] = {1.0, 1.0}, tp[1] = {0.0};
    EXPECT(!strcmp(tv_analysis_check(2, true, false, false, false), predict_tv_check(0, 2, 1, true, false, false, false, tau, tp)));
    EXPECT(!strcmp(tv_analysis_check(2, true, true, true, false), predict_tv_check(0, 2, 1, true, true, true, false, tau, tp)));
    EXPECT(!strcmp(tv_analysis_check(2, true, true, false, true), predict_tv_check(0, 2, 1, true, true, false, true, tau, tp)));
    if (failures) {
        fprintf(stderr, "%d invariant(s) failed\n", failures);
        return 1;
    }
    return 0;
}
