// qp_host_check.cpp -- the pure-host part of the quasi-periodic entry (psoap_amd/csrc/qp_plan.hpp: qp_check, qp_refused)
// built by a host compiler alone, with AddressSanitizer and UBSan (tests/test_qp_host.py).  One line per case on stdout --
// the refusal, or "ok" -- for the test to compare with what it expects, and a non-zero exit status when an invariant does
// not hold.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../psoap_amd/csrc/qp_plan.hpp"

using namespace psoap;

static int failures = 0;

#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// a full gradient call on a handle in good state
static QpCall good() { return QpCall{true, true, true, true, true, true, 3, 2, true, false, false}; }

static void say(const char* name, const QpCall& a)
{
    const char* why = qp_check(a);
    printf("%s : %s\n", name, why ? why : "ok");
}

int main()
{
    QpCall a = good();
    say("full", a);
    a = good(), a.grad_rest = false;
    say("no-optional", a);
    a = good(), a.grad_gp = a.grad_tau = a.grad_gamma = a.grad_period = a.grad_rest = false;
    say("value-only", a);
    a = good(), a.arrays = false;
    say("no-arrays", a);
    a = good(), a.grad_gp = false;
    say("value-with-temporal", a);
    a = good(), a.grad_gp = a.grad_tau = a.grad_gamma = a.grad_period = false;
    say("value-with-rest", a);
    a = good(), a.grad_tau = false;
    say("no-grad-tau", a);
    a = good(), a.grad_gamma = false;
    say("no-grad-gamma", a);
    a = good(), a.grad_period = false;
    say("no-grad-period", a);
    a = good(), a.B = 0;
    say("B0", a);
    a = good(), a.c = 0;
    say("c0", a);
    a = good(), a.c = 4;
    say("c4", a);
    a = good(), a.have_times = false;
    say("no-times", a);
    a = good(), a.open_stream = true;
    say("open-stream", a);
    a = good(), a.have_baseline = true;
    say("baseline", a);
    // the order of the refusals: arrays, the NULL rules, B, c, then the handle's state -- times, stream, baseline
    a = QpCall{false, false, true, false, false, true, 0, 4, false, true, true};
    EXPECT(strstr(qp_check(a), "bad arguments"));
    a.arrays = true;
    EXPECT(strstr(qp_check(a), "grad_gp == NULL"));
    a.grad_gp = true;
    EXPECT(strstr(qp_check(a), "go with grad_gp"));
    a.grad_gamma = a.grad_period = true;
    EXPECT(strstr(qp_check(a), "B must be"));
    a.B = 1;
    EXPECT(strstr(qp_check(a), "components"));
    a.c = 3;
    EXPECT(strstr(qp_check(a), "set_times"));
    a.have_times = true;
    EXPECT(strstr(qp_check(a), "open stream"));
    a.open_stream = false;
    EXPECT(strstr(qp_check(a), "baseline"));
    a.have_baseline = false;
    EXPECT(qp_check(a) == nullptr);

    // qp_refused reads exactly c values of proposal b from arrays of exactly B * c doubles (heap: the sanitizer sees an overrun)
    const double inf = INFINITY, nan = NAN;
    for (int c = 1; c <= 3; ++c) {
        const int B = 4;
        std::vector<double> gam((size_t)B * c, 1.0), per((size_t)B * c, 2.5);
        for (int b = 0; b < B; ++b) EXPECT(!qp_refused(gam.data(), per.data(), c, b));
        const double bad_gamma[] = {-1.0, -0.5e-300, nan, inf, -inf}, bad_period[] = {0.0, -0.0, -2.0, nan, inf, -inf, 4.9e-324, 5e-309};
        for (int k = 0; k < c; ++k) {
            for (double v : bad_gamma) {
                gam[(size_t)2 * c + k] = v;
                EXPECT(qp_refused(gam.data(), per.data(), c, 2));
                EXPECT(!qp_refused(gam.data(), per.data(), c, 1) && !qp_refused(gam.data(), per.data(), c, 3));
                gam[(size_t)2 * c + k] = 1.0;
            }
            for (double v : bad_period) {
                per[(size_t)(B - 1) * c + k] = v;
                EXPECT(qp_refused(gam.data(), per.data(), c, B - 1));
                EXPECT(!qp_refused(gam.data(), per.data(), c, B - 2));
                per[(size_t)(B - 1) * c + k] = 2.5;
            }
            // Gamma = 0 (and -0) is the time-variable model, a tiny and a huge finite period whose reciprocal is finite are periods
            gam[(size_t)k] = 0.0;
            EXPECT(!qp_refused(gam.data(), per.data(), c, 0));
            gam[(size_t)k] = -0.0;
            EXPECT(!qp_refused(gam.data(), per.data(), c, 0));
            per[(size_t)k] = 1e-300;
            EXPECT(!qp_refused(gam.data(), per.data(), c, 0));
            per[(size_t)k] = 1e300;
            EXPECT(!qp_refused(gam.data(), per.data(), c, 0));
            gam[(size_t)k] = 1.0, per[(size_t)k] = 2.5;
        }
    }
    if (failures) {
        fprintf(stderr, "%d invariant(s) failed\n", failures);
        return 1;
    }
    return 0;
}
