// qp_fisher_host_check.cpp -- the pure-host part of psoap_chunk_fisher_qp and psoap_chunk_loo_qp (psoap_amd/csrc/qp_plan.hpp:
// fisher_qp_check, loo_qp_check, fisher_qp_sizes) built by a host compiler alone, with AddressSanitizer and UBSan
// (tests/test_qp_fisher_host.py).  One line per case on stdout -- the refusal, or "ok" -- for the test to compare with what it
// expects, and a non-zero exit status when an invariant does not hold.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../psoap_amd/csrc/predict_plan.hpp"
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

static const int MAX_T = 32;

static void say(const char* name, const char* why) { printf("%s : %s\n", name, why ? why : "ok"); }

static bool same(const char* a, const char* b) { return (a == nullptr && b == nullptr) || (a && b && strcmp(a, b) == 0); }

int main()
{
    // fisher_qp_check(c, T, max_T, arrays, have_times, open_stream, have_baseline)
    say("fisher-good", fisher_qp_check(2, 8, MAX_T, true, true, false, false));
    say("fisher-T1", fisher_qp_check(1, 1, MAX_T, true, true, false, false));
    say("fisher-T32", fisher_qp_check(3, 32, MAX_T, true, true, false, false));
    say("fisher-no-arrays", fisher_qp_check(2, 8, MAX_T, false, true, false, false));
    say("fisher-c0", fisher_qp_check(0, 8, MAX_T, true, true, false, false));
    say("fisher-c4", fisher_qp_check(4, 8, MAX_T, true, true, false, false));
    say("fisher-T0", fisher_qp_check(2, 0, MAX_T, true, true, false, false));
    say("fisher-T33", fisher_qp_check(2, 33, MAX_T, true, true, false, false));
    say("fisher-no-times", fisher_qp_check(2, 8, MAX_T, true, false, false, false));
    say("fisher-open-stream", fisher_qp_check(2, 8, MAX_T, true, true, true, false));
    say("fisher-baseline", fisher_qp_check(2, 8, MAX_T, true, true, false, true));
    // the order: the arrays, c, T, the times, the stream, the baseline
    say("fisher-order-c-before-T", fisher_qp_check(0, 0, MAX_T, true, false, true, true));
    say("fisher-order-T-before-times", fisher_qp_check(2, 0, MAX_T, true, false, true, true));
    say("fisher-order-times-before-stream", fisher_qp_check(2, 8, MAX_T, true, false, true, true));
    say("fisher-order-stream-before-baseline", fisher_qp_check(2, 8, MAX_T, true, true, true, true));
    // loo_qp_check(c, arrays, have_times, open_stream, have_baseline)
    say("loo-good", loo_qp_check(2, true, true, false, false));
    say("loo-no-arrays", loo_qp_check(2, false, true, false, false));
    say("loo-c0", loo_qp_check(0, true, true, false, false));
    say("loo-c4", loo_qp_check(4, true, true, false, false));
    say("loo-no-times", loo_qp_check(2, true, false, false, false));
    say("loo-open-stream", loo_qp_check(2, true, true, true, false));
    say("loo-baseline", loo_qp_check(2, true, true, false, true));

    // every refusal but the baseline's is the time-variable twin's, word for word, over the whole grid of states
    for (int c = 0; c <= 4; ++c)
        for (int T : {0, 1, 32, 33})
            for (int bits = 0; bits < 16; ++bits) {
                const bool arrays = bits & 1, times = bits & 2, open = bits & 4, base = bits & 8;
                const char* q = fisher_qp_check(c, T, MAX_T, arrays, times, open, base);
                const char* t = fisher_tv_check(c, T, MAX_T, arrays, times, open, base);
                const char* ql = loo_qp_check(c, arrays, times, open, base);
                const char* tl = tv_analysis_check(c, arrays, times, open, base);
                EXPECT((q == nullptr) == (t == nullptr));
                EXPECT((ql == nullptr) == (tl == nullptr));
                if (q && !strstr(q, "baseline")) EXPECT(same(q, t));
                if (q && strstr(q, "baseline")) EXPECT(t && strstr(t, "baseline") && strstr(q, "quasi-periodic"));
                if (ql && !strstr(ql, "baseline")) EXPECT(same(ql, tl));
            }

    // the workspace arithmetic: what fisher_run asks of the Fisher workspace for the quasi-periodic call
    const int tile = 6 * 128 + 3 * 5;      // QpTile::DOUBLES of grad_kernels.hpp (psoap_gp.hip asserts the same number)
    {
        const FisherQpSizes s = fisher_qp_sizes(3, 8192, 64, 32, tile);
        EXPECT(s.grid == (size_t)32 * 3 * 8192 && s.hyper == 32u * 6 && s.temporal == 32u * 3);
        EXPECT(s.part == (size_t)64 * 65 / 2 * tile);
    }
    {
        const FisherQpSizes s = fisher_qp_sizes(1, 1, 1, 1, tile);
        EXPECT(s.grid == 1 && s.hyper == 2 && s.temporal == 1 && s.part == (size_t)tile);
    }
    {
        // no 32-bit overflow: P (P + 1) / 2 tiles of 783 doubles at P = 3000, T c N at N = 400000
        const FisherQpSizes s = fisher_qp_sizes(3, 400000, 3000, 32, tile);
        EXPECT(s.part == (size_t)3000 * 3001 / 2 * 783);
        EXPECT(s.grid == (size_t)38400000);
        std::vector<char> touch(64, 0);      // (something for AddressSanitizer to watch)
        EXPECT(touch[63] == 0);
    }
    // the records of one tangent are independent of T; the tangents grow linearly with it
    for (int T = 1; T <= MAX_T; ++T) {
        const FisherQpSizes a = fisher_qp_sizes(2, 300, 3, T, tile), b = fisher_qp_sizes(2, 300, 3, 1, tile);
        EXPECT(a.part == b.part && a.grid == T * b.grid && a.hyper == T * b.hyper && a.temporal == T * b.temporal);
    }
    return failures ? 1 : 0;
}
