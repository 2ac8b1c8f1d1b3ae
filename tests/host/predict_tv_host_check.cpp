// predict_tv_host_check.cpp -- the pure-host part of the predict under the time-variable kernel
// (psoap_amd/csrc/predict_plan.hpp: predict_tv_check, predict_tv_taus, predict_tv_flops, and the shape and staging
// arithmetic predict_tv_run takes from the plain call) built by a host compiler alone, with AddressSanitizer and UBSan
// (tests/test_predict_tv_host.py).  One line per case on stdout -- the refusal, or the sizes the run allocates and the grids
// it launches, for the test to compare with its own restatement -- and a non-zero exit status when an invariant does not hold.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

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

struct Acc {      // the library's MatAcc: four doubles
    double logdet_half, quad, info, pad;
};

static const double INF = std::numeric_limits<double>::infinity();
static const double QNAN = std::numeric_limits<double>::quiet_NaN();

// what predict_tv_run sizes and launches for a call that passed the check: the staging block written to its last double
// (the sanitizer watches its end), the rows of the staged sweep, the fills' grids
static void show(const char* name, int mode, int c, int N, int M)
{
    std::vector<double> tau((size_t)(c > 0 ? c : 1), 3.0), tp((size_t)(M > 0 ? M : 1), 1.5);
    const char* why = predict_tv_check(mode, c, M, true, true, false, false, tau.data(), tp.data());
    PredictShape g;
    if (!why) why = predict_shape(mode, c, N, M, 0.25, g);
    if (why) {
        printf("%s mode=%d c=%d N=%d M=%d : %s\n", name, mode, c, N, M, why);
        return;
    }
    EXPECT(!g.transposed_mean && g.Rx == 0 && g.Rtot_pad == g.Rq_pad && g.ld == (size_t)NB * (g.P + g.Mt));
    const PredictStaging s = predict_staging(g.Rq_pad, sizeof(Acc), 0);
    EXPECT(s.colx == s.rowx && s.rowx == s.diag && s.diag == s.total);      // no rows of the persistent launch
    std::vector<double> block(s.total, 0.0), gp(6, 0.5), mu_c(3, 0.25);
    predict_prior_means(g, mu_c.data(), block.data() + s.m0);
    predict_prior_variances(g, gp.data(), block.data() + s.prior);
    for (int q = 0; q < g.Rq_pad; ++q) block[s.mu + q] = block[s.var + q] = 1.0;
    Acc* acc = reinterpret_cast<Acc*>(block.data() + s.acc);
    acc[0] = Acc{1.0, 2.0, 0.0, 0.0};
    EXPECT(block[s.total - 1] == 0.0 && block[s.m0] == 0.25);
    // the staged sweep: row p updates and solves P - p + Mt tile columns; the last row's strip is the appended block alone
    long long update_tiles = 0, strip_tiles = 0;
    for (int p = 0; p < g.P; ++p) {
        const int ntile = g.P - p + g.Mt;
        EXPECT(ntile - 1 >= g.Mt && ntile - 1 >= 1);
        if (p > 0) update_tiles += (long long)p * ntile;
        strip_tiles += ntile - 1;
    }
    // the fills: a region launch per component block in mode 0, one otherwise; column offsets stay inside the row
    const int blocks = mode == 0 ? c : 1;
    for (int k = 0; k < blocks; ++k) {
        const int col0 = g.Npad + k * M;
        EXPECT(col0 + M <= (int)g.ld);
        if (mode == 0) EXPECT((size_t)(k * M + M) <= (size_t)g.Rq_pad);
    }
    const int St = g.Rq_pad / NB;
    printf("%s mode=%d c=%d N=%d M=%d : ld %zu Rq %d Rq_pad %d staging %zu cross %dx(%d,%d) prior %dx(%d,%d) sym %d update %lld strip %lld "
           "sigma %d gemv (%d,%d) flops %.6e %.6e %.6e\n",
           name, mode, c, N, M, g.ld, g.Rq, g.Rq_pad, s.total, blocks, (M + NB - 1) / NB, (N + NB - 1) / NB, blocks, (M + NB - 1) / NB,
           (M + NB - 1) / NB, g.P * (g.P + 1) / 2, update_tiles, strip_tiles, St * (St + 1) / 2, (g.Rq + 127) / 128, g.nslab,
           predict_tv_flops(g.Npad, g.Rq_pad, true, false), predict_tv_flops(g.Npad, g.Rq_pad, false, true),
           predict_tv_flops(g.Npad, g.Rq_pad, false, false));
    EXPECT(predict_tv_flops(g.Npad, g.Rq_pad, true, true) == predict_flops(g.Npad, g.Rq_pad, true, true));
}

static void refusal(const char* name, int mode, int c, int M, bool arrays, bool times, bool stream, bool baseline, const double* tau,
                    const double* tp)
{
    const char* why = predict_tv_check(mode, c, M, arrays, times, stream, baseline, tau, tp);
    printf("%s : %s\n", name, why ? why : "ok");
}

static void by_hand()
{
    double v[3];
    const double tau[3] = {5.0, INF, 7.0};
    predict_tv_taus(tau, 0, 3, v);
    EXPECT(v[0] == 5.0 && isinf(v[1]) && v[2] == 7.0);
    predict_tv_taus(tau, 2, 1, v);
    EXPECT(v[0] == 7.0 && isinf(v[1]) && v[1] > 0 && isinf(v[2]));
    predict_tv_taus(tau, 0, 2, v);
    EXPECT(v[0] == 5.0 && isinf(v[1]) && isinf(v[2]));
    // exactly M dates and c time scales are read: the vectors end where the check must stop
    std::vector<double> tp(130, 2.0), t2(2, 1.0);
    EXPECT(predict_tv_check(0, 2, 130, true, true, false, false, t2.data(), tp.data()) == nullptr);
    tp[129] = INF;
    EXPECT(predict_tv_check(0, 2, 130, true, true, false, false, t2.data(), tp.data()) != nullptr);
    EXPECT(predict_tv_check(0, 2, 129, true, true, false, false, t2.data(), tp.data()) == nullptr);
    // the order of the refusals: arguments and modes before the handle's state, the state before the values
    const double bad_tau[2] = {1.0, -1.0};
    EXPECT(strstr(predict_tv_check(2, 2, 4, true, false, true, true, bad_tau, tp.data()), "mode 2"));
    EXPECT(strstr(predict_tv_check(0, 2, 4, true, false, true, true, bad_tau, tp.data()), "set_times"));
    EXPECT(strstr(predict_tv_check(0, 2, 4, true, true, true, true, bad_tau, tp.data()), "open stream"));
    EXPECT(strstr(predict_tv_check(0, 2, 4, true, true, false, true, bad_tau, tp.data()), "baseline"));
    EXPECT(strstr(predict_tv_check(0, 2, 4, true, true, false, false, bad_tau, tp.data()), "tau"));
}

int main()
{
    // the cases of tests/test_gpu_timevar_predict.py
    show("N100-c2", 0, 2, 100, 50);
    show("N100-c2-sum", 1, 2, 100, 130);
    show("N300-c1", 2, 1, 300, 129);
    show("N129-c2", 0, 2, 129, 65);
    show("N300-c3", 0, 3, 300, 43);
    show("N300-c2", 0, 2, 300, 100);
    show("N520-c2", 0, 2, 520, 64);
    // the retrieve shape of the timing table, one date and two
    show("retrieve", 0, 3, 8192, 1024);
    show("retrieve-two-dates", 0, 3, 8192, 2048);
    show("one-point", 2, 1, 74, 1);
    // refusals by mode
    show("sum-of-three", 1, 3, 129, 129);
    show("f-c2", 2, 2, 10, 10);
    show("sum-c1", 1, 1, 10, 10);
    show("components-c1", 0, 1, 10, 10);
    show("mode3", 3, 1, 10, 10);
    show("c4", 0, 4, 10, 10);
    show("M0", 0, 2, 10, 0);
    // refusals by state and value
    const double one[3] = {1.0, 1.0, 1.0}, tp[4] = {0.0, -3.5, 1e9, 2.0};
    const double zero[2] = {1.0, 0.0}, neg[2] = {-2.0, 1.0}, nan_tau[2] = {QNAN, 1.0}, inf_tau[2] = {INF, INF};
    const double tp_inf[4] = {0.0, INF, 1.0, 2.0}, tp_ninf[4] = {0.0, 1.0, -INF, 2.0}, tp_nan[4] = {0.0, 1.0, 2.0, QNAN};
    refusal("ok", 0, 2, 4, true, true, false, false, one, tp);
    refusal("inf-tau", 0, 2, 4, true, true, false, false, inf_tau, tp);
    refusal("no-arrays", 0, 2, 4, false, true, false, false, one, tp);
    refusal("no-tau", 0, 2, 4, true, true, false, false, nullptr, tp);
    refusal("no-t_pred", 0, 2, 4, true, true, false, false, one, nullptr);
    refusal("no-times", 0, 2, 4, true, false, false, false, one, tp);
    refusal("open-stream", 0, 2, 4, true, true, true, false, one, tp);
    refusal("baseline", 0, 2, 4, true, true, false, true, one, tp);
    refusal("tau-zero", 0, 2, 4, true, true, false, false, zero, tp);
    refusal("tau-negative", 0, 2, 4, true, true, false, false, neg, tp);
    refusal("tau-nan", 0, 2, 4, true, true, false, false, nan_tau, tp);
    refusal("t_pred-inf", 0, 2, 4, true, true, false, false, one, tp_inf);
    refusal("t_pred-minus-inf", 0, 2, 4, true, true, false, false, one, tp_ninf);
    refusal("t_pred-nan", 0, 2, 4, true, true, false, false, one, tp_nan);
    by_hand();
    if (failures) {
        fprintf(stderr, "%d invariant(s) failed\n", failures);
        return 1;
    }
    return 0;
}
