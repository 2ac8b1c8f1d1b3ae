// predict_host_check.cpp -- the pure-host part of the predict family (psoap_amd/csrc/predict_plan.hpp) built by a host
// compiler alone, with AddressSanitizer and UBSan (tests/test_predict_host.py): the shape of [B | Cx^T], the argument
// validation, the layout of the pinned staging block, the sentinel rows of the persistent launch, the prior means and
// variances and the flop count.  One line per case on stdout -- the shape spelled out, for the test to compare with its own
// restatement -- and a non-zero exit status when an invariant does not hold.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <utility>
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

// the regions of a staging block: inside the total, disjoint, together all of it; every one is written to its last double
// (the sanitizer watches the block's end), the record slots through a pointer of their own type
static void staging(const PredictShape& g, size_t n_acc, int rows_x)
{
    const PredictStaging s = predict_staging(g.Rq_pad, n_acc * sizeof(Acc), rows_x);
    const size_t r = (size_t)g.Rq_pad, x = (size_t)rows_x * r;
    std::vector<std::pair<size_t, size_t>> regions = {{s.m0, r}, {s.mu, r}, {s.var, r}, {s.prior, r}, {s.acc, n_acc * sizeof(Acc) / sizeof(double)},
                                                      {s.colx, x}, {s.rowx, x}, {s.diag, rows_x ? r : 0}};
    std::sort(regions.begin(), regions.end());
    size_t at = 0;
    for (const auto& reg : regions) {
        EXPECT(reg.first >= at && reg.first + reg.second <= s.total);
        at = std::max(at, reg.first + reg.second);
    }
    EXPECT(at == s.total);
    std::vector<double> block(s.total, 0.0);
    EXPECT((reinterpret_cast<uintptr_t>(block.data() + s.acc) % alignof(Acc)) == 0 && (s.acc * sizeof(double)) % 8 == 0);
    Acc* acc = reinterpret_cast<Acc*>(block.data() + s.acc);
    for (size_t k = 0; k < n_acc; ++k) acc[k] = Acc{1.0, 2.0, 0.0, 0.0};
    std::vector<double> pred((size_t)g.c * g.M), gp(6, 0.5), mu_c(3, 0.25);
    for (size_t k = 0; k < pred.size(); ++k) pred[k] = 8.5 + 1e-5 * (double)k;
    predict_prior_means(g, mu_c.data(), block.data() + s.m0);
    predict_prior_variances(g, gp.data(), block.data() + s.prior);
    if (rows_x) {
        predict_abscissae(g, pred.data(), block.data() + s.colx, block.data() + s.rowx);
        predict_diag(g, gp.data(), block.data() + s.diag);
    }
    for (size_t k = 0; k < n_acc; ++k) EXPECT(acc[k].logdet_half == 1.0 && acc[k].quad == 2.0 && acc[k].info == 0.0);
}

static void show(const char* name, int mode, int c, int N, int M)
{
    PredictShape g;
    const char* why = predict_check(mode, c, N, M, true);
    if (!why) why = predict_shape(mode, c, N, M, 0.25, g);
    if (why) {
        printf("%s mode=%d c=%d N=%d M=%d : %s\n", name, mode, c, N, M, why);
        return;
    }
    EXPECT(g.Npad % NB == 0 && g.Npad >= N && g.Npad - N < NB && g.Rq_pad % NB == 0 && g.Rq_pad >= g.Rq && g.Rq_pad - g.Rq < NB);
    EXPECT(g.ld == (size_t)NB * (g.P + g.Mt) && g.Rtot_pad == NB * g.Mt && (g.Rx > 0) == g.transposed_mean);
    staging(g, 1, c);      // the plain call
    if (!g.transposed_mean) staging(g, 2, 0);      // the call under the marginalised continuum
    printf("%s mode=%d c=%d N=%d M=%d : Npad %d P %d Rq %d Rq_pad %d Rx %d Rx_pad %d Rtot_pad %d ld %zu Mt %d nslab %d offset %.2f "
           "transposed %d dag %d\n",
           name, mode, c, N, M, g.Npad, g.P, g.Rq, g.Rq_pad, g.Rx, g.Rx_pad, g.Rtot_pad, g.ld, g.Mt, g.nslab, g.offset,
           (int)g.transposed_mean, (int)g.dag_ok);
}

static void by_hand()
{
    // mode 0, two components on three points each: block k of the columns is component k alone
    const double pred[6] = {1, 2, 3, 4, 5, 6}, gp[6] = {2.0, 7.0, 3.0, 7.0, 0.5, 7.0}, mu_c[3] = {0.3, 0.2, 0.1};
    PredictShape g;
    EXPECT(!predict_shape(0, 2, 10, 3, 0.3, g) && g.Rq == 6 && g.Rq_pad == 128 && g.offset == 1.0);
    std::vector<double> colx(2 * 128, -7.0), rowx(2 * 128, -7.0), v(128, -7.0);
    predict_abscissae(g, pred, colx.data(), rowx.data());
    const double col0[7] = {1, 2, 3, 1e30, 1e30, 1e30, 0}, col1[7] = {1e30, 1e30, 1e30, 4, 5, 6, 0};
    const double row0[7] = {1, 2, 3, -1e30, -1e30, -1e30, 0}, row1[7] = {-1e30, -1e30, -1e30, 4, 5, 6, 0};
    for (int q = 0; q < 7; ++q)
        EXPECT(colx[q] == col0[q] && colx[128 + q] == col1[q] && rowx[q] == row0[q] && rowx[128 + q] == row1[q]);
    EXPECT(colx[127] == 0.0 && colx[255] == 0.0 && rowx[127] == 0.0 && rowx[255] == 0.0);
    predict_diag(g, gp, v.data());
    EXPECT(v[0] == 4.0 && v[2] == 4.0 && v[3] == 9.0 && v[5] == 9.0 && v[6] == 0.0 && v[127] == 0.0);
    predict_prior_means(g, mu_c, v.data());
    EXPECT(v[0] == 0.3 && v[2] == 0.3 && v[3] == 0.2 && v[5] == 0.2);
    // the sum of two: every component on every column, no sentinel; the nugget of predict_f_g_sum on the variance
    EXPECT(!predict_shape(1, 2, 10, 3, 0.3, g) && g.Rq == 3 && g.offset == 1.0);
    predict_abscissae(g, pred, colx.data(), nullptr);
    EXPECT(colx[0] == 1 && colx[2] == 3 && colx[3] == 0 && colx[128] == 4 && colx[130] == 6 && colx[131] == 0);
    EXPECT(predict_prior_variance(1, 2, 3, 1, gp) == 13.0 + 1e-8);
    predict_prior_means(g, mu_c, v.data());
    EXPECT(v[0] == 0.3 && v[2] == 0.3);
    // three components: mode 0 takes each amplitude alone, the sum of three has no nugget and takes the prior mean off fl
    EXPECT(predict_prior_variance(0, 3, 2, 1, gp) == 4.0 && predict_prior_variance(0, 3, 2, 2, gp) == 9.0 && predict_prior_variance(0, 3, 2, 5, gp) == 0.25);
    EXPECT(predict_prior_variance(1, 3, 2, 0, gp) == 13.25 && predict_prior_variance(2, 1, 2, 1, gp) == 4.0);
    EXPECT(!predict_shape(1, 3, 10, 10, 0.3, g) && g.offset == 0.3 && g.transposed_mean && g.Rx == 10);
    EXPECT(!predict_shape(2, 1, 10, 4, 0.3, g) && g.offset == 0.3);
    // n = r = 128: n^3 / 3 + n^3 + (n^3 | 2 n^2 | 0) + 2 n^2
    const double n3 = 128.0 * 128.0 * 128.0, n2 = 128.0 * 128.0;
    EXPECT(predict_flops(128, 128, true, false) == n3 / 3.0 + n3 + n3 + 2.0 * n2 && predict_flops(128, 128, true, true) == predict_flops(128, 128, true, false));
    EXPECT(predict_flops(128, 128, false, true) == n3 / 3.0 + n3 + 2.0 * n2 + 2.0 * n2 && predict_flops(128, 128, false, false) == n3 / 3.0 + n3 + 2.0 * n2);
}

int main()
{
    // the cases of the exact pin (tests/golden/make_analysis_pin.py)
    show("c", 0, 2, 129, 65);
    show("a-sum", 1, 2, 100, 130);
    show("b", 2, 1, 128, 128);
    show("f", 0, 2, 312, 100);
    show("transposed", 1, 3, 129, 129);
    // the edge shapes of tests/test_gpu_parity.py::test_predict_edge_shapes_vs_oracle
    show("one-point", 2, 1, 74, 1);
    show("one-point-joint", 0, 1, 74, 1);
    show("four-column-tiles", 0, 3, 252, 129);
    // the last shape the persistent launch takes, the first it does not
    show("dag-255", 2, 1, 128 * 250, 128 * 5);
    show("dag-256", 2, 1, 128 * 250 + 1, 128 * 5);
    // refusals
    show("sum-of-three-M", 1, 3, 129, 100);
    show("mode3", 3, 1, 10, 10);
    show("c4", 0, 4, 10, 10);
    show("N0", 0, 2, 0, 10);
    show("M0", 0, 2, 10, 0);
    show("f-c2", 2, 2, 10, 10);
    printf("no-arrays : %s\n", predict_check(0, 2, 10, 10, false));
    by_hand();
    if (failures) {
        fprintf(stderr, "%d invariant(s) failed\n", failures);
        return 1;
    }
    return 0;
}
