"""CPU: the two references of the component spectra under the marginalised continuum (tests/marg_predict_reference.py)
against each other and against the oracle's plain predict -- what tests/test_gpu_marg_predict.py then holds the device to.

The float64-against-long-double table (python tests/marg_predict_reference.py), errors as ``errors`` defines them:

    case                                     mu      Sigma        var
    a-N100-c2-o1-mode0-M50-one         6.05e-13   1.06e-13   1.06e-13
    a-N100-c2-o1-mode0-M50-flux        5.73e-13   9.34e-14   9.36e-14
    a-N100-c2-o1-mode1-M130-one        1.18e-12   2.25e-13   2.25e-13
    a-N100-c2-o1-mode1-M130-flux       1.10e-12   1.95e-13   1.95e-13
    b-N128-c1-o0-mode2-M128-one        4.23e-15   2.31e-15   1.31e-15
    b-N128-c1-o0-mode2-M128-flux       4.60e-15   2.21e-15   1.15e-15
    c-N129-c2-o2-mode0-M65-one         5.95e-14   2.93e-13   2.93e-13
    c-N129-c2-o2-mode0-M65-flux        1.11e-13   2.80e-13   2.79e-13
    d-N384-c1-o3-mode2-M129-one        2.03e-13   6.17e-14   6.14e-14
    d-N384-c1-o3-mode2-M129-flux       1.99e-13   6.34e-14   6.32e-14
    e-N300-c3-o1-mode0-M43-one         1.32e-13   3.45e-14   3.49e-14
    e-N300-c3-o1-mode0-M43-flux        1.22e-13   2.78e-14   2.81e-14
    f-N312-c2-o4-mode0-M100-one        2.92e-12   1.89e-12   1.89e-12
    f-N312-c2-o4-mode0-M100-flux       2.98e-12   1.60e-12   1.60e-12
    max                                2.98e-12   1.89e-12   1.89e-12

The sanity bound on the reference itself started at 1e-9 and was tightened, once this table existed, to 8 times its
maxima -- the project's margin (tests/test_gpu_grad.py) -- which is also the tolerance of the GPU tests."""
import numpy as np
import pytest

import marg_predict_reference as mp
import marg_reference as mr

_LD = np.longdouble
TABLE_MAX = {"mu": 2.98e-12, "Sigma": 1.89e-12, "var": 1.89e-12}
TOL = {k: 8.0 * v for k, v in TABLE_MAX.items()}


@pytest.mark.parametrize("kind", mp.WEIGHTS)
@pytest.mark.parametrize("pc", mp.PCASES, ids=mp.pcase_id)
def test_the_float64_route_agrees_with_the_dense_long_double_solve(pc, kind):
    f = mp.marg_predict_f64(*mp.pcase_args(pc, kind))
    err = mp.errors(f.mu, f.Sigma, f.var, mp.pcase_ext(pc, kind))
    print(mp.pcase_id(pc), kind, err)
    for k in mp.OUTPUTS:
        assert err[k] <= TOL[k], (k, err[k])
    assert err["mu"] <= 1e-9 and err["Sigma"] <= 1e-9 and err["var"] <= 1e-9      # (the bound before the table existed)


def test_a_vanishing_prior_gives_the_plain_predict_and_the_difference_falls_as_sd_squared():
    """case a, mode 0.  (K + H L H^T)^-1 = K^-1 - K^-1 H L H^T K^-1 + O(L^2): the difference to the plain predict is linear
    in Lambda = sd^2.  The second-order term is at most Lambda ||H^T K^-1 H|| of the first, and H^T K^-1 H <= n_e / sigma^2
    = 25 / 4e-4 per epoch: 1.6 % at a hundredth of the cases' prior (sd_0 = 5e-4), 0.016 % at a thousandth -- so the ratio
    of the two differences is 100 within 5 %."""
    pc = mp.PCASES[0]
    args = mp.pcase_args(pc, "one")
    mu0, S0 = mp.plain_predict_ext(*args[:7])
    sd = mr.prior_sd(mr.case_named(pc[0])[5])
    diff = []
    for scale in (1e-2, 1e-3):
        r = mp.marg_predict_ext(*mp.pcase_args(pc, "one", sd=scale * sd))
        diff.append((float(np.max(np.abs(r.mu - mu0))), float(np.max(np.abs(r.Sigma - S0)))))
    print(diff)
    for k in (0, 1):
        assert diff[1][k] < diff[0][k]
        assert abs(diff[0][k] / diff[1][k] / 100.0 - 1.0) < 0.05, diff
    # and at the smaller prior the marginal prediction is the plain one to that order: Lambda ||H^T K^-1 H|| = 1.6e-4 of
    # the largest entry of either output
    assert diff[1][0] < 1e-3 * float(np.max(np.abs(mu0))) and diff[1][1] < 1e-3 * float(np.max(np.abs(S0)))


@pytest.mark.parametrize("kind", mp.WEIGHTS)
@pytest.mark.parametrize("pc", mp.PCASES, ids=mp.pcase_id)
def test_the_marginal_covariance_is_the_plain_one_plus_a_positive_semidefinite_term(pc, kind):
    """Sigma_marg - Sigma_plain has no eigenvalue below -1e-12 max prior variance: its long-double Cholesky goes through once
    that much is added to the diagonal (it raises at a pivot that is not positive)."""
    import oracle
    ref = mp.pcase_ext(pc, kind)
    _, S0 = mp.plain_predict_ext(*mp.pcase_args(pc, kind)[:7])
    D = np.array(ref.Sigma - S0)
    D[np.diag_indices_from(D)] += _LD(1e-12) * ref.prior_max
    oracle._chol_ext(D)
    assert np.all(np.diag(ref.Sigma) >= np.diag(S0) - _LD(1e-12) * ref.prior_max)


def test_a_continuum_offset_within_the_prior_moves_the_marginal_mean_less_than_the_plain_mean():
    """The reason the feature exists, on case d (mode 2, N 384, three epochs of 128 pixels, order 3): H b with
    b[e, k] = +-prior_sd[k], the sign alternating with the epoch, is added to the flux.  The mean is linear in the flux, so
    the shift is Cx Kt^-1 H b against Cx K^-1 H b."""
    pc = mp.PCASES[4]
    assert pc[0] == "d"
    args = list(mp.pcase_args(pc, "one"))
    ch = mr.case_chunk(mr.case_named("d"))
    sd = mr.prior_sd(ch.order)
    b = np.concatenate([(1.0 if e % 2 == 0 else -1.0) * sd for e in range(ch.n_epochs)])
    assert np.all(np.abs(b.reshape(ch.n_epochs, -1)) <= sd)
    H = mr.basis(ch.x, ch.epoch_index, ch.n_epochs, ch.order)
    shifted = list(args)
    shifted[2] = ch.fl + H @ b
    marg = np.max(np.abs(mp.marg_predict_ext(*shifted).mu - mp.pcase_ext(pc, "one").mu))
    plain = np.max(np.abs(mp.plain_predict_ext(*shifted[:7])[0] - mp.plain_predict_ext(*args[:7])[0]))
    print("shift of the mean: marginal", float(marg), "plain", float(plain))
    assert marg < plain
