"""CPU: the references of the continuum-marginalised likelihood (tests/marg_reference.py) against each other and against
their limits, before anything on the device is compared with them."""
import numpy as np
import pytest

import marg_reference as mr

_LD = np.longdouble


@pytest.mark.parametrize("kind", mr.WEIGHTS)
@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_id)
def test_woodbury_route_and_dense_route_agree(case, kind):
    """marg_f64 (U^-T Ht, M = I + W^T W, ...) against marg_ext (the dense K + H Lambda H^T in long double): float64 rounding
    only.  The bounds are loose here -- the table tests/test_gpu_marg.py derives its tolerances from is `python
    tests/marg_reference.py`"""
    err = mr.errors(mr.marg_f64(*mr._case_args(case, kind)), mr.case_ext(case, kind), mr.prior_sd(case[5]))
    assert err["lnp"] < 1e-11 and err["quad"] < 1e-11 and err["logdet_K"] < 1e-11, err
    assert err["gain"] < 1e-9 and err["logdet_M"] < 1e-9, err
    assert err["beta"] < 1e-9 and err["beta_cov"] < 1e-9 and err["fl_cor"] < 1e-9, err


@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_id)
def test_vanishing_prior_reproduces_the_plain_likelihood(case):
    import oracle
    ch = mr.case_chunk(case)
    gp = mr.case_gp(case)
    sd = np.full(ch.order + 1, 1e-12)
    plain = oracle.lnlike(ch.lwls, ch.fl, ch.sigma, gp, mr.MU_GP)
    for kind in mr.WEIGHTS:
        w = mr.case_weight(case, kind)
        for fn in (mr.marg_f64, mr.marg_ext):
            m = fn(ch.lwls, ch.fl, ch.sigma, gp, ch.x, ch.epoch_index, ch.n_epochs, ch.order, sd, w, mr.MU_GP)
            assert abs(float(m.lnp) - plain) <= 1e-10 * max(1.0, abs(plain)), (fn.__name__, kind)


def test_an_empty_epoch_contributes_exactly_nothing():
    """case e with and without the columns of its empty epoch (id 1): the same likelihood to the last bit of the long double,
    mean 0 and covariance Lambda for the empty epoch's coefficients"""
    case = mr.case_named("e")
    ch = mr.case_chunk(case)
    gp, sd = mr.case_gp(case), mr.prior_sd(ch.order)
    full = mr.case_ext(case, "one")
    ep = np.asarray(ch.epoch_index).copy()
    assert not np.any(ep == 1)
    ep[ep > 1] -= 1
    less = mr.marg_ext(ch.lwls, ch.fl, ch.sigma, gp, ch.x, ep, ch.n_epochs - 1, ch.order, sd, None, mr.MU_GP)
    assert full.lnp == less.lnp
    assert np.all(full.beta[1] == 0)
    k = ch.order + 1
    assert np.array_equal(full.beta_cov[k:2 * k, k:2 * k], np.diag(np.asarray(sd, dtype=_LD) ** 2))
    assert np.all(full.beta_cov[k:2 * k, :k] == 0) and np.all(full.beta_cov[k:2 * k, 2 * k:] == 0)
    assert np.array_equal(np.delete(full.beta, 1, axis=0), less.beta)


@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_id)
def test_basis_is_numpy_chebyshev_with_per_epoch_domains(case):
    from numpy.polynomial import Chebyshev
    ch = mr.case_chunk(case)
    H = mr.basis(ch.x, ch.epoch_index, ch.n_epochs, ch.order, ch.fl)
    want = np.zeros_like(H)
    for e in range(ch.n_epochs):
        I = np.flatnonzero(ch.epoch_index == e)
        if I.size == 0:
            continue
        for k in range(ch.order + 1):
            want[I, e * (ch.order + 1) + k] = ch.fl[I] * Chebyshev.basis(k, domain=[ch.x[I].min(), ch.x[I].max()])(ch.x[I])
    # (numpy evaluates by Clenshaw's recurrence, the basis by the three-term one: rounding of u ~ 1e-11 times T_k' <= k^2)
    assert np.max(np.abs(H - want)) < 1e-9
    first = np.asarray(ch.epoch_index) == ch.epoch_index[0]          # T_0 = 1: the weight itself, and nothing outside the epoch
    col = int(ch.epoch_index[0]) * (ch.order + 1)
    assert np.array_equal(H[first, col], ch.fl[first]) and not np.any(H[~first, col])


def test_one_pixel_epoch_maps_to_zero():
    H = mr.basis(np.array([8.5, 8.6, 8.7]), np.array([0, 1, 1]), 2, 2)
    assert np.array_equal(H[0], [1.0, 0.0, -1.0, 0.0, 0.0, 0.0])
    assert np.allclose(H[1:, 3:], [[1.0, -1.0, 1.0], [1.0, 1.0, 1.0]], atol=1e-12)


def test_planted_tilt_is_recovered_by_the_reference():
    ch, gp, beta = mr.planted()
    m = mr.marg_ext(ch.lwls, ch.fl, ch.sigma, gp, ch.x, ch.epoch_index, ch.n_epochs, ch.order, mr.PLANT_SD, None, mr.MU_GP)
    sd_post = np.sqrt(np.diag(m.beta_cov).astype(np.float64)).reshape(beta.shape)
    assert np.all(np.abs(np.asarray(m.beta, dtype=np.float64) - beta) < 4.0 * sd_post)
    assert np.all(sd_post < np.asarray(mr.PLANT_SD))          # the data say something about every coefficient
    assert float(m.lnp) > float(mr.plain_ext(ch.lwls, ch.fl, ch.sigma, gp, mr.MU_GP))
