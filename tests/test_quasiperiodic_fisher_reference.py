"""CPU checks of the references for the Fisher information and the leave-one-out under the quasi-periodic kernel
(tests/quasiperiodic_fisher_reference.py) that tests/test_gpu_quasiperiodic_fisher.py is measured against, and of the algebra of
``covariance.quasiperiodic_laplace`` and ``covariance.periodicity_score`` on the float64 twin.

The Gamma and P columns of K_t are checked against something that does not share their derivation: the central difference of
``quasiperiodic_reference.matrix_ext`` in Gamma_c and P_c at two steps.  A central difference is second order, so halving the
step divides its discrepancy from the analytic K_t by 4 (between 3 and 5 here); a wrong term leaves one that does not fall.

The bound on F is the one the GPU test uses -- 8 x the largest error of the float64 twin against the long-double reference
(python tests/quasiperiodic_fisher_reference.py) -- and seven seeded defects of K_t or of the contraction show that it rejects a
wrong formula.  The smallest factor by which a defect leaves the bound is 1.98e+13 (the sign of the Gamma term; the others
4.98e+13 .. 8.44e+18, and inf where a row that must be exactly zero is not); the test asks for 1e10, three decades below it.
"""
import numpy as np
import pytest

import quasiperiodic_fisher_reference as qf
import quasiperiodic_reference as qr

_LD = np.longdouble
MARGIN = 8
TOL = {"F": MARGIN * 7.52e-15, "mu": MARGIN * 3.50e-16}        # tests/test_gpu_quasiperiodic_fisher.py: the table's last row
DEFECT_FLOOR = 1e10


def _case(name):
    return next(c for c in qf.CASES if qf.case_id(c) == name)


def test_the_cases_are_the_quasiperiodic_references_without_n520_and_the_tangents_cover_every_direction():
    assert [qf.case_id(c) for c in qf.CASES] == ["N100-c2", "N128-c2", "N129-c2", "N300-c1", "N300-c2", "N300-c3", "N300-c2-perm"]
    for case in qf.CASES:
        tan_lwl, tan_gp, tan_tau, tan_gamma, tan_period = qf.case_tangents(case)
        c = case[1][1]
        assert tan_gp.shape == (8, 2 * c) and all(a.shape == (8, c) for a in (tan_tau, tan_gamma, tan_period))
        assert all(np.any(a[2]) for a in (tan_lwl, tan_gp, tan_tau, tan_gamma, tan_period))                 # the mixed tangent
        for t, own in ((4, tan_gamma), (5, tan_period), (6, tan_period)):                                 # the pure ones
            assert np.count_nonzero(own[t]) == 1
            assert not any(np.any(a[t]) for a in (tan_lwl, tan_gp, tan_tau, tan_gamma, tan_period) if a is not own)
    assert abs(MARGIN * max(r[1] for r in qf.measure_f64()) - TOL["F"]) <= 0.01 * TOL["F"]      # the quoted table is this build's


@pytest.mark.parametrize("case", qf.CASES, ids=qf.case_id)
@pytest.mark.parametrize("what", ["gamma", "period"])
def test_gamma_and_period_columns_of_the_tangent_matrix_are_derivatives_of_matrix_ext(case, what):
    d = qf.case_data(case)
    c, N = d.lwls.shape
    zc, zx, z2 = np.zeros(c), np.zeros((c, N)), np.zeros(2 * c)
    for k in range(c):
        unit = np.zeros(c)
        unit[k] = 1.0
        dgam, dper = (unit, zc) if what == "gamma" else (zc, unit)
        Kt = qf.tangent_matrix_qp(d.lwls, d.times, d.gp, d.tau, d.gamma, d.period, zx, z2, zc, dgam, dper, _LD)
        assert np.array_equal(Kt, Kt.T)
        if what == "period" and d.gamma[k] == 0.0:
            assert np.all(Kt == 0)                     # Gamma = 0: K does not depend on P
            continue
        assert np.max(np.abs(Kt)) > 0

        def discrepancy(h):
            up, dn = [v.astype(_LD) for v in (d.gamma, d.period)], [v.astype(_LD) for v in (d.gamma, d.period)]
            i = 0 if what == "gamma" else 1
            up[i][k], dn[i][k] = up[i][k] + _LD(h), dn[i][k] - _LD(h)
            diff = (qr.matrix_ext(d.lwls, d.times, d.gp, d.tau, *up) - qr.matrix_ext(d.lwls, d.times, d.gp, d.tau, *dn)) / \
                (_LD(2) * _LD(h))
            return float(np.max(np.abs(diff - Kt)))

        # (a period 20-30 x shorter than the span: the phase moves by pi dt / P^2 h, which must stay small over the span)
        h = 0.05 if what == "gamma" else 1e-3 * d.period[k] * min(1.0, d.period[k] / d.span)
        e1, e2 = discrepancy(h), discrepancy(h / 2)
        print(f"{qf.case_id(case)} {what}_{k}: max |K_t| {float(np.max(np.abs(Kt))):.3e}, discrepancy {e1:.3e} at h, {e2:.3e} at h/2, "
              f"ratio {e1 / e2:.3f}")
        assert 3.0 <= e1 / e2 <= 5.0, (k, e1, e2)


@pytest.mark.parametrize("case", qf.CASES, ids=qf.case_id)
def test_float64_twin_within_the_derived_bound_of_the_long_double_reference(case):
    d = qf.case_data(case)
    F, F_mu = qf.case_ext(case)
    f, f_mu = qf.fisher_qp_f64(d.lwls, d.times, d.sigma, d.gp, d.tau, d.gamma, d.period, *qf.case_tangents(case))
    err = {"F": qf.rel_to_scale(f, F), "mu": float(abs(_LD(f_mu) - F_mu) / F_mu)}
    print(f"{qf.case_id(case)}: " + ", ".join(f"{k} {v:.2e} (bound {TOL[k]:.2e})" for k, v in err.items()))
    assert err["F"] <= TOL["F"] and err["mu"] <= TOL["mu"]
    assert np.array_equal(F, F.T) and F_mu > 0
    # the period of a component with Gamma = 0 carries no information (tangent 6: dP of the last component)
    assert (d.gamma[-1] == 0.0) == bool(np.all(F[6] == 0)) == bool(np.all(f[6] == 0))
    assert F[4, 4] > 0 and F[5, 5] > 0


@pytest.mark.parametrize("name", ["N129-c2", "N300-c2-perm"])
def test_float64_leave_one_out_twin_within_its_printed_bound(name):
    import loo_reference as lr
    rows = dict(qf.measure_loo_f64())
    quoted = {"pix_mean": 7.22e-15, "pix_var": 1.38e-13, "pix_logp": 3.04e-13, "loo_logp": 3.00e-15, "ep_resid": 5.38e-15,
              "ep_chi2": 2.54e-14, "ep_logp": 4.41e-15}
    for k in lr.OUTPUTS:
        assert rows[name][k] <= 1.01 * quoted[k], (k, rows[name][k])


def test_gamma_zero_twin_is_the_time_variable_twin():
    """with every Gamma = 0 and no Gamma part the covariance derivatives ARE ``timevar_fisher_reference.tangent_matrix_tv``'s
    whatever the periods and their tangents hold"""
    import timevar_fisher_reference as tf
    case = _case("N300-c3")
    d = qf.case_data(case)
    c = 3
    tan_lwl, tan_gp, tan_tau, _g, tan_period = qf.case_tangents(case)
    for t in range(8):
        a = qf.tangent_matrix_qp(d.lwls, d.times, d.gp, d.tau, np.zeros(c), d.period, tan_lwl[t], tan_gp[t], tan_tau[t], np.zeros(c),
                                 tan_period[t] + 1.0)
        b = tf.tangent_matrix_tv(d.lwls, d.times, d.gp, d.tau, tan_lwl[t], tan_gp[t], tan_tau[t])
        assert np.array_equal(a, b), t


@pytest.mark.parametrize("defect", qf.DEFECTS)
def test_a_seeded_defect_is_rejected_by_the_bound(defect):
    factor = qf.defect_factor(defect)
    print(f"{defect}: leaves the bound of F by a factor of {factor:.3g}")
    assert factor >= DEFECT_FLOOR


# ---- the algebra of quasiperiodic_laplace and periodicity_score on the twin ----------------------------------------------
def _unit_fisher(case):
    d = qf.case_data(case)
    c, N = d.lwls.shape
    eye = np.eye(5 * c)
    F = qf.fisher_qp_f64(d.lwls, d.times, d.sigma, d.gp, d.tau, d.gamma, d.period, np.zeros((5 * c, c, N)), eye[:, :2 * c],
                         eye[:, 2 * c:3 * c], eye[:, 3 * c:4 * c], eye[:, 4 * c:])[0]
    return d, c, F


def test_laplace_restricts_f_log_and_transforms_the_standard_deviations_back():
    from psoap_amd import covariance
    d, c, F = _unit_fisher(_case("N300-c3"))      # tau = (0.25 span, inf, 2 span), Gamma = (1, 2.5, 0)
    cov, sd_gp, sd_tau, sd_gamma, sd_period = covariance._qp_laplace_from_fisher(F, d.gp, d.tau, d.gamma, d.period, None)
    idx = np.array([0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 13])      # gp; tau_0, tau_2; Gamma_0, Gamma_1; P_0, P_1
    theta = np.concatenate([d.gp, d.tau, d.gamma, d.period])[idx]
    F_log = theta[:, None] * F[np.ix_(idx, idx)] * theta[None, :]
    assert cov.shape == (12, 12)
    np.testing.assert_allclose(cov @ F_log, np.eye(12), atol=1e-8)
    sd = theta * np.sqrt(np.diag(cov))
    np.testing.assert_allclose(np.concatenate([sd_gp, sd_tau[[0, 2]], sd_gamma[:2], sd_period[:2]]), sd, rtol=1e-12)
    assert np.isnan(sd_tau[1]) and np.isnan(sd_gamma[2]) and np.isnan(sd_period[2])
    # the marginal error bar is never below the conditional one
    assert np.all(sd >= theta / np.sqrt(np.diag(F_log)) * (1 - 1e-12))
    # `free` follows _fit_quasiperiodic's dictionary: the period of component 1 held
    held = covariance._qp_laplace_from_fisher(F, d.gp, d.tau, d.gamma, d.period, {"period": [True, False, False]})
    assert held[0].shape == (11, 11) and np.isnan(held[4][1]) and held[4][0] <= sd_period[0] * (1 + 1e-12)
    with pytest.raises(ValueError, match="free takes"):
        covariance._qp_laplace_from_fisher(F, d.gp, d.tau, d.gamma, d.period, {"P": [True] * 3})
    # a free period of a component with Gamma = 0: its row of F is exactly zero
    assert np.all(F[14] == 0)
    with pytest.raises(np.linalg.LinAlgError, match="quasiperiodic_laplace"):
        covariance._qp_laplace_from_fisher(F, d.gp, d.tau, d.gamma, d.period, {"period": [True, True, True]})
    with pytest.raises(np.linalg.LinAlgError):
        covariance._qp_laplace_from_fisher(np.full_like(F, np.nan), d.gp, d.tau, d.gamma, d.period, None)
    # with two blocks the general helper is _laplace_from_fisher
    a = covariance._laplace_from_fisher(F[:9, :9], d.gp, d.tau, np.isfinite(d.tau))
    b = covariance._laplace_from_fisher_blocks(F[:9, :9], np.concatenate([d.gp, d.tau]),
                                               np.concatenate([np.ones(6, dtype=bool), np.isfinite(d.tau)]), "x")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1][:6]) and np.array_equal(a[2], b[1][6:], equal_nan=True)


def test_the_efficient_information_is_the_schur_complement():
    from psoap_amd import covariance
    rng = np.random.default_rng(31)
    A = rng.standard_normal((7, 7)) * np.logspace(-3, 3, 7)[None, :]
    F = A.T @ A
    z, S, I = covariance._periodicity_from_fisher(2.5, F)
    schur = F[6, 6] - F[6, :6] @ np.linalg.solve(F[:6, :6], F[:6, 6])
    np.testing.assert_allclose(I, schur, rtol=1e-8)
    np.testing.assert_allclose(I, 1.0 / np.linalg.inv(F)[6, 6], rtol=1e-8)
    assert S == 2.5 and z == pytest.approx(2.5 / np.sqrt(schur), rel=1e-8) and 0 < I <= F[6, 6]
    tan_gp, tan_tau, tan_gamma = covariance._periodicity_tangents(3, np.array([True, False, True]), 1)
    assert tan_gp.shape == (9, 6) and np.array_equal(tan_gp[:6], np.eye(6)) and not np.any(tan_gp[6:])
    assert np.array_equal(np.argwhere(tan_tau), [[6, 0], [7, 2]]) and np.array_equal(np.argwhere(tan_gamma), [[8, 1]])
    with pytest.raises(np.linalg.LinAlgError):
        covariance._periodicity_from_fisher(1.0, np.full((3, 3), np.nan))


def test_the_planted_period_lies_within_its_error_bar_and_the_score_tells_the_two_draws_apart():
    """the twin's fit and the twin's F (what the GPU test repeats on the device): |P_fit - 84.5907| < 5 sd_period; z at the
    planted period, at Gamma = 0 on the fit's (gp, tau), is large and positive on the planted draw and below 3 on the other"""
    from psoap_amd import covariance
    gp, tau, gamma, period = qr.fit_on_twin(True)[:4]
    F = qf.fit_fisher_twin(True, gp, tau, gamma, period)
    _cov, _sd_gp, sd_tau, sd_gamma, sd_period = covariance._qp_laplace_from_fisher(F, gp, tau, gamma, period, None)
    print(f"P_0 {period[0]:.6f} +- {sd_period[0]:.6f}, Gamma_0 {gamma[0]:.6f} +- {sd_gamma[0]:.6f}, tau_0 {tau[0]:.4f} +- {sd_tau[0]:.4f}")
    assert abs(period[0] - 84.5907) < 5 * sd_period[0] and 0.2 < sd_period[0] < 0.8
    assert np.all(F[9] == 0) and np.all(F[5] == 0)      # P_1 (Gamma_1 = 0) and tau_1 = inf
    z = {}
    for planted in (True, False):
        g, t = qr.fit_on_twin(planted)[:2]
        z[planted], S, I = qf.score_twin(planted, g, t, qr.fit_case(planted).P0)
        print(f"{'planted' if planted else 'Gamma = 0 draw'}: z {z[planted]:+.4f}  S {S:+.6e}  I {I:.6e}")
    assert z[True] > 5.0 and z[False] < 3.0
    assert z[True] == pytest.approx(1488.149, rel=1e-4) and z[False] == pytest.approx(-1.8246, rel=1e-3)
