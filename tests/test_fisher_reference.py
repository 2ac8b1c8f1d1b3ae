"""CPU checks of the Fisher-information references (tests/fisher_reference.py) that the GPU tests are measured against.

The formula of the covariance derivative K_t is checked against something that does not share its derivation: the central
difference of the ORACLE's fill along the tangent.  A central difference is second order, so halving the step divides its
discrepancy from the analytic K_t by 4 (between 3 and 5 here); a wrong term in K_t leaves a discrepancy that does not fall.
(Along an amplitude K is a quadratic and the central difference is exact: there the discrepancy must be rounding alone.)
The same criterion checks the composition of grid tangents with the orbit Jacobian against differenced oracle velocities.
"""
import numpy as np
import pytest

import fisher_reference as fr
from psoap_amd import synthetic as syn


def _fill(oracle, lwls, gp):
    K = np.empty((lwls.shape[1],) * 2)
    oracle.fill_sym(K, np.ascontiguousarray(lwls), np.asarray(gp, dtype=np.float64))
    return K


@pytest.mark.parametrize("case", fr.CASES, ids=fr.case_id)
def test_tangent_matrix_is_the_derivative_of_the_oracles_fill(oracle, case):
    ch, gp = fr.case_chunk(case), fr.case_gp(case)
    tan_lwl, tan_gp = fr.case_tangents(case)
    for t in range(tan_gp.shape[0]):
        Kt = fr.tangent_matrix(ch.lwls, gp, tan_lwl[t], tan_gp[t])
        assert np.array_equal(Kt, Kt.T) and np.max(np.abs(Kt)) > 0

        def discrepancy(h):
            up = _fill(oracle, ch.lwls + h * tan_lwl[t], gp + h * tan_gp[t])
            dn = _fill(oracle, ch.lwls - h * tan_lwl[t], gp - h * tan_gp[t])
            return np.max(np.abs((up - dn) / (2 * h) - Kt))

        h = fr.fd_step(case, t)
        e1, e2 = discrepancy(h), discrepancy(h / 2)
        print(f"{fr.case_id(case)} tangent {t}: max |K_t| {np.max(np.abs(Kt)):.3e}, discrepancy {e1:.3e} at h, {e2:.3e} at h/2, "
              f"ratio {e1 / e2:.3f}")
        if t < 2 * case[1] and t % 2 == 0:
            # K is quadratic in an amplitude: the central difference is EXACT at any step and there is no truncation error
            # to fall -- what is left is the rounding of the two fills, eps max|K| each, over 2 h (a margin of 8)
            bound = 8 * np.finfo(np.float64).eps * np.max(np.abs(_fill(oracle, ch.lwls, gp))) / h
            assert e1 <= bound and e2 <= bound, (t, e1, e2, bound)
        else:
            assert 3.0 <= e1 / e2 <= 5.0, (t, e1, e2)


@pytest.mark.parametrize("case", fr.CASES, ids=fr.case_id)
def test_fisher_is_symmetric_and_positive_semi_definite(case):
    ch = fr.case_chunk(case)
    F_ext, F_mu = fr.case_ext(case)
    F64, f_mu = fr.fisher_f64(ch.lwls, ch.sigma, fr.case_gp(case), *fr.case_tangents(case))
    assert F_mu > 0 and f_mu > 0
    for F in (np.asarray(F_ext, dtype=np.float64), F64):
        scale = np.max(np.diag(F))
        assert np.max(np.abs(F - F.T)) <= 1e-12 * scale
        low = np.min(np.linalg.eigvalsh(0.5 * (F + F.T)))
        print(f"{fr.case_id(case)}: smallest eigenvalue {low:.3e}, largest diagonal entry {scale:.3e}")
        assert low >= -1e-12 * scale
    assert np.array_equal(F_ext, F_ext.T)


def test_tangents_through_the_orbit_jacobian_match_differenced_oracle_velocities(oracle):
    """SB2 with e = 0.25, one epoch table, N = 100: F from the analytic K_t of the tangents dx_i = -J[c, epoch, i] / c_kms
    (the long-double Jacobian of tests/orbit_grad_reference.py) against F from central differences of the fill on grids
    shifted by the velocities of oracle/orbit_oracle.py.  gamma moves every grid alike and leaves K as it is: its row of F
    is exactly zero and it takes no part in the comparison."""
    import orbit_grad_reference as ogr
    import orbit_oracle
    model, case = "SB2", fr.CASES[0]
    assert case[0] == 100
    ch, gp = fr.case_chunk(case), fr.case_gp(case)
    p = np.array(syn.ORBIT_BASE[model], dtype=np.float64)
    assert p[2] > 0.2                                  # an eccentric orbit
    ep, n_orb = ch.epoch_index, p.shape[0]

    def grids(q):
        return ch.lwl[None, :] - orbit_oracle.velocities(model, q, ch.dates)[:, ep] / fr.C_KMS

    base = grids(p)
    K = _fill(oracle, base, gp)
    K[np.diag_indices_from(K)] += ch.sigma ** 2
    J, _ = ogr.jacobian_ext(model, p, ch.dates)       # (c, n_epochs, n_orb)
    tan = np.asarray(-np.moveaxis(J, 2, 0)[:, :, ep] / np.longdouble(fr.C_KMS), dtype=np.float64)
    Kt = [fr.tangent_matrix(base, gp, tan[i], np.zeros(4)) for i in range(n_orb)]
    assert np.all(Kt[n_orb - 1] == 0.0)               # gamma
    live = list(range(n_orb - 1))
    F, _ = fr.fisher_from_matrices(K, [Kt[i] for i in live])
    # steps: 0.25 % of q, K, e; a quarter of a degree; 0.0025 day in P and T0
    steps = 0.25 * np.array([0.01 * p[0], 0.01 * p[1], 0.01 * p[2], 1.0, 0.01, 0.01])

    def differenced(scale):
        out = []
        for i in live:
            dq = np.zeros(n_orb)
            dq[i] = scale * steps[i]
            out.append((_fill(oracle, grids(p + dq), gp) - _fill(oracle, grids(p - dq), gp)) / (2 * dq[i]))
        return fr.fisher_from_matrices(K, out)[0]

    e1, e2 = fr.rel_to_scale(differenced(1.0), F), fr.rel_to_scale(differenced(0.5), F)
    print(f"max |F_fd - F| / sqrt(F_ss F_tt): {e1:.3e} at h, {e2:.3e} at h/2, ratio {e1 / e2:.3f}")
    assert 3.0 <= e1 / e2 <= 5.0
