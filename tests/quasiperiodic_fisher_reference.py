"""CPU references for the Fisher information and the leave-one-out under the quasi-periodic kernel
(tests/test_quasiperiodic_fisher_reference.py, tests/test_gpu_quasiperiodic_fisher.py), modelled on
tests/timevar_fisher_reference.py and tests/quasiperiodic_reference.py.

    K[m,n] = sum_c a_c^2 e + sigma_m^2 delta_mn,   e = exp(p_c d^2 + q_c dt^2 - Gamma_c s^2),   s, co = sin, cos(pi dt / P_c)

A tangent t is a direction (dx_t (c, N), da_tc, dl_tc, dtau_tc, dGamma_tc, dP_tc):

    K_t[m,n] = sum_c e (2 a_c da_tc + a_c^2 c_kms^2 / l_c^3 d^2 dl_tc + a_c^2 2 p_c d (dx_tc[n] - dx_tc[m])
                        + a_c^2 / tau_c^3 dt^2 dtau_tc - a_c^2 s^2 dGamma_tc + a_c^2 Gamma_c pi / P_c^2 dt (2 s co) dP_tc)
    F_st     = 1/2 tr(K^-1 K_s K^-1 K_t)            F_mu = 1^T K^-1 1

``fisher_qp_ext`` in np.longdouble on ``quasiperiodic_reference.matrix_ext`` and the oracle's long-double Cholesky;
``fisher_qp_f64`` its float64 twin on ``quasiperiodic_reference.matrix_f64`` -- the device's argument order -- through
``fisher_reference.fisher_from_matrices``.  The twin takes a ``defect``, one of DEFECTS.  ``loo_qp_ext`` and ``loo_qp_f64`` run
the closed forms of tests/loo_reference.py on the same two matrices.

Run as a script it prints, per case, max_st |f64 - long double| / sqrt(F_ss F_tt) and |f64 - long double| / F_mu, the
leave-one-out errors in the units of tests/test_gpu_loo.py, and the factor by which every seeded defect leaves the bound: the
tables from which tests/test_gpu_quasiperiodic_fisher.py takes its bounds.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import fisher_reference as fr  # noqa: E402  (puts the oracle and the repository on the path)
import loo_reference as lr  # noqa: E402
import quasiperiodic_reference as qr  # noqa: E402
import timevar_fisher_reference as tf  # noqa: E402

_LD = np.longdouble
C_KMS = fr.C_KMS
MU_GP = qr.MU_GP
MARGIN = 8

# quasiperiodic_reference's cases without N = 520: one tile, exactly one tile, one tile plus one row, three ragged tiles, and
# the pixels of N = 300 in no time order
CASES = tuple(case for case in qr.CASES if case[1][0] != 520)
case_id, case_data = qr.case_id, qr.case_data
case_epochs = tf.case_epochs
rel_to_scale = tf.rel_to_scale

DEFECTS = ("sin_for_sin2",         # sin in place of sin^2 in the Gamma term of K_t
           "two_pi",               # 2 pi in place of pi in the dP coefficient
           "gamma_missing",        # Gamma missing from the dP coefficient
           "p_for_p2",             # 1 / P in place of 1 / P^2 in the dP coefficient
           "wrong_component",      # the next component's P in the phase of the tangent's terms
           "gamma_sign",           # the sign of the Gamma term
           "tv_e_contract")        # the time-variable e (no periodic term) in the contraction


def tangent_matrix_qp(lwls, times, gp, tau, gamma, period, dx, dgp, dtau, dgam, dper, T=np.float64, defect=None):
    """K_t (N, N) of one tangent in the number type ``T``; in float64 the argument of exp() in the device's order (p * d * d,
    + q * dt * dt, + (-Gamma) * s * s with s, co = sincospi(dt * (1 / P)))"""
    lwls = np.atleast_2d(lwls)
    c, N = lwls.shape
    ckms = T("2.99792458e5") if T is _LD else T(C_KMS)
    pi = qr._PI_LD if T is _LD else T(np.pi)
    t = np.asarray(times, dtype=T)
    DT = t[None, :] - t[:, None]
    out = np.zeros((N, N), dtype=T)
    with np.errstate(under="ignore"):
        for k in range(c):
            a, l, tk, gk, pk = T(gp[2 * k]), T(gp[2 * k + 1]), T(tau[k]), T(gamma[k]), T(period[k])
            da, dl, dtk, dgk, dpk = T(dgp[2 * k]), T(dgp[2 * k + 1]), T(dtau[k]), T(dgam[k]), T(dper[k])
            x, u = np.asarray(lwls[k], dtype=T), np.asarray(dx[k], dtype=T)
            D = x[None, :] - x[:, None]
            p = T(-0.5) * ckms * ckms / (l * l)
            q = T(-0.5) / (tk * tk)
            S, Co = qr._phase(DT, period[k], T, None, k, period)
            A = p * D * D
            A = A + q * DT * DT
            if defect != "tv_e_contract":
                A = A + (-gk) * S * S
            E = np.exp(A)
            St, Cot = S, Co       # the phase of the tangent's own terms
            if defect == "wrong_component":
                St, Cot = qr._phase(DT, period[(k + 1) % c], T, None, k, period)
            cg = -(a * a) * dgk
            if defect == "gamma_sign":
                cg = -cg
            cp = a * a * (T(1) if defect == "gamma_missing" else gk) * (T(2) * pi if defect == "two_pi" else pi) / \
                (pk if defect == "p_for_p2" else pk * pk) * dpk
            out += E * (T(2) * a * da + a * a * (ckms * ckms) / (l * l * l) * (D * D) * dl
                        + a * a * T(2) * p * D * (u[None, :] - u[:, None]) + a * a / (tk * tk * tk) * dtk * (DT * DT)
                        + cg * (St if defect == "sin_for_sin2" else St * St) + cp * (DT * (T(2) * St * Cot)))
    return out


def fisher_qp_ext(lwls, times, sigma, gp, tau, gamma, period, tan_lwl, tan_gp, tan_tau, tan_gamma, tan_period):
    """(F (T, T), F_mu) with every step in long double"""
    import oracle
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    N = lwls.shape[1]
    K = qr.matrix_ext(lwls, times, gp, tau, gamma, period)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=_LD) ** 2
    L = oracle._chol_ext(K)
    Li = oracle._fsolve_ext(L, np.eye(N, dtype=_LD))          # L^-1
    P = [Li @ tangent_matrix_qp(lwls, times, gp, tau, gamma, period, *tan, T=_LD) @ Li.T
         for tan in zip(tan_lwl, tan_gp, tan_tau, tan_gamma, tan_period)]
    T = len(P)
    F = np.zeros((T, T), dtype=_LD)
    for s in range(T):
        for t in range(s, T):
            F[s, t] = F[t, s] = _LD(0.5) * np.sum(P[s] * P[t])
    y = Li @ np.ones(N, dtype=_LD)
    return F, y @ y


_IN_CONTRACTION = ("tv_e_contract",)


def fisher_qp_f64(lwls, times, sigma, gp, tau, gamma, period, tan_lwl, tan_gp, tan_tau, tan_gamma, tan_period, defect=None):
    """the same in float64: ``quasiperiodic_reference.matrix_f64``, then ``fisher_reference.fisher_from_matrices``.  With a
    ``defect`` of the contraction, F_st = 1/2 sum K_s G_t takes its K_s from the defective formula and G_t from the sound one."""
    assert defect is None or defect in DEFECTS
    lwls = np.ascontiguousarray(np.atleast_2d(lwls), dtype=np.float64)
    K = qr.matrix_f64(lwls, times, gp, tau, gamma, period, sigma)
    tans = list(zip(tan_lwl, tan_gp, tan_tau, tan_gamma, tan_period))
    fill_defect = None if defect in _IN_CONTRACTION else defect
    Kt = [tangent_matrix_qp(lwls, times, gp, tau, gamma, period, *tan, defect=fill_defect) for tan in tans]
    F, F_mu = fr.fisher_from_matrices(K, Kt)
    if defect in _IN_CONTRACTION:
        from scipy.linalg import cho_factor, cho_solve
        Kinv = cho_solve(cho_factor(K, lower=False), np.eye(K.shape[0]))
        Ks = [tangent_matrix_qp(lwls, times, gp, tau, gamma, period, *tan, defect=defect) for tan in tans]
        F = np.array([[0.5 * np.sum(ks * (Kinv @ kt @ Kinv)) for kt in Kt] for ks in Ks])
    return F, F_mu


# ---- the leave-one-out on a given K ------------------------------------------------------------------------------------
def loo_qp_ext(lwls, times, fl, sigma, gp, tau, gamma, period, mu_GP=1.0, epoch_index=None, n_epochs=None) -> lr.Loo:
    """``loo_reference.loo_ext`` on ``quasiperiodic_reference.matrix_ext``: every step in long double"""
    import oracle
    K = qr.matrix_ext(lwls, times, gp, tau, gamma, period)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=_LD) ** 2
    N = K.shape[0]
    L = oracle._chol_ext(K)
    Li = oracle._fsolve_ext(L, np.eye(N, dtype=_LD))
    X = Li.T @ Li
    X = X + X @ (np.eye(N, dtype=_LD) - K @ X)          # Newton: the residual of the inverse squared
    A = _LD(0.5) * (X + X.T)
    r = np.asarray(fl, dtype=_LD) - _LD(mu_GP)
    z = Li @ r
    lnp = _LD(-0.5) * (z @ z + _LD(2) * np.sum(np.log(np.diag(L))))

    def solve_block(Aee, ae):
        Le = oracle._chol_ext(Aee)
        y = oracle._fsolve_ext(Le, ae)
        s = oracle._fsolve_ext(Le.T[::-1, ::-1], y[::-1])[::-1]
        return s, _LD(2) * np.sum(np.log(np.diag(Le)))

    if epoch_index is not None and n_epochs is None:
        n_epochs = int(np.max(epoch_index)) + 1
    return lr._finish(_LD, lnp, A, A @ r, fl, epoch_index, n_epochs, solve_block)


def loo_qp_f64(lwls, times, fl, sigma, gp, tau, gamma, period, mu_GP=1.0, epoch_index=None, n_epochs=None) -> lr.Loo:
    """``loo_reference.loo_f64`` on ``quasiperiodic_reference.matrix_f64``"""
    from scipy.linalg import cho_factor, cho_solve
    K = qr.matrix_f64(lwls, times, gp, tau, gamma, period, sigma)
    N = K.shape[0]
    factor = cho_factor(K, lower=False)
    r = np.asarray(fl, dtype=np.float64) - mu_GP
    alpha = cho_solve(factor, r)
    A = cho_solve(factor, np.eye(N))
    lnp = -0.5 * (r @ alpha + np.sum(2 * np.log(np.diag(factor[0]))))

    def solve_block(Aee, ae):
        f = cho_factor(Aee, lower=False)
        return cho_solve(f, ae), np.sum(2 * np.log(np.diag(f[0])))

    if epoch_index is not None and n_epochs is None:
        n_epochs = int(np.max(epoch_index)) + 1
    return lr._finish(np.float64, lnp, A, alpha, fl, epoch_index, n_epochs, solve_block)


# ---- the cases ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_tangents(case):
    """(tan_lwl (T, c, N), tan_gp (T, 2c), tan_tau, tan_gamma, tan_period (T, c)), T = 8, after the pattern of
    ``timevar_fisher_reference.case_tangents``: 0 the amplitude and 1 the length scale of component 0; 2 a MIXED tangent --
    every hyper-parameter, tau, Gamma and P of every component and a grid direction at once; 3 pure dtau of component 0;
    4 pure dGamma and 5 pure dP of the component with the largest Gamma; 6 pure dP of the LAST component (in four cases its
    Gamma is 0: an exactly-zero row and column); 7 a grid tangent.  tau = inf takes no finite step: its dtau is as written and
    its coefficient is 0."""
    d = case_data(case)
    c, N = d.lwls.shape
    t_lwl, _t_gp, _t_tau = tf.case_tangents(case)
    grid = t_lwl[3 * c:]
    T = 8
    tan_lwl, tan_gp = np.zeros((T, c, N)), np.zeros((T, 2 * c))
    tan_tau, tan_gamma, tan_period = np.zeros((T, c)), np.zeros((T, c)), np.zeros((T, c))
    k = int(np.argmax(d.gamma))
    tan_gp[0, 0] = 1.0
    tan_gp[1, 1] = 1.0
    tan_gp[2] = 0.3 * d.gp * np.where(np.arange(2 * c) % 2 == 0, 1.0, -0.5)
    tan_tau[2] = np.where(np.isfinite(d.tau), 0.2 * d.tau, 1.0)
    tan_gamma[2] = 0.25 + 0.1 * np.arange(c)
    tan_period[2] = 0.05 * d.period * np.where(np.arange(c) % 2 == 0, 1.0, -1.0)
    tan_lwl[2] = 0.5 * grid[0]
    tan_tau[3, 0] = 1.0
    tan_gamma[4, k] = 1.0
    tan_period[5, k] = 1.0
    tan_period[6, c - 1] = 1.0
    tan_lwl[7] = grid[1]
    out = (tan_lwl, tan_gp, tan_tau, tan_gamma, tan_period)
    for a in out:
        a.setflags(write=False)
    return out


def _hyper(d):
    return d.gp, d.tau, d.gamma, d.period


@functools.lru_cache(maxsize=None)
def case_ext(case):
    d = case_data(case)
    F, F_mu = fisher_qp_ext(d.lwls, d.times, d.sigma, *_hyper(d), *case_tangents(case))
    F.setflags(write=False)
    return F, F_mu


@functools.lru_cache(maxsize=None)
def case_loo_ext(case) -> lr.Loo:
    d = case_data(case)
    ep, ne = case_epochs(case)
    return loo_qp_ext(d.lwls, d.times, d.fl, d.sigma, *_hyper(d), MU_GP, ep, ne)


@functools.lru_cache(maxsize=None)
def measure_f64(defect=None):
    rows = []
    for case in CASES:
        d = case_data(case)
        F, F_mu = case_ext(case)
        f, f_mu = fisher_qp_f64(d.lwls, d.times, d.sigma, *_hyper(d), *case_tangents(case), defect=defect)
        rows.append((case_id(case), rel_to_scale(f, F), float(abs(_LD(f_mu) - F_mu) / F_mu)))
    return tuple(rows)


LOO_CASES = tuple(case for case in CASES if case_id(case) in ("N129-c2", "N300-c2-perm"))


@functools.lru_cache(maxsize=None)
def measure_loo_f64():
    rows = []
    for case in LOO_CASES:
        d = case_data(case)
        ep, ne = case_epochs(case)
        f = loo_qp_f64(d.lwls, d.times, d.fl, d.sigma, *_hyper(d), MU_GP, ep, ne)
        rows.append((case_id(case), lr.errors(f, case_loo_ext(case))))
    return tuple(rows)


def bound_F() -> float:
    """MARGIN x the twin's largest error of F over the cases, in units of sqrt(F_ss F_tt)"""
    return MARGIN * max(r[1] for r in measure_f64())


def defect_factor(defect) -> float:
    """by which factor the twin with ``defect`` seeded into it leaves ``bound_F`` (the largest over the cases; inf where a row
    that must be exactly zero is not)"""
    return max(r[1] for r in measure_f64(defect)) / bound_F()


# ---- the fit of quasiperiodic_reference.fit_case on the twin: error bars and the periodicity score -----------------------
def fit_fisher_twin(planted_fit: bool, gp, tau, gamma, period):
    """the twin's (5c, 5c) information, unit tangents in the order of ``covariance.fisher_information_quasiperiodic``"""
    fc = qr.fit_case(planted_fit)
    c, N = fc.lwls.shape
    eye = np.eye(5 * c)
    return fisher_qp_f64(fc.lwls, fc.t0, fc.sigma, gp, tau, gamma, period, np.zeros((5 * c, c, N)), eye[:, :2 * c],
                         eye[:, 2 * c:3 * c], eye[:, 3 * c:4 * c], eye[:, 4 * c:])[0]


def score_twin(planted_fit: bool, gp, tau, period, component=0, free_tau=None):
    """``covariance.periodicity_score`` on the twin -> (z, S, I)"""
    from psoap_amd import covariance
    fc = qr.fit_case(planted_fit)
    c, N = fc.lwls.shape
    tau = np.asarray(tau, dtype=np.float64)
    per = np.ones(c)
    per[component] = period
    zero = np.zeros(c)
    free = np.isfinite(tau) if free_tau is None else np.asarray(free_tau, dtype=bool)
    S = qr.qp_f64(fc.lwls, fc.t0, fc.fl, fc.sigma, gp, tau, zero, per, 1.0).gamma[component]
    tan_gp, tan_tau, tan_gamma = covariance._periodicity_tangents(c, free, component)
    T = tan_gp.shape[0]
    F = fisher_qp_f64(fc.lwls, fc.t0, fc.sigma, gp, tau, zero, per, np.zeros((T, c, N)), tan_gp, tan_tau, tan_gamma,
                      np.zeros((T, c)))[0]
    return covariance._periodicity_from_fisher(S, F)


@functools.lru_cache(maxsize=None)
def timevar_fit_on_twin(planted_fit: bool):
    """(gp, tau) of the time-variable model fitted to the draw on the twin (``covariance._fit_timevar`` at Gamma = 0 from the
    start of ``fit_case``): where the periodicity score is evaluated"""
    from psoap_amd import covariance
    fc = qr.fit_case(planted_fit)
    vg = qr.fit_twin(fc)
    zero, one = np.zeros(2), np.ones(2)
    gp, tau, _res = covariance._fit_timevar(lambda g, t: vg(g, t, zero, one)[:3], 2, fc.start[0], fc.start[1], None, 1e-10)
    return gp, tau


if __name__ == "__main__":
    rows = measure_f64()
    print(f"{'case':13s} {'F':>10s} {'F_mu':>10s}")
    for name, a, b in rows:
        print(f"{name:13s} {a:10.2e} {b:10.2e}")
    print(f"{'max':13s} " + " ".join(f"{max(r[k] for r in rows):10.2e}" for k in (1, 2)))
    print(f"{'bound (8 x)':13s} " + " ".join(f"{MARGIN * max(r[k] for r in rows):10.2e}" for k in (1, 2)))
    print()
    rows = measure_loo_f64()
    print(f"{'case':13s} " + " ".join(f"{k:>10s}" for k in lr.OUTPUTS))
    for name, err in rows:
        print(f"{name:13s} " + " ".join(f"{err[k]:10.2e}" for k in lr.OUTPUTS))
    print(f"{'max':13s} " + " ".join(f"{max(r[1][k] for r in rows):10.2e}" for k in lr.OUTPUTS))
    print()
    for name in DEFECTS:
        print(f"defect {name:16s} leaves the bound of F by a factor of {defect_factor(name):.3g}")
    print()
    from psoap_amd import covariance
    gp, tau, gamma, period = qr.fit_on_twin(True)[:4]
    F = fit_fisher_twin(True, gp, tau, gamma, period)
    _cov, sd_gp, sd_tau, sd_gamma, sd_period = covariance._qp_laplace_from_fisher(F, gp, tau, gamma, period, None)
    print(f"planted fit on the twin: P_0 {period[0]:.6f} +- {sd_period[0]:.6f}   Gamma_0 {gamma[0]:.6f} +- {sd_gamma[0]:.6f}   "
          f"tau_0 {tau[0]:.4f} +- {sd_tau[0]:.4f}   |P_fit - P_true| / sd {abs(period[0] - qr.fit_case(True).P0) / sd_period[0]:.3f}")
    for planted_fit in (True, False):
        what = "planted" if planted_fit else "Gamma = 0 draw"
        gp_f, tau_f = qr.fit_on_twin(planted_fit)[:2]
        z, S, I = score_twin(planted_fit, gp_f, tau_f, qr.fit_case(planted_fit).P0)
        print(f"periodicity score at P_0 on the fit's (gp, tau), {what}: z {z:+.4f}  S {S:+.6e}  I {I:.6e}")
        gp_tv, tau_tv = timevar_fit_on_twin(planted_fit)
        z, S, I = score_twin(planted_fit, gp_tv, tau_tv, qr.fit_case(planted_fit).P0)
        print(f"    ... on the re-fitted time-variable model (tau_0 {tau_tv[0]:.4f}), {what}: z {z:+.4f}  S {S:+.6e}  I {I:.6e}")
