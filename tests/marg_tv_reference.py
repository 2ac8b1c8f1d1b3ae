"""CPU references for the time-variable kernel under the marginalised continuum (tests/test_marg_tv_reference.py,
tests/test_gpu_marg_timevar.py): tests/timevar_reference.py composed with tests/marg_reference.py.

    Kt = K_tv + H Lambda H^T,   K_tv,ij = sum_c a_c^2 exp(p_c d_cij^2 + q_c dt_ij^2) + sigma_i^2 delta_ij
    lnL = -1/2 (r^T Kt^-1 r + log det Kt),  r = fl - mu_GP

H does not depend on tau, so with alpha_m = Kt^-1 r and Q_m = alpha_m alpha_m^T - Kt^-1 every derivative is the one of
tests/timevar_reference.py with Q_m and alpha_m; in particular dlnL/dtau_c = 1/2 a_c^2 / tau_c^3 sum_ij Q_m,ij e_cij dt_ij^2.
A tangent is (dx (c, N), dgp (2c,), dtau (c,)) and F_st = 1/2 tr(Kt^-1 K_s Kt^-1 K_t) with the K_t of
tests/timevar_fisher_reference.py.

``marg_tv_ext`` builds the dense Kt in np.longdouble (``timevar_reference.matrix_ext`` + ``marg_reference.basis``) and inverts
it through the oracle's long-double Cholesky: no Woodbury identity.  ``marg_tv_f64`` is the device's route in float64 with
SciPy on ``timevar_reference.matrix_f64``: Wi = U^-T, Wh = U^-T Ht, M = I + Wh^T Wh = U_M^T U_M, Vt = U_M^-T Wh^T Wi,
Kt^-1 = Wi^T Wi - Vt^T Vt, alpha_m = Wi^T (z - Wh M^-1 Wh^T z).  Both return a ``MargTv``: the value, parts, beta, beta_cov and
fl_cor, the four gradients with their cancellation scales, and the (3c, 3c) Fisher matrix of (gp, tau).

The cases are ``marg_reference.CASES`` a-f with both ``WEIGHTS``; t_i is the date of pixel i's epoch minus the earliest date,
the dates those of the generated chunk the case is cut from; tau per component from ``timevar_reference._TAU``'s fractions of
the span (0.25, 2) with ``inf`` mixed in where c > 1.

Run as a script it prints, per case and weight, the error of ``marg_tv_f64`` against ``marg_tv_ext`` in the measures of
tests/test_gpu_marg.py (value side), tests/test_gpu_marg_grad.py / tests/test_gpu_timevar.py (gradients, relative to the
cancellation scale S) and tests/test_gpu_timevar_fisher.py (F relative to sqrt(F_ss F_tt)): the table from which
tests/test_gpu_marg_timevar.py takes its bounds; then the smallest error each seeded defect of the twin leaves.
"""
from __future__ import annotations

import functools
import os
import sys
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import grad_reference as gr  # noqa: E402  (puts the oracle and the repository on the path)
import marg_reference as mr  # noqa: E402
import timevar_fisher_reference as tfr  # noqa: E402
import timevar_reference as tr  # noqa: E402
from psoap_amd import synthetic as syn  # noqa: E402

_LD = np.longdouble
_INF = float("inf")
MU_GP = mr.MU_GP
MARGIN = 8                                   # the project's margin over the float64 table (tests/test_gpu_grad.py)

DEFECTS = ("plain_Q",              # grad_tau contracted with Q = alpha alpha^T - K^-1 of the plain K
           "VtV_dropped_tau",      # Vt^T Vt left out of the Kt^-1 of the tau term
           "tau_squared",          # 1 / tau^2 for 1 / tau^3
           "index_time")           # dt from the pixel index instead of the times

# tau per case as multiples of the span of the dates: a finite value (0.25 or 2, timevar_reference._TAU) mixed with inf
# where c > 1; the c = 3 case has both finite fractions
TAU = {"a": (0.25, _INF), "b": (2.0,), "c": (_INF, 2.0), "d": (0.25,), "e": (0.25, _INF, 2.0), "f": (2.0, _INF)}
assert all(m in (0.25, 2.0, _INF) for v in TAU.values() for m in v) and {0.25, 2.0} <= set(sum(tr._TAU.values(), ()))


@dataclass
class MargTv:
    lnp: object
    parts: np.ndarray          # z^T z, log det K, gain, log det M
    beta: np.ndarray           # (n_epochs, order + 1)
    beta_cov: np.ndarray       # (q, q)
    fl_cor: np.ndarray         # (N,)
    gp: np.ndarray             # (2c,) gradients ...
    tau: np.ndarray            # (c,)
    lwl: np.ndarray            # (c, N)
    mu: object
    s_gp: np.ndarray           # ... and their cancellation scales
    s_tau: np.ndarray
    s_lwl: np.ndarray
    s_mu: object
    F: np.ndarray              # (3c, 3c): unit tangents of gp, then of tau
    F_mu: object


def unit_tangents(c, N):
    """(tan_lwl (3c, c, N) zeros, tan_gp (3c, 2c), tan_tau (3c, c)): the unit tangents of (gp, tau)"""
    eye = np.eye(3 * c)
    return np.zeros((3 * c, c, N)), np.ascontiguousarray(eye[:, :2 * c]), np.ascontiguousarray(eye[:, 2 * c:])


# ---- long double, on the dense Kt --------------------------------------------------------------------------------------------
def dense_ext(lwls, times, sigma, gp, tau, x, epoch_index, n_epochs, order, sd, weight=None):
    """-> (C, L, Li, H, lam): Kt in long double, its lower Cholesky factor, L^-1, the basis and the prior variances"""
    import oracle
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    N = lwls.shape[1]
    K = tr.matrix_ext(lwls, times, gp, tau)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=_LD) ** 2
    H = mr.basis(x, epoch_index, n_epochs, order, weight, T=_LD)
    lam = np.tile(np.asarray(sd, dtype=_LD) ** 2, n_epochs)
    C = K + (H * lam[None, :]) @ H.T
    C = _LD(0.5) * (C + C.T)
    L = oracle._chol_ext(C)
    return K, C, L, oracle._fsolve_ext(L, np.eye(N, dtype=_LD)), H, lam


def fisher_ext(Li, lwls, times, gp, tau, tan_lwl, tan_gp, tan_tau):
    """(F (T, T), F_mu) in long double from L^-1 of Kt: P_t = L^-1 K_t L^-T, F_st = 1/2 sum P_s P_t"""
    N = Li.shape[0]
    P = [Li @ tfr.tangent_matrix_tv(lwls, times, gp, tau, dx, dgp, dtau, _LD) @ Li.T
         for dx, dgp, dtau in zip(tan_lwl, tan_gp, tan_tau)]
    T = len(P)
    F = np.zeros((T, T), dtype=_LD)
    for s in range(T):
        for t in range(s, T):
            F[s, t] = F[t, s] = _LD(0.5) * np.sum(P[s] * P[t])
    y = Li @ np.ones(N, dtype=_LD)
    return F, y @ y


def marg_tv_ext(lwls, times, fl, sigma, gp, tau, x, epoch_index, n_epochs, order, sd, weight=None, mu_GP=1.0,
                tangents=None) -> MargTv:
    """every step in long double, on the dense K_tv + H Lambda H^T and its explicit inverse.  ``tangents``: (tan_lwl, tan_gp,
    tan_tau) of F (default: ``unit_tangents``)"""
    import oracle
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    c, N = lwls.shape
    K, C, L, Li, H, lam = dense_ext(lwls, times, sigma, gp, tau, x, epoch_index, n_epochs, order, sd, weight)
    r = np.asarray(fl, dtype=_LD) - _LD(mu_GP)
    zc = Li @ r
    alpha = Li.T @ zc
    Cinv = Li.T @ Li
    logdet_C, quad_C = _LD(2) * np.sum(np.log(np.diag(L))), zc @ zc
    lnp = _LD(-0.5) * (quad_C + logdet_C)
    HL = H * lam[None, :]
    V = Li @ HL
    beta = V.T @ zc
    cov = np.diag(lam) - V.T @ V
    cov = _LD(0.5) * (cov + cov.T)
    Lk = oracle._chol_ext(K)
    z = oracle._fsolve_ext(Lk, r)
    quad, logdet_K = z @ z, _LD(2) * np.sum(np.log(np.diag(Lk)))
    parts = np.array([quad, logdet_K, quad - quad_C, logdet_C - logdet_K], dtype=_LD)
    g_gp, g_tau, g_x, g_mu, s_gp, s_tau, s_x, s_mu = tr._contract(np.outer(alpha, alpha) - Cinv, lwls, times, gp, tau, alpha, _LD)
    F, F_mu = fisher_ext(Li, lwls, times, gp, tau, *(unit_tangents(c, N) if tangents is None else tangents))
    return MargTv(lnp, parts, beta.reshape(n_epochs, order + 1), cov, np.asarray(fl, dtype=_LD) - H @ beta, g_gp, g_tau, g_x, g_mu,
                  s_gp, s_tau, s_x, s_mu, F, F_mu)


# ---- float64, the device's route ---------------------------------------------------------------------------------------------
def _tau_sum(Q, lwls, t, gp, tau, cube=True):
    """dlnL/dtau (c,) from Q in float64: 1/2 a^2 / tau^3 sum Q e dt^2, e with the argument in the device's order"""
    c = lwls.shape[0]
    DT = t[None, :] - t[:, None]
    out = np.zeros(c)
    with np.errstate(under="ignore"):
        for k in range(c):
            a, l, tk = gp[2 * k], gp[2 * k + 1], tau[k]
            D = lwls[k][None, :] - lwls[k][:, None]
            A = (-0.5 * (tr.C_KMS * tr.C_KMS) / (l * l)) * D * D
            A = A + (-0.5 / (tk * tk)) * DT * DT
            out[k] = 0.5 * (a * a) / (tk * tk * tk if cube else tk * tk) * np.sum(Q * np.exp(A) * (DT * DT))
    return out


def marg_tv_f64(lwls, times, fl, sigma, gp, tau, x, epoch_index, n_epochs, order, sd, weight=None, mu_GP=1.0, tangents=None,
                defect=None, K=None) -> MargTv:
    """the device's formulae in float64 (Wi, Wh, M, Vt, alpha_m) on ``timevar_reference.matrix_f64``.  ``defect``: one of
    DEFECTS, a wrong formula in dlnL/dtau a test must be able to tell from the right one.  ``K``: the filled matrix, noise on
    its diagonal, in the place of ``matrix_f64``'s (the static twins fill with the oracle's exp(), not numpy's)"""
    from scipy.linalg import cho_factor, cho_solve, solve_triangular
    assert defect is None or defect in DEFECTS
    lwls = np.ascontiguousarray(np.atleast_2d(lwls), dtype=np.float64)
    gp, tau = np.asarray(gp, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    t = np.asarray(times, dtype=np.float64)
    c, N = lwls.shape
    if K is None:
        K = tr.matrix_f64(lwls, t, gp, tau, sigma)
    U = np.triu(cho_factor(K, lower=False)[0])
    s = np.tile(np.asarray(sd, dtype=np.float64), n_epochs)
    Ht = mr.basis(x, epoch_index, n_epochs, order, weight) * s[None, :]
    r = np.asarray(fl, dtype=np.float64) - mu_GP
    Wi = solve_triangular(U, np.eye(N), trans="T", lower=False)
    Wh = solve_triangular(U, Ht, trans="T", lower=False)
    z = solve_triangular(U, r, trans="T", lower=False)
    M = np.eye(Ht.shape[1]) + Wh.T @ Wh
    fm = cho_factor(M, lower=False)
    UM = np.triu(fm[0])
    bt = Wh.T @ z
    yv = solve_triangular(UM, bt, trans="T", lower=False)
    g = solve_triangular(UM, yv, lower=False)
    Minv = cho_solve(fm, np.eye(M.shape[0]))
    quad, logdet_K, gain, logdet_M = z @ z, 2 * np.sum(np.log(np.diag(U))), yv @ yv, 2 * np.sum(np.log(np.diag(UM)))
    lnp = -0.5 * (((quad - gain) + logdet_K) + logdet_M)
    # Kt^-1 and alpha_m for the gradient as ``marg_grad_reference.marg_grad_f64`` forms them (V = Wi^T Wh U_M^-1), for F as
    # ``marg_fisher_reference.woodbury_f64`` does (Vt = U_M^-T Wh^T Wi): the same matrices, each static twin's own bits
    Y = solve_triangular(UM, Wh.T, trans="T", lower=False).T
    V = Wi.T @ Y
    Kinv = Wi.T @ Wi
    Ainv = Kinv - V @ V.T
    alpha = Wi.T @ (z - Y @ yv)
    Vt = solve_triangular(UM, Wh.T @ Wi, trans="T", lower=False)
    Ainv_F = Kinv - Vt.T @ Vt
    with np.errstate(under="ignore"):
        g_gp, g_tau, g_x, g_mu, s_gp, s_tau, s_x, s_mu = tr._contract(np.outer(alpha, alpha) - Ainv, lwls, t, gp, tau, alpha,
                                                                       np.float64)
        if defect == "plain_Q":
            a0 = Wi.T @ z
            g_tau = _tau_sum(np.outer(a0, a0) - Kinv, lwls, t, gp, tau)
        elif defect == "VtV_dropped_tau":
            g_tau = _tau_sum(np.outer(alpha, alpha) - Kinv, lwls, t, gp, tau)
        elif defect == "tau_squared":
            g_tau = _tau_sum(np.outer(alpha, alpha) - Ainv, lwls, t, gp, tau, cube=False)
        elif defect == "index_time":
            g_tau = _tau_sum(np.outer(alpha, alpha) - Ainv, lwls, np.arange(N, dtype=np.float64), gp, tau)
        if defect is not None:
            g_tau = np.where(np.isfinite(tau), g_tau, 0.0)
    # F: G_t = 1/2 (A Z + Z^T A) with Z = K_t A, F_st = 1/2 sum K_s G_t (marg_fisher_reference.fisher_f64 with the TV tangents)
    tans = unit_tangents(c, N) if tangents is None else tangents
    Kt = [tfr.tangent_matrix_tv(lwls, t, gp, tau, dx, dgp, dtau) for dx, dgp, dtau in zip(*tans)]
    G = []
    for k in Kt:
        Z = k @ Ainv_F
        G.append(0.5 * (Ainv_F @ Z + Z.T @ Ainv_F))
    F = np.array([[0.5 * np.sum(ks * gt) for gt in G] for ks in Kt])
    y1, v1 = Wi @ np.ones(N), Vt @ np.ones(N)
    return MargTv(float(lnp), np.array([quad, logdet_K, gain, logdet_M]), (s * g).reshape(n_epochs, order + 1),
                  s[:, None] * Minv * s[None, :], np.asarray(fl, dtype=np.float64) - Ht @ g, g_gp, g_tau, g_x, float(g_mu),
                  s_gp, s_tau, s_x, float(s_mu), F, float(y1 @ y1 - v1 @ v1))


# ---- the cases -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_dates(case):
    """the date of every run of the case: those of the generated chunk ``marg_reference.case_chunk`` cuts its pixels from"""
    _, N, c, _ne, runs, _order = case
    full = syn.make_chunk(c, len(runs), max(n for _, n in runs), seed=9500 + N + c, sigma0=mr.SIGMA)
    return np.asarray(full.dates, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def case_times(case):
    """-> (times (N,), span): t_i = the date of pixel i's epoch minus the earliest date"""
    dates = case_dates(case)
    t = np.concatenate([np.full(n, dates[k]) for k, (_, n) in enumerate(case[4])]) - dates.min()
    t = np.ascontiguousarray(t)
    t.setflags(write=False)
    return t, float(dates.max() - dates.min())


def case_tau(case):
    return np.array(TAU[case[0]], dtype=np.float64) * case_times(case)[1]


def case_args(case, kind, tau=None):
    """the arguments of ``marg_tv_ext`` / ``marg_tv_f64`` up to mu_GP"""
    ch = mr.case_chunk(case)
    return (ch.lwls, case_times(case)[0], ch.fl, ch.sigma, mr.case_gp(case), case_tau(case) if tau is None else tau, ch.x,
            ch.epoch_index, ch.n_epochs, ch.order, mr.prior_sd(ch.order), mr.case_weight(case, kind), MU_GP)


@functools.lru_cache(maxsize=None)
def case_tangents(case):
    """(tan_lwl (T, c, N), tan_gp (T, 2c), tan_tau (T, c)), T = 3c + 1: the unit tangents of (gp, tau), then the seeded random
    grid tangent of ``marg_fisher_reference.case_tangents``"""
    import marg_fisher_reference as mfr
    _, N, c = case[:3]
    lw, g, ta = unit_tangents(c, N)
    tan_lwl = np.concatenate([lw, mfr.case_tangents(case)[0][2 * c + 2][None]])
    tan_gp, tan_tau = np.concatenate([g, np.zeros((1, 2 * c))]), np.concatenate([ta, np.zeros((1, c))])
    for a in (tan_lwl, tan_gp, tan_tau):
        a.setflags(write=False)
    return tan_lwl, tan_gp, tan_tau


@functools.lru_cache(maxsize=None)
def case_ext(case, kind) -> MargTv:
    """the long-double reference of a case; F (3c + 1, 3c + 1) along ``case_tangents``"""
    return marg_tv_ext(*case_args(case, kind), tangents=case_tangents(case))


def case_f64(case, kind, defect=None, tau=None, K=None) -> MargTv:
    return marg_tv_f64(*case_args(case, kind, tau), tangents=case_tangents(case), defect=defect, K=K)


OUTPUTS = ("lnp", "quad", "logdet_K", "gain", "logdet_M", "beta", "beta_cov", "fl_cor", "grad_gp", "grad_tau", "grad_mu",
           "grad_lwl", "F", "F_mu")


def errors(got, ref: MargTv, sd, want_fisher=True) -> dict:
    """per output: the value side in the measures of ``marg_reference.errors``, the gradients relative to the cancellation
    scale S (grad_tau: ``timevar_reference.rel_tau``), F relative to sqrt(F_ss F_tt) with exact zeros asked where the
    reference has them (``timevar_fisher_reference.rel_to_scale``), F_mu relative to itself"""
    out = mr.errors(got, ref, sd)
    out.update({"grad_gp": gr.rel_to_scale(got.gp, ref.gp, ref.s_gp), "grad_tau": tr.rel_tau(got.tau, ref.tau, ref.s_tau),
                "grad_mu": gr.rel_to_scale(got.mu, ref.mu, ref.s_mu), "grad_lwl": gr.rel_to_scale(got.lwl, ref.lwl, ref.s_lwl)})
    if want_fisher:
        out["F"] = tfr.rel_to_scale(got.F, ref.F)
        out["F_mu"] = float(abs(_LD(got.F_mu) - ref.F_mu) / ref.F_mu)
    return out


def measure_f64(defect=None, fisher=True):
    """per case and weight the errors of the twin against long double; ``fisher`` False leaves F out (the defects sit in
    dlnL/dtau alone)"""
    rows = []
    for case in mr.CASES:
        for kind in mr.WEIGHTS:
            got = case_f64(case, kind, defect) if fisher else marg_tv_f64(*case_args(case, kind), tangents=([], [], []), defect=defect)
            rows.append((f"{mr.case_id(case)}-{kind}", errors(got, case_ext(case, kind), mr.prior_sd(case[5]), want_fisher=fisher)))
    return rows


# The float64 table (python tests/marg_tv_reference.py), its last row: the largest error of the float64 evaluation against
# the long-double one, per output.  tests/test_marg_tv_reference.py checks that a fresh measurement does not exceed it; the
# device's tolerance is MARGIN times it (lnp: the relative 1e-10 of the sibling tests).
F64_MAX = {
    "quad": 1.20e-14, "logdet_K": 1.27e-15, "gain": 5.59e-12, "logdet_M": 5.18e-13, "beta": 1.07e-12, "beta_cov": 3.71e-12,
    "fl_cor": 1.62e-12, "grad_gp": 8.23e-16, "grad_tau": 4.71e-15, "grad_mu": 6.18e-15, "grad_lwl": 3.17e-12, "F": 5.94e-13,
    "F_mu": 3.60e-14,
}
LNP_RTOL = 1e-10
LNP_F64_MAX = 8.16e-14      # the same row's lnp: how far the float64 value itself is from long double, relative to max(1, |lnp|)
TOL = {k: MARGIN * v for k, v in F64_MAX.items()}


# ---- the planted chunk of marg_reference.planted with its dates -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_times():
    """-> (times (N,) Julian dates of every pixel's epoch, span): the dates of the chunk ``marg_reference.planted`` generates"""
    ch = syn.make_chunk(2, mr.PLANT_EPOCHS, mr.PLANT_PIX, seed=mr.PLANT_SEED, sigma0=mr.SIGMA)
    t = np.ascontiguousarray(ch.dates[np.asarray(ch.epoch_index)])
    return t, float(ch.dates.max() - ch.dates.min())


if __name__ == "__main__":
    rows = measure_f64()
    print(f"{'case':20s} " + " ".join(f"{k:>9s}" for k in OUTPUTS))
    for name, err in rows:
        print(f"{name:20s} " + " ".join(f"{err[k]:9.2e}" for k in OUTPUTS))
    print(f"{'max':20s} " + " ".join(f"{max(r[1][k] for r in rows):9.2e}" for k in OUTPUTS))
    print()
    print("seeded defects: the smallest, over the cases and weights, of grad_tau's error / scale")
    for d in DEFECTS:
        print(f"{d:16s} {min(e['grad_tau'] for _, e in measure_f64(d, fisher=False)):10.2e}")
