"""CPU references for the likelihood under time-variable component spectra (tests/test_timevar_reference.py,
tests/test_gpu_timevar.py), modelled on tests/grad_reference.py.

    lnL = -1/2 (r^T K^-1 r + log det K),  r = fl - mu_GP,
    K_ij = sum_c a_c^2 exp(p_c d_cij^2 + q_c dt_ij^2) + sigma_i^2 delta_ij
    d_cij = x_c[j] - x_c[i],  p_c = -1/2 c_kms^2 / l_c^2;     dt_ij = t[j] - t[i],  q_c = -1/2 / tau_c^2

With alpha = K^-1 r, Q = alpha alpha^T - K^-1 and k_cij = a_c^2 exp(p_c d_cij^2 + q_c dt_ij^2):

    dlnL/da_c    = 1/2 sum_ij Q_ij 2 k_cij / a_c
    dlnL/dl_c    = 1/2 sum_ij Q_ij k_cij c_kms^2 d_cij^2 / l_c^3
    dlnL/dtau_c  = 1/2 sum_ij Q_ij k_cij dt_ij^2 / tau_c^3
    dlnL/dx_c[i] = sum_j Q_ij k_cij (-2 p_c d_cij)
    dlnL/dmu_GP  = sum_i alpha_i

Two evaluations from the explicit inverse: ``tv_ext`` in np.longdouble on the long-double helpers of the oracle, ``tv_f64`` in
float64 with SciPy's ``cho_factor`` / ``cho_solve`` on a matrix whose exp() arguments are formed in the device's operation
order (``p * d * d``, then ``+ q * dt * dt``, every operation rounded on its own).  Both return, per output, the cancellation
scale S = 1/2 sum_ij |Q_ij| |dK_ij/dtheta| of its sum (sum_i |alpha_i| for mu_GP).

``python tests/timevar_reference.py`` prints |f64 - long double| / S per case and output: what the tolerances of
tests/test_gpu_timevar.py are derived from.
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

_LD = np.longdouble
MU_GP = gr.MU_GP
C_KMS = 2.99792458e5


@dataclass(frozen=True)
class TvGrad:
    lnp: float
    gp: np.ndarray        # (2c,)
    tau: np.ndarray       # (c,)
    lwl: np.ndarray       # (c, N)
    mu: float
    s_gp: np.ndarray      # the scales of the same shapes
    s_tau: np.ndarray
    s_lwl: np.ndarray
    s_mu: float


def _contract(Q, lwls, times, gp, tau, alpha, T):
    """the five formulas, and their scales, from Q in the number type ``T`` (gr._contract with the temporal factor)"""
    c, N = lwls.shape
    ckms = T("2.99792458e5") if T is _LD else T(2.99792458e5)
    aQ = np.abs(Q)
    t = np.asarray(times, dtype=T)
    DT = t[None, :] - t[:, None]
    g_gp, s_gp = np.zeros(2 * c, dtype=T), np.zeros(2 * c, dtype=T)
    g_tau, s_tau = np.zeros(c, dtype=T), np.zeros(c, dtype=T)
    g_x, s_x = np.zeros((c, N), dtype=T), np.zeros((c, N), dtype=T)
    for k in range(c):
        a, l, tk = T(gp[2 * k]), T(gp[2 * k + 1]), T(tau[k])
        x = np.asarray(lwls[k], dtype=T)
        D = x[None, :] - x[:, None]
        p = T(-0.5) * ckms * ckms / (l * l)
        q = T(-0.5) / (tk * tk)
        Kc = a * a * np.exp(p * D * D + q * DT * DT)
        g_gp[2 * k] = T(0.5) * np.sum(Q * (T(2) * Kc / a))
        s_gp[2 * k] = T(0.5) * np.sum(aQ * np.abs(T(2) * Kc / a))
        dl = Kc * (ckms * ckms) * (D * D) / (l * l * l)
        g_gp[2 * k + 1] = T(0.5) * np.sum(Q * dl)
        s_gp[2 * k + 1] = T(0.5) * np.sum(aQ * np.abs(dl))
        dtau = Kc * (DT * DT) / (tk * tk * tk)
        g_tau[k] = T(0.5) * np.sum(Q * dtau)
        s_tau[k] = T(0.5) * np.sum(aQ * np.abs(dtau))
        dx = Kc * (T(-2) * p * D)
        g_x[k] = np.sum(Q * dx, axis=1)
        s_x[k] = np.sum(aQ * np.abs(dx), axis=1)
    return g_gp, g_tau, g_x, np.sum(alpha), s_gp, s_tau, s_x, np.sum(np.abs(alpha))


def matrix_ext(lwls, times, gp, tau):
    """K without the noise term in long double, built as the oracle's ``_sym_ext`` builds the static one (the diagonal is
    sum amp^2)"""
    import oracle
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    t = np.asarray(times, dtype=_LD)
    DT = t[None, :] - t[:, None]
    K = 0
    for k in range(lwls.shape[0]):
        x = np.asarray(lwls[k], dtype=_LD)
        r = x[None, :] - x[:, None]
        amp, l, tk = gp[2 * k], gp[2 * k + 1], _LD(tau[k])
        K = K + _LD(amp) ** 2 * np.exp(_LD(-0.5) * oracle._C_KMS * oracle._C_KMS / (_LD(l) * _LD(l)) * r * r +
                                       _LD(-0.5) / (tk * tk) * DT * DT)
    K[np.diag_indices_from(K)] = sum(_LD(gp[2 * k]) ** 2 for k in range(lwls.shape[0]))
    return K


def tv_ext(lwls, times, fl, sigma, gp, tau, mu_GP=1.0) -> TvGrad:
    """every step in long double: K, its Cholesky factor, the explicit inverse, the contraction"""
    import oracle
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    N = lwls.shape[1]
    K = matrix_ext(lwls, times, gp, tau)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=_LD) ** 2
    L = oracle._chol_ext(K)
    Li = oracle._fsolve_ext(L, np.eye(N, dtype=_LD))          # L^-1
    r = np.asarray(fl, dtype=_LD) - _LD(mu_GP)
    z = Li @ r
    alpha = Li.T @ z
    Kinv = Li.T @ Li
    lnp = _LD(-0.5) * (z @ z + _LD(2) * np.sum(np.log(np.diag(L))))
    g_gp, g_tau, g_x, g_mu, s_gp, s_tau, s_x, s_mu = _contract(np.outer(alpha, alpha) - Kinv, lwls, times, gp, tau, alpha, _LD)
    return TvGrad(float(lnp), g_gp, g_tau, g_x, g_mu, s_gp, s_tau, s_x, s_mu)


def matrix_f64(lwls, times, gp, tau, sigma=None, want_args=False):
    """K in float64 as the device's fill forms it (k_fill_sym_tv): per component the argument ``p * d * d`` then
    ``+ q * dt * dt`` with every operation rounded on its own, ``a^2 exp()``, the components added in order; the diagonal is
    ``sum a^2 (+ sigma^2)``.  ``want_args``: also the (c, N, N) arguments, for the places where exp() must be exactly +0."""
    lwls = np.ascontiguousarray(np.atleast_2d(lwls), dtype=np.float64)
    gp, tau = np.asarray(gp, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    t = np.asarray(times, dtype=np.float64)
    c, N = lwls.shape
    DT = t[None, :] - t[:, None]
    K, args, dsum = None, [], None
    with np.errstate(under="ignore"):
        for k in range(c):
            amp, l = gp[2 * k], gp[2 * k + 1]
            a2 = amp * amp
            p2 = -0.5 * (C_KMS * C_KMS) / (l * l)
            q2 = -0.5 / (tau[k] * tau[k])
            D = lwls[k][None, :] - lwls[k][:, None]
            A = p2 * D * D
            A = A + q2 * DT * DT
            term = a2 * np.exp(A)
            K = term if k == 0 else K + term
            dsum = a2 if k == 0 else dsum + a2
            args.append(A)
    diag = np.full(N, dsum)
    if sigma is not None:
        s = np.asarray(sigma, dtype=np.float64)
        diag = diag + s * s
    K[np.diag_indices_from(K)] = diag
    return (K, np.stack(args)) if want_args else K


def tv_f64(lwls, times, fl, sigma, gp, tau, mu_GP=1.0) -> TvGrad:
    """the same in float64: ``matrix_f64``, SciPy's cho_factor, K^-1 and alpha from cho_solve"""
    from scipy.linalg import cho_factor, cho_solve
    lwls = np.ascontiguousarray(np.atleast_2d(lwls), dtype=np.float64)
    gp, tau = np.asarray(gp, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    N = lwls.shape[1]
    K = matrix_f64(lwls, times, gp, tau, sigma)
    factor = cho_factor(K, lower=False)
    r = np.asarray(fl, dtype=np.float64) - mu_GP
    alpha = cho_solve(factor, r)
    Kinv = cho_solve(factor, np.eye(N))
    lnp = -0.5 * (r @ alpha + np.sum(2 * np.log(np.diag(factor[0]))))
    with np.errstate(under="ignore"):
        g_gp, g_tau, g_x, g_mu, s_gp, s_tau, s_x, s_mu = _contract(np.outer(alpha, alpha) - Kinv, lwls, times, gp, tau, alpha,
                                                                   np.float64)
    return TvGrad(float(lnp), g_gp, g_tau, g_x, float(g_mu), s_gp, s_tau, s_x, float(s_mu))


# ---- the cases of tests/test_gpu_timevar.py ---------------------------------------------------------------------------
# (name, the shape of grad_reference.CASES, tau per component as multiples of the span of the dates, pixels permuted):
# every c = 2 case has one finite and one infinite tau, the c = 3 case 0.25 x span, inf and 2 x span; the last case is
# N = 300, c = 2 with the pixels in a random order, so the times are in no epoch order.
_INF = float("inf")
_TAU = {(100, 2): (0.25, _INF), (128, 2): (_INF, 2.0), (129, 2): (2.0, _INF), (300, 1): (0.25,), (300, 2): (_INF, 0.25),
        (300, 3): (0.25, _INF, 2.0), (520, 2): (0.25, _INF)}
CASES = tuple((gr.case_id(s), s, _TAU[s[:2]], False) for s in gr.CASES) + (("N300-c2-perm", gr.CASES[4], (2.0, _INF), True),)


def case_id(case):
    return case[0]


@dataclass(frozen=True)
class TvCase:
    lwls: np.ndarray      # (c, N)
    times: np.ndarray     # (N,) dates[epoch] - min(dates), days
    fl: np.ndarray
    sigma: np.ndarray
    gp: np.ndarray
    tau: np.ndarray
    span: float


@functools.lru_cache(maxsize=None)
def case_data(case) -> TvCase:
    _name, shape, mult, permuted = case
    ch = gr.case_chunk(shape)
    times = ch.dates[ch.epoch_index] - ch.dates.min()
    span = float(ch.dates.max() - ch.dates.min())
    lwls, fl, sigma = ch.lwls, ch.fl, ch.sigma
    if permuted:
        perm = np.random.default_rng(7200 + shape[0] + shape[1]).permutation(ch.N)
        lwls, times, fl, sigma = lwls[:, perm], times[perm], fl[perm], sigma[perm]
    c_ = np.ascontiguousarray
    return TvCase(c_(lwls), c_(times), c_(fl), c_(sigma), gr.case_gp(shape), np.array(mult, dtype=np.float64) * span, span)


@functools.lru_cache(maxsize=None)
def case_ext(case) -> TvGrad:
    d = case_data(case)
    return tv_ext(d.lwls, d.times, d.fl, d.sigma, d.gp, d.tau, MU_GP)


def rel_tau(got, ref, scale):
    """``gr.rel_to_scale`` over the components with a finite tau (at tau = inf the derivative and its scale are both 0: the
    tests ask for an exact 0 there)"""
    keep = np.asarray(scale, dtype=_LD) > 0
    if not np.any(keep):
        return 0.0
    return gr.rel_to_scale(np.asarray(got)[keep], np.asarray(ref)[keep], np.asarray(scale)[keep])


def errors(got: TvGrad, ref: TvGrad) -> dict:
    return {"gp": gr.rel_to_scale(got.gp, ref.gp, ref.s_gp), "tau": rel_tau(got.tau, ref.tau, ref.s_tau),
            "mu": gr.rel_to_scale(got.mu, ref.mu, ref.s_mu), "lwl": gr.rel_to_scale(got.lwl, ref.lwl, ref.s_lwl)}


OUTPUTS = ("gp", "tau", "mu", "lwl")


def measure_f64():
    """the float64 SciPy evaluation against the long-double one on CASES: per case the error relative to S of each output"""
    rows = []
    for case in CASES:
        d, ref = case_data(case), case_ext(case)
        e = errors(tv_f64(d.lwls, d.times, d.fl, d.sigma, d.gp, d.tau, MU_GP), ref)
        rows.append((case_id(case),) + tuple(e[k] for k in OUTPUTS))
    return rows


if __name__ == "__main__":
    rows = measure_f64()
    print(f"{'case':13s} " + " ".join(f"{'grad_' + k:>10s}" for k in OUTPUTS))
    for row in rows:
        print(f"{row[0]:13s} " + " ".join(f"{v:10.2e}" for v in row[1:]))
    print(f"{'max':13s} " + " ".join(f"{max(r[k] for r in rows):10.2e}" for k in range(1, 5)))
