"""CPU references for the likelihood under the quasi-periodic kernel (tests/test_quasiperiodic_reference.py,
tests/test_gpu_quasiperiodic.py), modelled on tests/timevar_reference.py.

    lnL = -1/2 (r^T K^-1 r + log det K),  r = fl - mu_GP,
    K_ij = sum_c a_c^2 exp(p_c d_cij^2 + q_c dt_ij^2 - Gamma_c sin^2(pi dt_ij / P_c)) + sigma_i^2 delta_ij
    d_cij = x_c[j] - x_c[i],  p_c = -1/2 c_kms^2 / l_c^2;     dt_ij = t[j] - t[i],  q_c = -1/2 / tau_c^2

With alpha = K^-1 r, Q = alpha alpha^T - K^-1 and k_cij = a_c^2 exp(...) the formulas of timevar_reference hold with this k, and

    dlnL/dGamma_c = -1/2 sum_ij Q_ij k_cij sin^2(pi dt_ij / P_c)
    dlnL/dP_c     =  1/2 Gamma_c pi / P_c^2 sum_ij Q_ij k_cij dt_ij sin(2 pi dt_ij / P_c)

Two evaluations from the explicit inverse: ``qp_ext`` in np.longdouble on the long-double helpers of the oracle, ``qp_f64`` in
float64 with SciPy's ``cho_factor`` / ``cho_solve`` on a matrix whose exp() arguments are formed in the device's operation order
(``p * d * d``, ``+ q * dt * dt``, ``u = dt * (1 / P)``, ``s, co = sincospi(u)``, ``+ (-Gamma) * s * s``, every operation rounded
on its own).  NumPy has no sincospi: the twin reduces ``u`` by its nearest integer -- exact in floating point -- and takes
``sin`` and ``cos`` of ``pi r``, ``|r| <= 1/2``, which is good to about two ulp.  Both return, per output, the cancellation scale
S = 1/2 sum_ij |Q_ij| |dK_ij/dtheta| of its sum (sum_i |alpha_i| for mu_GP).

``qp_f64(..., defect=name)`` seeds one of DEFECTS into the twin: what tests/test_quasiperiodic_reference.py holds the derived
bounds against.

``python tests/quasiperiodic_reference.py`` prints |f64 - long double| / S per case and output, the fill's error, and the factor
by which every seeded defect leaves the bound: what the tolerances of tests/test_gpu_quasiperiodic.py are derived from.
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
import timevar_reference as tv  # noqa: E402

_LD = np.longdouble
MU_GP = gr.MU_GP
C_KMS = 2.99792458e5
MARGIN = 8
LNP_RTOL = 1e-10
_PI_LD = _LD("3.14159265358979323846264338327950288")

# name -> what is wrong.  "matrix" defects change K as well (a device with that defect would fill and contract with it);
# the others sit in one finishing formula.
DEFECTS = {
    "sin-for-sin2": "sin in place of sin^2 in d lnL / d Gamma",
    "two-pi-phase": "2 pi in place of pi in the phase, in the fill and the contraction",
    "wrong-period": "the next component's P in the place of a component's own, in the fill and the contraction",
    "gamma-missing": "Gamma missing from d lnL / d P",
    "dt-missing": "dt missing from d lnL / d P",
    "gamma-sign": "the sign of d lnL / d Gamma",
}


@dataclass(frozen=True)
class QpGrad:
    lnp: float
    gp: np.ndarray        # (2c,)
    tau: np.ndarray       # (c,)
    gamma: np.ndarray     # (c,)
    period: np.ndarray    # (c,)
    lwl: np.ndarray       # (c, N)
    mu: float
    s_gp: np.ndarray      # the scales of the same shapes
    s_tau: np.ndarray
    s_gamma: np.ndarray
    s_period: np.ndarray
    s_lwl: np.ndarray
    s_mu: float


def sincospi_f64(u):
    """(sin(pi u), cos(pi u)) in float64 from the exact reduction r = u - rint(u), |r| <= 1/2; sin(pi u) is +0 at u = 0"""
    u = np.asarray(u, dtype=np.float64)
    n = np.rint(u)
    r = u - n
    sign = np.where(np.fmod(n, 2.0) == 0.0, 1.0, -1.0)
    s = np.where(r == 0.0, 0.0, sign * np.sin(np.pi * r))
    return s, sign * np.cos(np.pi * r)


def _phase(DT, period, T, defect, k, periods):
    """(sin, cos) of pi dt / P_k in the number type T, as the evaluation of that type forms it, with the phase defects"""
    if defect == "wrong-period":
        period = periods[(k + 1) % len(periods)]
    mult = 2.0 if defect == "two-pi-phase" else 1.0
    if T is _LD:
        ph = _PI_LD * _LD(mult) * DT / _LD(period)
        return np.sin(ph), np.cos(ph)
    return sincospi_f64(mult * (DT * (1.0 / float(period))))


def _contract(Q, lwls, times, gp, tau, gamma, period, alpha, T, defect=None):
    """the seven formulas, and their scales, from Q in the number type ``T`` (tv._contract with the periodic factor)"""
    c, N = lwls.shape
    ckms = T("2.99792458e5") if T is _LD else T(2.99792458e5)
    pi = _PI_LD if T is _LD else T(np.pi)
    aQ = np.abs(Q)
    t = np.asarray(times, dtype=T)
    DT = t[None, :] - t[:, None]
    z2, zc = (lambda: np.zeros(2 * c, dtype=T)), (lambda: np.zeros(c, dtype=T))
    g_gp, s_gp, g_tau, s_tau, g_gam, s_gam, g_per, s_per = z2(), z2(), zc(), zc(), zc(), zc(), zc(), zc()
    g_x, s_x = np.zeros((c, N), dtype=T), np.zeros((c, N), dtype=T)
    for k in range(c):
        a, l, tk, gk, pk = T(gp[2 * k]), T(gp[2 * k + 1]), T(tau[k]), T(gamma[k]), T(period[k])
        x = np.asarray(lwls[k], dtype=T)
        D = x[None, :] - x[:, None]
        p = T(-0.5) * ckms * ckms / (l * l)
        q = T(-0.5) / (tk * tk)
        S, Co = _phase(DT, period[k], T, defect, k, period)
        Kc = a * a * np.exp(p * D * D + q * DT * DT - gk * S * S)
        g_gp[2 * k] = T(0.5) * np.sum(Q * (T(2) * Kc / a))
        s_gp[2 * k] = T(0.5) * np.sum(aQ * np.abs(T(2) * Kc / a))
        dl = Kc * (ckms * ckms) * (D * D) / (l * l * l)
        g_gp[2 * k + 1] = T(0.5) * np.sum(Q * dl)
        s_gp[2 * k + 1] = T(0.5) * np.sum(aQ * np.abs(dl))
        dtau = Kc * (DT * DT) / (tk * tk * tk)
        g_tau[k] = T(0.5) * np.sum(Q * dtau)
        s_tau[k] = T(0.5) * np.sum(aQ * np.abs(dtau))
        dgam = -Kc * (S if defect == "sin-for-sin2" else S * S)
        if defect == "gamma-sign":
            dgam = -dgam
        g_gam[k] = T(0.5) * np.sum(Q * dgam)
        s_gam[k] = T(0.5) * np.sum(aQ * np.abs(dgam))
        dper = Kc * (T(1) if defect == "gamma-missing" else gk) * pi / (pk * pk) * (T(1) if defect == "dt-missing" else DT) * \
            (T(2) * S * Co)
        g_per[k] = T(0.5) * np.sum(Q * dper)
        s_per[k] = T(0.5) * np.sum(aQ * np.abs(dper))
        dx = Kc * (T(-2) * p * D)
        g_x[k] = np.sum(Q * dx, axis=1)
        s_x[k] = np.sum(aQ * np.abs(dx), axis=1)
    return (g_gp, g_tau, g_gam, g_per, g_x, np.sum(alpha)), (s_gp, s_tau, s_gam, s_per, s_x, np.sum(np.abs(alpha)))


def matrix_ext(lwls, times, gp, tau, gamma, period):
    """K without the noise term in long double (tv.matrix_ext with the periodic factor; the diagonal is sum amp^2)"""
    import oracle
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    t = np.asarray(times, dtype=_LD)
    DT = t[None, :] - t[:, None]
    K = 0
    for k in range(lwls.shape[0]):
        x = np.asarray(lwls[k], dtype=_LD)
        r = x[None, :] - x[:, None]
        amp, l, tk = gp[2 * k], gp[2 * k + 1], _LD(tau[k])
        S = np.sin(_PI_LD * DT / _LD(period[k]))
        K = K + _LD(amp) ** 2 * np.exp(_LD(-0.5) * oracle._C_KMS * oracle._C_KMS / (_LD(l) * _LD(l)) * r * r +
                                       _LD(-0.5) / (tk * tk) * DT * DT - _LD(gamma[k]) * S * S)
    K[np.diag_indices_from(K)] = sum(_LD(gp[2 * k]) ** 2 for k in range(lwls.shape[0]))
    return K


def qp_ext(lwls, times, fl, sigma, gp, tau, gamma, period, mu_GP=1.0) -> QpGrad:
    """every step in long double: K, its Cholesky factor, the explicit inverse, the contraction"""
    import oracle
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    N = lwls.shape[1]
    K = matrix_ext(lwls, times, gp, tau, gamma, period)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=_LD) ** 2
    L = oracle._chol_ext(K)
    Li = oracle._fsolve_ext(L, np.eye(N, dtype=_LD))          # L^-1
    r = np.asarray(fl, dtype=_LD) - _LD(mu_GP)
    z = Li @ r
    alpha = Li.T @ z
    Kinv = Li.T @ Li
    lnp = _LD(-0.5) * (z @ z + _LD(2) * np.sum(np.log(np.diag(L))))
    g, s = _contract(np.outer(alpha, alpha) - Kinv, lwls, times, gp, tau, gamma, period, alpha, _LD)
    return QpGrad(float(lnp), *g, *s)


def matrix_f64(lwls, times, gp, tau, gamma, period, sigma=None, want_args=False, defect=None):
    """K in float64 as the device's fill forms it (k_fill_sym_qp): per component the argument ``p * d * d``, ``+ q * dt * dt``,
    ``+ (-Gamma) * s * s`` with ``s = sinpi(dt * (1 / P))`` and every operation rounded on its own, ``a^2 exp()``, the components
    added in order; the diagonal is ``sum a^2 (+ sigma^2)``.  ``want_args``: also the (c, N, N) arguments."""
    lwls = np.ascontiguousarray(np.atleast_2d(lwls), dtype=np.float64)
    gp, tau = np.asarray(gp, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    gamma, period = np.asarray(gamma, dtype=np.float64), np.asarray(period, dtype=np.float64)
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
            S, _ = _phase(DT, period[k], np.float64, defect, k, period)
            A = A + (-gamma[k]) * S * S
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


def qp_f64(lwls, times, fl, sigma, gp, tau, gamma, period, mu_GP=1.0, defect=None) -> QpGrad:
    """the same in float64: ``matrix_f64``, SciPy's cho_factor, K^-1 and alpha from cho_solve; ``defect``: one of DEFECTS"""
    from scipy.linalg import cho_factor, cho_solve
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")
    lwls = np.ascontiguousarray(np.atleast_2d(lwls), dtype=np.float64)
    gp, tau = np.asarray(gp, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    gamma, period = np.asarray(gamma, dtype=np.float64), np.asarray(period, dtype=np.float64)
    N = lwls.shape[1]
    K = matrix_f64(lwls, times, gp, tau, gamma, period, sigma, defect=defect)
    factor = cho_factor(K, lower=False)
    r = np.asarray(fl, dtype=np.float64) - mu_GP
    alpha = cho_solve(factor, r)
    Kinv = cho_solve(factor, np.eye(N))
    lnp = -0.5 * (r @ alpha + np.sum(2 * np.log(np.diag(factor[0]))))
    with np.errstate(under="ignore"):
        g, s = _contract(np.outer(alpha, alpha) - Kinv, lwls, times, gp, tau, gamma, period, alpha, np.float64, defect)
    return QpGrad(float(lnp), *g[:5], float(g[5]), *s[:5], float(s[5]))


# ---- the cases of tests/test_gpu_quasiperiodic.py -----------------------------------------------------------------------
# The data of timevar_reference.CASES; per case (tau, Gamma, P) per component, tau and P as multiples of the span of the dates.
# Among them: P shorter than the span by a factor of more than 20 (N100-c2, N300-c1, N300-c3 and the permuted case: the phase
# reduction), P longer than the span (N128-c2, N300-c3, N520-c2), a component with Gamma = 0 (N100-c2, N129-c2, N300-c2,
# N300-c3) and a purely periodic one, tau = inf with Gamma > 0 (N128-c2, N300-c3, N520-c2, the permuted case).
_INF = float("inf")
_QP = {
    "N100-c2": ((0.25, _INF), (1.5, 0.0), (0.03, 0.7)),
    "N128-c2": ((_INF, 2.0), (2.0, 0.5), (0.4, 3.0)),
    "N129-c2": ((2.0, _INF), (0.8, 0.0), (0.21, 1.0)),
    "N300-c1": ((0.25,), (1.0,), (0.045,)),
    "N300-c2": ((_INF, 0.25), (0.0, 3.0), (1.0, 0.3)),
    "N300-c3": ((0.25, _INF, 2.0), (1.0, 2.5, 0.0), (0.04, 0.35, 1.5)),
    "N520-c2": ((0.25, _INF), (0.7, 1.2), (1.7, 0.11)),
    "N300-c2-perm": ((2.0, _INF), (1.5, 0.6), (0.37, 0.045)),
}
CASES = tuple((name, shape, _QP[name], permuted) for name, shape, _mult, permuted in tv.CASES)
assert len(CASES) == len(_QP)


def case_id(case):
    return case[0]


@dataclass(frozen=True)
class QpCase:
    lwls: np.ndarray      # (c, N)
    times: np.ndarray     # (N,) dates[epoch] - min(dates), days
    fl: np.ndarray
    sigma: np.ndarray
    gp: np.ndarray
    tau: np.ndarray
    gamma: np.ndarray
    period: np.ndarray
    span: float


@functools.lru_cache(maxsize=None)
def case_data(case) -> QpCase:
    name, shape, (tau, gamma, period), permuted = case
    d = tv.case_data((name, shape, tau, permuted))
    f = lambda v: np.array(v, dtype=np.float64)  # noqa: E731
    return QpCase(d.lwls, d.times, d.fl, d.sigma, d.gp, d.tau, f(gamma), f(period) * d.span, d.span)


@functools.lru_cache(maxsize=None)
def case_ext(case) -> QpGrad:
    d = case_data(case)
    return qp_ext(d.lwls, d.times, d.fl, d.sigma, d.gp, d.tau, d.gamma, d.period, MU_GP)


OUTPUTS = ("gp", "tau", "gamma", "period", "mu", "lwl")


def errors(got, ref: QpGrad) -> dict:
    """per output the error relative to its cancellation scale; grad_tau, grad_gamma and grad_period over the components whose
    scale is not 0 (``tv.rel_tau``: where it is -- tau = inf, Gamma = 0 for the period -- the tests ask for an exact 0)"""
    return {"gp": gr.rel_to_scale(got.gp, ref.gp, ref.s_gp), "tau": tv.rel_tau(got.tau, ref.tau, ref.s_tau),
            "gamma": tv.rel_tau(got.gamma, ref.gamma, ref.s_gamma), "period": tv.rel_tau(got.period, ref.period, ref.s_period),
            "mu": gr.rel_to_scale(got.mu, ref.mu, ref.s_mu), "lwl": gr.rel_to_scale(got.lwl, ref.lwl, ref.s_lwl)}


def lnp_error(got_lnp, ref: QpGrad) -> float:
    return abs(got_lnp - ref.lnp) / max(1.0, abs(ref.lnp))


def fill_error(got, ext) -> float:
    """max |got - ext| / ext over the elements where ext is a normal float64 with room below it (>= 1e-300); below that the
    result is subnormal or zero, and ``got`` must be too"""
    ext = np.asarray(ext, dtype=_LD)
    big = ext >= _LD(1e-300)
    if np.any(np.asarray(got)[~big] > 1e-299):
        return float("inf")
    return float(np.max(np.abs(np.asarray(got, dtype=_LD)[big] - ext[big]) / ext[big]))


@functools.lru_cache(maxsize=None)
def measure_f64(defect=None):
    """the float64 twin (with ``defect`` seeded into it) against the long-double evaluation on CASES: per case the error relative
    to S of each output, the relative error of lnp and -- without a defect -- the fill's"""
    rows = []
    for case in CASES:
        d, ref = case_data(case), case_ext(case)
        got = qp_f64(d.lwls, d.times, d.fl, d.sigma, d.gp, d.tau, d.gamma, d.period, MU_GP, defect)
        e = errors(got, ref)
        e["lnp"] = lnp_error(got.lnp, ref)
        if defect is None:
            e["fill"] = fill_error(matrix_f64(d.lwls, d.times, d.gp, d.tau, d.gamma, d.period, d.sigma),
                                   matrix_ext(d.lwls, d.times, d.gp, d.tau, d.gamma, d.period) +
                                   np.diag(np.asarray(d.sigma, dtype=_LD) ** 2))
        rows.append((case_id(case), e))
    return tuple(rows)


def bounds() -> dict:
    """the derived bounds: per gradient output and for the fill MARGIN x the twin's largest error over the cases; lnp keeps the
    siblings' relative 1e-10"""
    rows = measure_f64()
    out = {k: MARGIN * max(e[k] for _, e in rows) for k in OUTPUTS + ("fill",)}
    out["lnp"] = LNP_RTOL
    return out


def defect_factor(defect) -> tuple:
    """-> (the output that leaves its bound furthest, by which factor) with ``defect`` seeded into the twin"""
    b = bounds()
    worst = {k: max(e[k] for _, e in measure_f64(defect)) / b[k] for k in OUTPUTS + ("lnp",)}
    k = max(worst, key=worst.get)
    return k, worst[k]


# ---- the fit of tests/test_gpu_quasiperiodic.py (and its CPU half in tests/test_quasiperiodic_reference.py) ------------------
@dataclass(frozen=True)
class FitCase:
    lwls: np.ndarray
    times: np.ndarray     # Julian dates per pixel (covariance subtracts the minimum); t0 = times - min
    t0: np.ndarray
    fl: np.ndarray
    sigma: np.ndarray
    span: float
    truth: tuple          # (gp, tau, gamma, period) the flux was drawn from
    start: tuple          # (gp0, tau0, gamma0, period0) of both fits
    P0: float


@functools.lru_cache(maxsize=None)
def fit_case(planted: bool) -> FitCase:
    """An SB2 chunk of N = 300 pixels over 12 epochs (span 364 days), flux drawn by ``synthetic.draw_quasiperiodic_flux``.
    ``planted``: component 0 repeats with P_0 = span / 4.3 (4.3 cycles, Gamma = 2) and decays over tau = 2 x span; otherwise
    the same draw with Gamma = 0, the time-variable model.  Component 1 is static in both.  Both fits start 10 % off in P."""
    from psoap_amd import synthetic as syn
    ch = syn.make_chunk(2, 12, 25, seed=9100)
    times = ch.dates[ch.epoch_index]
    t0 = times - times.min()
    span = float(t0.max())
    P0 = span / 4.3
    gp = np.array(syn.GP_BASE[2], dtype=np.float64)
    tau, gamma, period = np.array([2.0 * span, _INF]), np.array([2.0 if planted else 0.0, 0.0]), np.array([P0, 1.0])
    fl = syn.draw_quasiperiodic_flux(ch.lwls, t0, ch.sigma, gp, tau, gamma, period, 1.0, 9200)
    start = (gp * np.array([1.2, 0.9, 0.85, 1.15]), np.array([1.2 * span, _INF]), np.array([1.0, 0.0]), np.array([1.1 * P0, 1.0]))
    return FitCase(ch.lwls, times, t0, fl, ch.sigma.copy(), span, (gp, tau, gamma, period), start, P0)


def fit_twin(fc: FitCase):
    """``value_grad`` of the drivers of psoap_amd.covariance on the float64 twin"""
    def value_grad(gp, tau, gamma, period):
        g = qp_f64(fc.lwls, fc.t0, fc.fl, fc.sigma, gp, tau, gamma, period, 1.0)
        return g.lnp, g.gp, g.tau, g.gamma, g.period
    return value_grad


@functools.lru_cache(maxsize=None)
def fit_on_twin(planted: bool):
    """-> (gp, tau, gamma, period, lnp, lnp_gamma0, lnp_timevar, SciPy's result) of the drivers on the twin: what
    ``optimize_GP_quasiperiodic(..., full_output=True)`` returns from the device"""
    from psoap_amd import covariance
    fc = fit_case(planted)
    vg = fit_twin(fc)
    gp, tau, gamma, period, res = covariance._fit_quasiperiodic(vg, 2, *fc.start, None, covariance.default_period_bounds(fc.t0), 1e-10)
    lnp_gamma0, lnp_tv = covariance._quasiperiodic_null(vg, 2, gp, tau, None, 1e-10)
    return gp, tau, gamma, period, -float(res["fun"]), lnp_gamma0, lnp_tv, res


if __name__ == "__main__":
    rows = measure_f64()
    cols = OUTPUTS + ("lnp", "fill")
    print(f"{'case':13s} " + " ".join(f"{k if k in ('lnp', 'fill') else 'grad_' + k:>11s}" for k in cols))
    for name, e in rows:
        print(f"{name:13s} " + " ".join(f"{e[k]:11.2e}" for k in cols))
    print(f"{'max':13s} " + " ".join(f"{max(e[k] for _, e in rows):11.2e}" for k in cols))
    b = bounds()
    print(f"{'bound':13s} " + " ".join(f"{b[k]:11.2e}" for k in cols))
    print()
    for name in DEFECTS:
        k, f = defect_factor(name)
        print(f"defect {name:14s} leaves the bound of {k:7s} by a factor of {f:.3g}")
