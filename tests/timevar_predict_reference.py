"""CPU references for the component spectra at a date under the time-variable kernel (tests/test_timevar_predict_reference.py,
tests/test_gpu_timevar_predict.py): the conditional of the plain predict modes with the temporal factor of
tests/timevar_reference.py in the data covariance, the cross-covariance and the prior.

    k_c(x, t; x', t') = a_c^2 exp(p_c (x' - x)^2 + q_c (t' - t)^2),   p_c = -1/2 c_kms^2 / l_c^2,  q_c = -1/2 / tau_c^2
    K  (N x N): sum_c k_c over the pixels (x_c[i], t[i]), the diagonal sum_c a_c^2 + sigma_i^2
    Ct (N x R): k_c between pixel i and prediction point (xp_c[m], tp[m]) -- tp is shared by the components
    A  (R x R): k_c between prediction points, the diagonal by the fill_V11_f rule (a_c^2; + 1e-8 in mode 1)
    mu = m0 + Ct^T K^-1 (fl - offset),   Sigma = A - Ct^T K^-1 Ct        (modes, m0, offset, blocks: oracle.predict_ext)

``tv_predict_ext`` forms K, Ct and A dense in np.longdouble and uses the oracle's long-double Cholesky and solves.
``tv_predict_f64`` follows the device's route in float64 with SciPy -- W = U^-T Ct, z = U^-T r, mu = m0 + W^T z,
Sigma = A - W^T W, var = diag(A) - column norms -- with the exp() argument formed as ``timevar_reference.matrix_f64`` forms
it (``p * d * d``, then ``+ q * dt * dt``, every operation rounded on its own).

Run as a script it prints, per case, the error of the float64 evaluation against the long-double one: the table from which
tests/test_gpu_timevar_predict.py takes its bounds.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import grad_reference as gr  # noqa: E402  (puts the oracle and the repository on the path)
import timevar_reference as tr  # noqa: E402
from marg_predict_reference import Pred, errors  # noqa: E402,F401  (mu absolute; Sigma and var in units of the largest prior variance)

_LD = np.longdouble
MU_GP = tr.MU_GP
OUTPUTS = ("mu", "Sigma", "var")
DEFECTS = ("dt-swapped-in-one-factor", "tau-of-the-wrong-component", "no-temporal-factor-in-A", "no-temporal-factor-in-Cx",
           "q-without-the-half", "t_pred-at-the-block-offset")

# (case of timevar_reference.CASES, mode, M, dates): the smallest shapes at which a tile edge of either block of [K | Cx^T]
# can go wrong.  dates: "epoch" one observed epoch's date; "mid" midway between two epochs; "one" a date inside the span;
# "two" two dates inside the span, M split into two runs (the first the longer); "beyond" one span beyond the last epoch
PCASES = (
    ("N100-c2", 0, 50, "epoch"),        # R = 100, everything in one tile
    ("N100-c2", 1, 130, "mid"),         # R crosses a tile, the sum mode and its nugget
    ("N300-c1", 2, 129, "one"),
    ("N129-c2", 0, 65, "two"),          # 33 + 32 points, R = 130, N one pixel into the second tile
    ("N300-c3", 0, 43, "beyond"),       # R = 129
    ("N300-c2-perm", 0, 100, "two"),    # pixel times in no epoch order
    ("N520-c2", 0, 64, "two"),          # K crosses four block rows
)


def pcase_id(pc):
    return f"{pc[0]}-mode{pc[1]}-M{pc[2]}-{pc[3]}"


def tv_case(pc):
    case, = [c for c in tr.CASES if tr.case_id(c) == pc[0]]
    return case


def pcase_mus(pc):
    """prior means as tests/marg_predict_reference.py has them: one per component in mode 0, else MU_GP"""
    c = tv_case(pc)[1][1]
    return np.array([0.3, 0.2, 0.1][:c]) if pc[1] == 0 else np.array([MU_GP])


def pcase_dates(pc):
    """the dates of the case, in days from the first epoch"""
    ch = gr.case_chunk(tv_case(pc)[1])
    d = np.sort(ch.dates - ch.dates.min())
    span = float(d[-1])
    return {"epoch": [d[1]], "mid": [0.5 * (d[1] + d[2])], "one": [0.4 * span], "two": [0.25 * span, 0.75 * span],
            "beyond": [2.0 * span]}[pc[3]]


def pcase_pred(pc, dates=None):
    """-> (pred (c, M), t_pred (M,)): one run per date, each a linspace over the range of component 0's grid"""
    d = tr.case_data(tv_case(pc))
    dates = pcase_dates(pc) if dates is None else dates
    M, n = pc[2], len(dates)
    runs = [M // n + (1 if k < M % n else 0) for k in range(n)]
    lo, hi = np.min(d.lwls[0]), np.max(d.lwls[0])
    grid = np.concatenate([np.linspace(lo, hi, num=r) for r in runs])
    t_pred = np.concatenate([np.full(r, t) for r, t in zip(runs, dates)])
    return np.ascontiguousarray(np.tile(grid, (d.lwls.shape[0], 1))), np.ascontiguousarray(t_pred)


# ---- the pieces -----------------------------------------------------------------------------------------------------------
def _kernel(T, x_row, t_row, x_col, t_col, amp, l, tau, q_scale=-0.5, flip=False):
    """a^2 exp(p d^2 + q dt^2), (rows, columns), in the number type T and the device's operation order"""
    ckms = _LD("2.99792458e5") if T is _LD else T(2.99792458e5)
    D = np.asarray(x_col, dtype=T)[None, :] - np.asarray(x_row, dtype=T)[:, None]
    DT = np.asarray(t_col, dtype=T)[None, :] - np.asarray(t_row, dtype=T)[:, None]
    amp, l, tau = T(amp), T(l), T(tau)
    p = T(-0.5) * (ckms * ckms) / (l * l)
    q = T(q_scale) / (tau * tau)
    with np.errstate(under="ignore"):
        A = p * D * D
        A = A + q * DT * (-DT if flip else DT)
        return amp * amp * np.exp(A), A


def pieces(T, mode, lwls, times, pred, t_pred, mu_c, gp, tau, defect=None, want_args=False):
    """(Ct (N, R), A (R, R), m0 (R,), offset) in the number type T; ``defect``: one of DEFECTS seeded into the cross and prior
    fills (the faults a fill kernel or its host step can have); ``want_args``: the (c, N, M) arguments of Ct's exp() instead"""
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    pred = np.atleast_2d(np.asarray(pred, dtype=np.float64))
    c, M = lwls.shape[0], pred.shape[1]
    assert defect is None or defect in DEFECTS
    assert not (mode == 1 and c != 2) and not (mode == 2 and c != 1) and not (mode == 0 and c < 2)
    mu_c = [float(m) for m in np.atleast_1d(mu_c)]
    inf = float("inf")
    beyond = np.concatenate([np.asarray(t_pred, dtype=np.float64), np.zeros((c - 1) * M)])      # what lies behind t_pred
    cross, prior, args = [], [], []
    for k in range(c):
        amp, l = gp[2 * k], gp[2 * k + 1]
        tk = tau[(k + 1) % c] if defect == "tau-of-the-wrong-component" else tau[k]
        qs = -1.0 if defect == "q-without-the-half" else -0.5
        tp = beyond[k * M:(k + 1) * M] if (defect == "t_pred-at-the-block-offset" and mode == 0) else t_pred
        Ck, Ak = _kernel(T, lwls[k], times, pred[k], tp, amp, l, inf if defect == "no-temporal-factor-in-Cx" else tk, qs,
                         flip=defect == "dt-swapped-in-one-factor")
        Pk, _ = _kernel(T, pred[k], tp, pred[k], tp, amp, l, inf if defect == "no-temporal-factor-in-A" else tk, qs)
        Pk[np.diag_indices_from(Pk)] = T(amp) * T(amp)
        cross.append(Ck), prior.append(Pk), args.append(Ak)
    if want_args:
        return np.stack(args)
    if mode == 0:
        A = np.zeros((c * M, c * M), dtype=T)
        for k in range(c):
            A[k * M:(k + 1) * M, k * M:(k + 1) * M] = prior[k]
        return np.concatenate(cross, axis=1), A, np.concatenate([np.full(M, m, dtype=T) for m in mu_c]), T(1.0)
    Ct, A = cross[0], prior[0]
    for k in range(1, c):
        Ct, A = Ct + cross[k], A + prior[k]
    if mode == 1:
        A[np.diag_indices_from(A)] += T(1e-8)
    return Ct, A, np.full(M, mu_c[0], dtype=T), (T(1.0) if mode == 1 else T(mu_c[0]))


def cross_args_f64(lwls, times, pred, t_pred, gp, tau):
    """(c, N, M): the float64 arguments of exp() in the cross-covariance as the device forms them -- where one is <= -746 the
    device's exp() is exactly +0"""
    c = np.atleast_2d(lwls).shape[0]
    return pieces(np.float64, 0 if c > 1 else 2, lwls, times, pred, t_pred, np.zeros(c), gp, tau, want_args=True)


# ---- the two evaluations -----------------------------------------------------------------------------------------------
def data_cov_ext(lwls, times, sigma, gp, tau):
    K = tr.matrix_ext(lwls, times, gp, tau)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=_LD) ** 2
    return K


def tv_predict_ext(mode, lwls, times, fl, sigma, pred, t_pred, mu_c, gp, tau, defect=None, L=None) -> Pred:
    """every step in long double on the dense matrices (L: the factor of the data covariance where the caller has it)"""
    import oracle
    if L is None:
        L = oracle._chol_ext(data_cov_ext(lwls, times, sigma, gp, tau))
    Ct, A, m0, offset = pieces(_LD, mode, lwls, times, pred, t_pred, mu_c, gp, tau, defect)
    W = oracle._fsolve_ext(L, Ct)
    z = oracle._fsolve_ext(L, np.asarray(fl, dtype=_LD) - offset)
    Sigma = A - W.T @ W
    return Pred(m0 + W.T @ z, Sigma, np.diag(Sigma).copy(), np.max(np.diag(A)))


def tv_predict_f64(mode, lwls, times, fl, sigma, pred, t_pred, mu_c, gp, tau) -> Pred:
    """the device's route in float64: timevar_reference.matrix_f64, SciPy's cho_factor and triangular solves"""
    from scipy.linalg import cho_factor, solve_triangular
    K = tr.matrix_f64(lwls, times, gp, tau, sigma)
    U = cho_factor(K, lower=False)[0]
    Ct, A, m0, offset = pieces(np.float64, mode, lwls, times, pred, t_pred, mu_c, gp, tau)
    W = solve_triangular(U, Ct, trans="T", lower=False)
    z = solve_triangular(U, np.asarray(fl, dtype=np.float64) - offset, trans="T", lower=False)
    return Pred(m0 + W.T @ z, A - W.T @ W, np.diag(A) - np.sum(W * W, axis=0), np.max(np.diag(A)))


# ---- references of the cases, and the float64 table ---------------------------------------------------------------------
def pcase_args(pc, tau=None, dates=None):
    d = tr.case_data(tv_case(pc))
    pred, t_pred = pcase_pred(pc, dates)
    return (pc[1], d.lwls, d.times, d.fl, d.sigma, pred, t_pred, pcase_mus(pc), d.gp, d.tau if tau is None else np.asarray(tau, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def pcase_factor(pc):
    import oracle
    d = tr.case_data(tv_case(pc))
    L = oracle._chol_ext(data_cov_ext(d.lwls, d.times, d.sigma, d.gp, d.tau))
    L.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
def pcase_ext(pc) -> Pred:
    ref = tv_predict_ext(*pcase_args(pc), L=pcase_factor(pc))
    for a in (ref.mu, ref.Sigma, ref.var):
        a.setflags(write=False)
    return ref


def measure_f64():
    rows = []
    for pc in PCASES:
        f = tv_predict_f64(*pcase_args(pc))
        rows.append((pcase_id(pc), errors(f.mu, f.Sigma, f.var, pcase_ext(pc))))
    return rows


if __name__ == "__main__":
    rows = measure_f64()
    print(f"{'case':32s} " + " ".join(f"{k:>10s}" for k in OUTPUTS))
    for name, err in rows:
        print(f"{name:32s} " + " ".join(f"{err[k]:10.2e}" for k in OUTPUTS))
    print(f"{'max':32s} " + " ".join(f"{max(r[1][k] for r in rows):10.2e}" for k in OUTPUTS))
