"""CPU references for the component spectra under the marginalised continuum (tests/test_marg_predict_reference.py,
tests/test_gpu_marg_predict.py): the conditional of the plain predict modes with Kt = K + H Lambda H^T as data covariance.

    r = fl - offset, Cx (R x N), A, m0 as the plain mode has them (oracle.predict_ext);  H, Lambda as tests/marg_reference.py
    mu = m0 + Cx Kt^-1 r,   Sigma = A - Cx Kt^-1 Cx^T

``marg_predict_ext`` forms the dense C = K + H Lambda H^T in np.longdouble, factors it with the oracle's long-double
Cholesky and solves with it -- no Woodbury identity, so it is independent of the device's route.  ``marg_predict_f64`` is
the device's route (Wc = U^-T Cx^T, Wh = U^-T H Lambda^1/2, M = I + Wh^T Wh, G = Wh^T Wc, Y = U_M^-T G, ...) in float64
with SciPy.

Run as a script it prints, per case and weight, the error of the float64 evaluation against the long-double one: the
table from which tests/test_gpu_marg_predict.py takes its bounds.
"""
from __future__ import annotations

import functools
import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "oracle"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import marg_reference as mr  # noqa: E402
from loo_reference import _matrix_ext  # noqa: E402

_LD = np.longdouble
MU_GP = mr.MU_GP
WEIGHTS = mr.WEIGHTS
OUTPUTS = ("mu", "Sigma", "var")

# (chunk of marg_reference.CASES, mode, M): the smallest shapes at which a tile edge of each of the three column blocks of
# [K | Cx^T | Ht] can go wrong
PCASES = (
    ("a", 0, 50),       # N 100, c 2: R = 100, everything in one tile
    ("a", 1, 130),      # R crosses a tile, the sum mode and its nugget
    ("b", 2, 128),      # N 128, c 1: exact tiles
    ("c", 0, 65),       # N 129, c 2: R = 130, N one pixel into the second tile
    ("d", 2, 129),      # N 384, c 1: epoch edges on tile edges
    ("e", 0, 43),       # N 300, c 3: R = 129, an empty epoch, runs out of id order
    ("f", 0, 100),      # N 312, c 2, q = 130 (Q = 2): R = 200; [M | G] crosses a block row in both blocks
)


def pcase_id(pc):
    return f"{mr.case_id(mr.case_named(pc[0]))}-mode{pc[1]}-M{pc[2]}"


def pcase_mus(pc):
    """prior means: one per component in mode 0 (the offset there is the reference's fixed 1.0); MU_GP -- prior mean and
    offset -- in mode 2, prior mean in mode 1"""
    c = mr.case_named(pc[0])[2]
    return np.array([0.3, 0.2, 0.1][:c]) if pc[1] == 0 else np.array([MU_GP])


def pcase_pred(pc):
    """the prediction grids of retrieve_components: linspace over the range of component 0's grid, the same for every component"""
    ch = mr.case_chunk(mr.case_named(pc[0]))
    g = np.linspace(np.min(ch.lwls[0]), np.max(ch.lwls[0]), num=pc[2])
    return np.ascontiguousarray(np.tile(g, (ch.lwls.shape[0], 1)))


@dataclass
class Pred:
    mu: np.ndarray
    Sigma: np.ndarray
    var: np.ndarray
    prior_max: object       # the largest prior variance: the unit of the Sigma and var errors


# ---- the pieces of the plain modes ---------------------------------------------------------------------------------------
def pieces_ext(mode, lwls, pred, mu_c, gp):
    """(Ct (N, R), A (R, R), m0 (R,), offset) of ``oracle.predict_ext``'s ``mode`` in long double"""
    import oracle
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    pred = np.atleast_2d(np.asarray(pred, dtype=np.float64))
    c, M = lwls.shape[0], pred.shape[1]
    mu_c = [float(m) for m in np.atleast_1d(mu_c)]
    if mode == 0:
        Ct = np.concatenate([oracle._fill_ext(lwls[k], pred[k], gp[2 * k], gp[2 * k + 1]) for k in range(c)], axis=1)
        A = np.zeros((c * M, c * M), dtype=_LD)
        for k in range(c):
            A[k * M:(k + 1) * M, k * M:(k + 1) * M] = oracle._sym_ext(pred[k:k + 1], gp[2 * k:2 * k + 2])
        return Ct, A, np.concatenate([np.full(M, m, dtype=_LD) for m in mu_c]), _LD(1.0)
    assert not (mode == 1 and c != 2) and not (mode == 2 and c != 1)
    Ct = sum(oracle._fill_ext(lwls[k], pred[k], gp[2 * k], gp[2 * k + 1]) for k in range(c))
    A = sum(oracle._sym_ext(pred[k:k + 1], gp[2 * k:2 * k + 2]) for k in range(c))
    if mode == 1:
        A[np.diag_indices_from(A)] += _LD(1e-8)
    return Ct, A, np.full(M, mu_c[0], dtype=_LD), (_LD(1.0) if mode == 1 else _LD(mu_c[0]))


def pieces_f64(mode, lwls, pred, mu_c, gp):
    """the same from the oracle's float64 fills (the numbers the device's fills are pinned to)"""
    import oracle
    lwls = np.ascontiguousarray(np.atleast_2d(lwls), dtype=np.float64)
    pred = np.ascontiguousarray(np.atleast_2d(pred), dtype=np.float64)
    (c, N), M = lwls.shape, pred.shape[1]
    cross, prior = [], []
    for k in range(c):
        t = np.empty((N, M))
        oracle.fill_V12_f(t, lwls[k], pred[k], gp[2 * k], gp[2 * k + 1])
        cross.append(t)
        t = np.empty((M, M))
        oracle.fill_V11_f(t, pred[k], gp[2 * k], gp[2 * k + 1])
        prior.append(t)
    if mode == 0:
        A = np.zeros((c * M, c * M))
        for k in range(c):
            A[k * M:(k + 1) * M, k * M:(k + 1) * M] = prior[k]
        return np.concatenate(cross, axis=1), A, np.concatenate([np.full(M, float(m)) for m in mu_c]), 1.0
    Ct, A = cross[0], prior[0]
    for k in range(1, c):
        Ct, A = Ct + cross[k], A + prior[k]
    if mode == 1:
        A = A + 1e-8 * np.eye(M)
    return Ct, A, np.full(M, float(mu_c[0])), (1.0 if mode == 1 else float(mu_c[0]))


# ---- the two evaluations -----------------------------------------------------------------------------------------------
def marg_predict_ext(mode, lwls, fl, sigma, pred, mu_c, gp, x, epoch_index, n_epochs, order, sd, weight=None) -> Pred:
    """every step in long double, on the dense K + H Lambda H^T"""
    import oracle
    K = _matrix_ext(lwls, sigma, gp)
    H = mr.basis(x, epoch_index, n_epochs, order, weight, T=_LD)
    lam = np.tile(np.asarray(sd, dtype=_LD) ** 2, n_epochs)
    C = K + (H * lam[None, :]) @ H.T
    C = _LD(0.5) * (C + C.T)
    Ct, A, m0, offset = pieces_ext(mode, lwls, pred, mu_c, gp)
    L = oracle._chol_ext(C)
    W = oracle._fsolve_ext(L, Ct)
    z = oracle._fsolve_ext(L, np.asarray(fl, dtype=_LD) - offset)
    Sigma = A - W.T @ W
    Sigma = _LD(0.5) * (Sigma + Sigma.T)
    return Pred(m0 + W.T @ z, Sigma, np.diag(Sigma).copy(), np.max(np.diag(A)))


def plain_predict_ext(mode, lwls, fl, sigma, pred, mu_c, gp):
    """the oracle's plain predict, long double"""
    import oracle
    mu, Sigma = oracle.predict_ext(mode, lwls, fl, sigma, pred, mu_c, gp)
    return mu, _LD(0.5) * (Sigma + Sigma.T)


def marg_predict_f64(mode, lwls, fl, sigma, pred, mu_c, gp, x, epoch_index, n_epochs, order, sd, weight=None) -> Pred:
    """the device's formulae in float64: the oracle's fills, SciPy's cho_factor and triangular solves"""
    import oracle
    from scipy.linalg import cho_factor, solve_triangular
    lwls = np.ascontiguousarray(np.atleast_2d(lwls), dtype=np.float64)
    gp = np.asarray(gp, dtype=np.float64)
    N = lwls.shape[1]
    K = np.empty((N, N))
    oracle.fill_sym(K, lwls, gp)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=np.float64) ** 2
    U = cho_factor(K, lower=False)[0]
    s = np.tile(np.asarray(sd, dtype=np.float64), n_epochs)
    Ht = mr.basis(x, epoch_index, n_epochs, order, weight) * s[None, :]
    Ct, A, m0, offset = pieces_f64(mode, lwls, pred, mu_c, gp)
    Wc = solve_triangular(U, Ct, trans="T", lower=False)
    Wh = solve_triangular(U, Ht, trans="T", lower=False)
    z = solve_triangular(U, np.asarray(fl, dtype=np.float64) - offset, trans="T", lower=False)
    UM = cho_factor(np.eye(Ht.shape[1]) + Wh.T @ Wh, lower=False)[0]
    Y = solve_triangular(UM, Wh.T @ Wc, trans="T", lower=False)
    y = solve_triangular(UM, Wh.T @ z, trans="T", lower=False)
    mu = m0 + (Wc.T @ z - Y.T @ y)
    Sigma = A - Wc.T @ Wc + Y.T @ Y
    var = (np.diag(A) - np.sum(Wc * Wc, axis=0)) + np.sum(Y * Y, axis=0)
    return Pred(mu, Sigma, var, np.max(np.diag(A)))


# ---- references of the cases, and the float64 table ---------------------------------------------------------------------
def pcase_args(pc, kind, sd=None):
    case = mr.case_named(pc[0])
    ch = mr.case_chunk(case)
    return (pc[1], ch.lwls, ch.fl, ch.sigma, pcase_pred(pc), pcase_mus(pc), mr.case_gp(case), ch.x, ch.epoch_index, ch.n_epochs,
            ch.order, mr.prior_sd(ch.order) if sd is None else sd, mr.case_weight(case, kind))


@functools.lru_cache(maxsize=None)
def pcase_ext(pc, kind) -> Pred:
    ref = marg_predict_ext(*pcase_args(pc, kind))
    for a in (ref.mu, ref.Sigma, ref.var):
        a.setflags(write=False)
    return ref


def errors(mu, Sigma, var, ref: Pred) -> dict:
    """per output the error measure of tests/test_gpu_marg_predict.py: mu absolute; Sigma and var absolute in units of the
    largest prior variance; an output that is None is left out"""
    def ld(v):
        return np.asarray(v, dtype=_LD)

    out = {"mu": float(np.max(np.abs(ld(mu) - ref.mu)))}
    if Sigma is not None:
        out["Sigma"] = float(np.max(np.abs(ld(Sigma) - ref.Sigma)) / ref.prior_max)
    if var is not None:
        out["var"] = float(np.max(np.abs(ld(var) - ref.var)) / ref.prior_max)
    return out


def measure_f64():
    rows = []
    for pc in PCASES:
        for kind in WEIGHTS:
            f = marg_predict_f64(*pcase_args(pc, kind))
            rows.append((f"{pcase_id(pc)}-{kind}", errors(f.mu, f.Sigma, f.var, pcase_ext(pc, kind))))
    return rows


if __name__ == "__main__":
    rows = measure_f64()
    print(f"{'case':32s} " + " ".join(f"{k:>10s}" for k in OUTPUTS))
    for name, err in rows:
        print(f"{name:32s} " + " ".join(f"{err[k]:10.2e}" for k in OUTPUTS))
    print(f"{'max':32s} " + " ".join(f"{max(r[1][k] for r in rows):10.2e}" for k in OUTPUTS))
