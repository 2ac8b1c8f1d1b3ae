"""CPU references for the Fisher information of the GP likelihood (tests/test_fisher_reference.py, tests/test_gpu_fisher.py).

    K[m,n] = sum_c a_c^2 exp(p_c d^2) + sigma_m^2 delta_mn,  d = x_c[n] - x_c[m],  p_c = -1/2 c_kms^2 / l_c^2

A tangent t is a direction (dx_t (c, N), da_tc, dl_tc) in (grid, hyper-parameter) space; with e = exp(p_c d^2)

    K_t[m,n] = sum_c e (2 a_c da_tc + a_c^2 c_kms^2 / l_c^3 d^2 dl_tc + a_c^2 2 p_c d (dx_tc[n] - dx_tc[m]))
    F_st     = 1/2 tr(K^-1 K_s K^-1 K_t)            F_mu = 1^T K^-1 1

Two evaluations of the same formulas: ``fisher_ext`` in np.longdouble on the long-double helpers of the oracle (with
K = L L^T, P_t = L^-1 K_t L^-T and F_st = 1/2 sum P_s P_t), ``fisher_f64`` in float64 with SciPy's ``cho_factor`` /
``cho_solve`` (G_t = K^-1 K_t K^-1, F_st = 1/2 sum K_s G_t).  F is positive semi-definite, so sqrt(F_ss F_tt) bounds |F_st|:
that is the scale an error of F_st is measured against; F_mu is measured against itself.

Run as a script it prints, per case, max_st |f64 - long double| / sqrt(F_ss F_tt) and |f64 - long double| / F_mu: the table
from which tests/test_gpu_fisher.py takes its bounds.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "oracle"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import grad_reference as gr  # noqa: E402

_LD = np.longdouble
C_KMS = 2.99792458e5

# grad_reference's cases without N = 520: one tile, exactly one tile, one tile plus one row, three tiles with a ragged edge
CASES = tuple(case for case in gr.CASES if case[0] != 520)
case_id, case_chunk, case_gp = gr.case_id, gr.case_chunk, gr.case_gp


def tangent_matrix(lwls, gp, dx, dgp, T=np.float64):
    """K_t (N, N) of one tangent (dx (c, N), dgp (2c,)) in the number type ``T``"""
    lwls = np.atleast_2d(lwls)
    c, N = lwls.shape
    ckms = T("2.99792458e5") if T is _LD else T(C_KMS)
    out = np.zeros((N, N), dtype=T)
    for k in range(c):
        a, l = T(gp[2 * k]), T(gp[2 * k + 1])
        da, dl = T(dgp[2 * k]), T(dgp[2 * k + 1])
        x, u = np.asarray(lwls[k], dtype=T), np.asarray(dx[k], dtype=T)
        D = x[None, :] - x[:, None]
        p = T(-0.5) * ckms * ckms / (l * l)
        E = np.exp(p * D * D)
        out += E * (T(2) * a * da + a * a * (ckms * ckms) / (l * l * l) * (D * D) * dl
                    + a * a * T(2) * p * D * (u[None, :] - u[:, None]))
    return out


def fisher_ext(lwls, sigma, gp, tan_lwl, tan_gp):
    """(F (T, T), F_mu) with every step in long double"""
    import oracle
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    N = lwls.shape[1]
    K = oracle._sym_ext(lwls, gp)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=_LD) ** 2
    L = oracle._chol_ext(K)
    Li = oracle._fsolve_ext(L, np.eye(N, dtype=_LD))          # L^-1
    P = []
    for dx, dgp in zip(tan_lwl, tan_gp):
        P.append(Li @ tangent_matrix(lwls, gp, dx, dgp, _LD) @ Li.T)
    T = len(P)
    F = np.zeros((T, T), dtype=_LD)
    for s in range(T):
        for t in range(s, T):
            F[s, t] = F[t, s] = _LD(0.5) * np.sum(P[s] * P[t])
    y = Li @ np.ones(N, dtype=_LD)
    return F, y @ y


def fisher_f64(lwls, sigma, gp, tan_lwl, tan_gp):
    """the same in float64: the oracle's fill, SciPy's cho_factor, K^-1 from cho_solve"""
    import oracle
    lwls = np.ascontiguousarray(np.atleast_2d(lwls), dtype=np.float64)
    gp = np.asarray(gp, dtype=np.float64)
    N = lwls.shape[1]
    K = np.empty((N, N))
    oracle.fill_sym(K, lwls, gp)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=np.float64) ** 2
    return fisher_from_matrices(K, [tangent_matrix(lwls, gp, dx, dgp) for dx, dgp in zip(tan_lwl, tan_gp)])


def fisher_from_matrices(K, Kt):
    """(F, F_mu) in float64 from K and the list of covariance derivatives K_t, whatever made them"""
    from scipy.linalg import cho_factor, cho_solve
    N = K.shape[0]
    factor = cho_factor(K, lower=False)
    Kinv = cho_solve(factor, np.eye(N))
    G = [Kinv @ k @ Kinv for k in Kt]
    T = len(Kt)
    F = np.array([[0.5 * np.sum(Kt[s] * G[t]) for t in range(T)] for s in range(T)])
    return F, float(np.ones(N) @ cho_solve(factor, np.ones(N)))


@functools.lru_cache(maxsize=None)
def case_tangents(case):
    """(tan_lwl (T, c, N), tan_gp (T, 2c)), T = 2c + 3: the 2c hyper-parameter unit tangents; two velocity tangents,
    dx = -1/c_kms on the pixels of the first epoch of the first component and of the last epoch of the last component;
    one seeded random dx (normal, in units of 1 km/s)"""
    N, c, ne, _ = case
    ch = case_chunk(case)
    T = 2 * c + 3
    tan_lwl, tan_gp = np.zeros((T, c, N)), np.zeros((T, 2 * c))
    tan_gp[:2 * c] = np.eye(2 * c)
    ep = ch.epoch_index
    tan_lwl[2 * c, 0, ep == 0] = -1.0 / C_KMS
    tan_lwl[2 * c + 1, c - 1, ep == ne - 1] = -1.0 / C_KMS
    tan_lwl[2 * c + 2] = np.random.default_rng(7700 + N + c).standard_normal((c, N)) / C_KMS
    tan_lwl.setflags(write=False)
    tan_gp.setflags(write=False)
    return tan_lwl, tan_gp


def fd_step(case, t):
    """the step of a central difference along tangent t of ``case_tangents``: 2 % of the hyper-parameter, 0.05 km/s"""
    c = case[1]
    return 0.02 * case_gp(case)[t] if t < 2 * c else 0.05


@functools.lru_cache(maxsize=None)
def case_ext(case):
    ch = case_chunk(case)
    F, F_mu = fisher_ext(ch.lwls, ch.sigma, case_gp(case), *case_tangents(case))
    F.setflags(write=False)
    return F, F_mu


def rel_to_scale(got, ref):
    """max_st |got - ref| / sqrt(ref_ss ref_tt)"""
    got, ref = np.asarray(got, dtype=_LD), np.asarray(ref, dtype=_LD)
    d = np.sqrt(np.diag(ref))
    return float(np.max(np.abs(got - ref) / np.outer(d, d)))


def measure_f64():
    rows = []
    for case in CASES:
        ch = case_chunk(case)
        F, F_mu = case_ext(case)
        f, f_mu = fisher_f64(ch.lwls, ch.sigma, case_gp(case), *case_tangents(case))
        rows.append((case_id(case), rel_to_scale(f, F), float(abs(_LD(f_mu) - F_mu) / F_mu)))
    return rows


if __name__ == "__main__":
    rows = measure_f64()
    print(f"{'case':10s} {'F':>10s} {'F_mu':>10s}")
    for name, a, b in rows:
        print(f"{name:10s} {a:10.2e} {b:10.2e}")
    print(f"{'max':10s} " + " ".join(f"{max(r[k] for r in rows):10.2e}" for k in (1, 2)))
