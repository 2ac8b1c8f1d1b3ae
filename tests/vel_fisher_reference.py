"""CPU references for the epoch-velocity Fisher information (tests/test_vel_fisher_reference.py, tests/test_gpu_vel_fisher.py).

The tangent of v[c, e] moves the grid of component c on the pixels of epoch e: dx = -1 / c_kms there, zero elsewhere.  With
d = x_c[n] - x_c[m], p_c = -1/2 c_kms^2 / l_c^2, G = K^-1 and the antisymmetric, cross-epoch-only

    Dv_c[m, n] = a_c^2 2 p_c d exp(p_c d^2) / c_kms * [epoch(m) != epoch(n)]

the covariance derivative of v[c, e] is P_e R + R^T P_e^T, R the rows of Dv_c in epoch e, and with Z_c = G Dv_c
(A_c = Dv_c G = -Z_c^T) and X_cc' = Dv_c G Dv_c'^T = Z_c^T Dv_c'

    F[(c, e), (c', f)] = sum over m in e, n in f of ( A_c[m, n] A_c'[n, m] + G[n, m] X_cc'[m, n] )

``vel_fisher_f64`` is that in float64 with SciPy's ``cho_factor``; the long-double truth is ``fisher_reference.fisher_ext``
with the c E tangents of ``vel_tangents``.  Row c * E + e: the order of grad_vel.  F has c null directions, one constant
shift per component (the kernel is stationary), and is the information of the velocities AT FIXED hyper-parameters.

``cpu_fit`` runs the Fisher-scoring loop of psoap_amd.lnprob.epoch_velocities (``velocity_scoring``) on
grad_reference.grad_f64 + vel_fisher_f64: the CPU twin of the fit.

Run as a script it prints, per case, max |f64 - long double| / sqrt(F_ss F_tt): the table from which
tests/test_gpu_vel_fisher.py takes its bound.
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

import fisher_reference as fr  # noqa: E402
import grad_reference as gr  # noqa: E402

C_KMS = fr.C_KMS
CASES = fr.CASES
# c = 3, 12 (11) epochs x 30 pixels cut to N = 300 by case_chunk's recipe: c E = 36 (33), more than the generic path takes
CASE_36 = (300, 3, 12, 30)
CASE_33 = (300, 3, 11, 30)
# Seeded defects of the structured formula that must leave the bound.  "within_epoch_upper": the within-epoch block kept above
# the diagonal only.  Kept on BOTH sides it is no defect ("within_epoch_kept", NOT_A_DEFECT): Dv_c stays antisymmetric, the
# within-epoch block of P_e R + R^T P_e^T cancels and F is the same to rounding -- the exact zeros save work, not correctness.
DEFECTS = ("within_epoch_upper", "aat_dropped", "gx_dropped", "dv_sign", "cross_transposed", "half")
NOT_A_DEFECT = "within_epoch_kept"


def vel_tangents(case):
    """(tan_lwl (c E, c, N), tan_gp (c E, 2c) zeros): dx = -1/c_kms on component c, epoch e, row c * E + e"""
    N, c, ne, _ = case
    ep = gr.case_chunk(case).epoch_index
    return epoch_tangents(c, N, ep, ne)


def epoch_tangents(c, N, epoch_index, n_epochs):
    tan = np.zeros((c * n_epochs, c, N))
    for k in range(c):
        for e in range(n_epochs):
            tan[k * n_epochs + e, k, np.asarray(epoch_index) == e] = -1.0 / C_KMS
    return tan, np.zeros((c * n_epochs, 2 * c))


def dv_matrices(lwls, gp, epoch_index, defect=None):
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    ep = np.asarray(epoch_index)
    cross = ep[:, None] != ep[None, :]
    out = []
    for k in range(lwls.shape[0]):
        a, l = float(gp[2 * k]), float(gp[2 * k + 1])
        p = -0.5 * C_KMS * C_KMS / (l * l)
        D = lwls[k][None, :] - lwls[k][:, None]
        M = a * a * 2.0 * p * D * np.exp(p * D * D) / C_KMS
        if defect == "within_epoch_upper":
            M = M * (cross | np.triu(np.ones_like(cross)))
        elif defect != "within_epoch_kept":
            M = M * cross
        if defect == "dv_sign" and k == lwls.shape[0] - 1:
            M = np.where(np.triu(np.ones_like(M, dtype=bool)), M, -M)      # a sign lost below the diagonal: symmetric, not antisymmetric
        out.append(M)
    return out


def vel_fisher_from_inverse(G, Dv, epoch_index, n_epochs, defect=None):
    """the structured formula from G = K^-1 and the c matrices Dv_c"""
    c, N = len(Dv), G.shape[0]
    B = np.zeros((N, n_epochs))
    B[np.arange(N), np.asarray(epoch_index)] = 1.0
    A = [d @ G for d in Dv]
    F = np.zeros((c * n_epochs, c * n_epochs))
    for k in range(c):
        for j in range(k + 1):
            X = A[k] @ Dv[j].T
            T = np.zeros((N, N))
            if defect != "aat_dropped":
                T += A[k] * A[j].T
            if defect != "gx_dropped":
                T += G.T * X
            if defect == "half":
                T *= 0.5
            blk = B.T @ T @ B
            F[k * n_epochs:(k + 1) * n_epochs, j * n_epochs:(j + 1) * n_epochs] = blk
            if j != k:
                F[j * n_epochs:(j + 1) * n_epochs, k * n_epochs:(k + 1) * n_epochs] = blk if defect == "cross_transposed" else blk.T
    return F


def vel_fisher_f64(lwls, sigma, gp, epoch_index, n_epochs, defect=None):
    """F (c E, c E) in float64: the oracle's fill, SciPy's cho_factor, K^-1 from cho_solve, the structured formula"""
    import oracle
    from scipy.linalg import cho_factor, cho_solve
    lwls = np.ascontiguousarray(np.atleast_2d(lwls), dtype=np.float64)
    gp = np.asarray(gp, dtype=np.float64)
    N = lwls.shape[1]
    K = np.empty((N, N))
    oracle.fill_sym(K, lwls, gp)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=np.float64) ** 2
    G = cho_solve(cho_factor(K, lower=False), np.eye(N))
    return vel_fisher_from_inverse(G, dv_matrices(lwls, gp, epoch_index, defect), epoch_index, n_epochs, defect)


@functools.lru_cache(maxsize=None)
def case_ext(case):
    """the long-double truth: fisher_reference.fisher_ext with the c E velocity tangents"""
    ch = gr.case_chunk(case)
    F, _ = fr.fisher_ext(ch.lwls, ch.sigma, gr.case_gp(case), *vel_tangents(case))
    F.setflags(write=False)
    return F


def case_f64(case, defect=None):
    ch = gr.case_chunk(case)
    return vel_fisher_f64(ch.lwls, ch.sigma, gr.case_gp(case), ch.epoch_index, case[2], defect)


def null_vectors(c, n_epochs):
    """(c, c E): the constant shift of each component"""
    u = np.zeros((c, c * n_epochs))
    for k in range(c):
        u[k, k * n_epochs:(k + 1) * n_epochs] = 1.0
    return u


def null_residual(F, c, n_epochs):
    """max over components and rows of |F u_c|_s / (sqrt(F_ss) sum_t sqrt(F_tt))"""
    d = np.sqrt(np.abs(np.diag(np.asarray(F, dtype=np.float64))))
    scale = d * np.sum(d)
    scale[scale == 0.0] = 1.0
    return float(max(np.max(np.abs(np.asarray(F, dtype=np.float64) @ u) / scale) for u in null_vectors(c, n_epochs)))


rel_to_scale = fr.rel_to_scale


# ---- the fit ----------------------------------------------------------------------------------------------------------
# Fisher scoring converges linearly (the information is the EXPECTED curvature, the data's own differs), and on chunks this
# small 20 iterations are often not enough: of the seeds 7903 .. 7924, with the flux drawn from the model itself, three
# reach a decrement of 1e-10 within 20 iterations from both starts (7905 .. 7908 .. 7917; measured with this module).
# 7917 does in 15 and 17.
FIT_SEED = 7917
FIT_OFFSET_SEED = 7901
FIT_MU = 1.0


@functools.lru_cache(maxsize=None)
def fit_chunk():
    """the synthetic SB2 chunk of the fit tests: 6 epochs x 50 pixels (N = 300) of syn.make_chunk, its flux replaced by a
    seeded draw from the model itself -- N(FIT_MU, K + sigma^2) at the chunk's velocities and the benchmark
    hyper-parameters -- so that the information describes the likelihood it is used on"""
    import dataclasses
    import oracle
    from psoap_amd import synthetic as syn
    ch = syn.make_chunk(2, 6, 50, seed=FIT_SEED)
    K = np.empty((ch.N, ch.N))
    oracle.fill_sym(K, np.ascontiguousarray(ch.lwls), fit_gp())
    K[np.diag_indices_from(K)] += ch.sigma ** 2
    fl = FIT_MU + np.linalg.cholesky(K) @ np.random.default_rng(FIT_SEED + 50).standard_normal(ch.N)
    return dataclasses.replace(ch, fl=np.ascontiguousarray(fl))


def fit_gp():
    from psoap_amd import synthetic as syn
    return np.array(syn.GP_BASE[2], dtype=np.float64)


def cpu_fit(ch, gp, vel0, mu_GP=FIT_MU, max_iter=20, tol=1e-10):
    """psoap_amd.lnprob.velocity_scoring -- the loop of epoch_velocities -- on grad_reference.grad_f64 + vel_fisher_f64"""
    from psoap_amd.lnprob import velocity_scoring
    ep, E, c = ch.epoch_index, ch.n_epochs, ch.n_components

    def grids(vel):
        return ch.lwl[None, :] + (-vel[:, ep]) / C_KMS

    def value(vel):
        return gr.grad_f64(grids(vel), ch.fl, ch.sigma, gp, mu_GP).lnp

    def grad_info(vel):
        lw = grids(vel)
        g = gr.grad_f64(lw, ch.fl, ch.sigma, gp, mu_GP)
        gv = np.array([-np.bincount(ep, weights=g.lwl[k], minlength=E) / C_KMS for k in range(c)])
        return gv, vel_fisher_f64(lw, ch.sigma, gp, ep, E)

    return velocity_scoring(value, grad_info, vel0, np.bincount(ep, minlength=E) > 0, max_iter, tol)


@functools.lru_cache(maxsize=None)
def cpu_fit_optimum():
    """the CPU twin's velocities on fit_chunk from the chunk's true velocities, and the start of the fit tests: 1 km/s off
    it along a seeded direction of zero mean per component (the null directions are never moved)"""
    ch = fit_chunk()
    fit = cpu_fit(ch, fit_gp(), ch.velocities)
    d = np.random.default_rng(FIT_OFFSET_SEED).standard_normal(fit["vel"].shape)
    d -= d.mean(axis=1, keepdims=True)
    d /= np.max(np.abs(d))
    return fit, fit["vel"] + d


def measure_f64():
    return [(fr.case_id(case), rel_to_scale(case_f64(case), case_ext(case))) for case in CASES]


if __name__ == "__main__":
    rows = measure_f64()
    print(f"{'case':10s} {'F':>10s}")
    for name, a in rows:
        print(f"{name:10s} {a:10.2e}")
    print(f"{'max':10s} {max(r[1] for r in rows):10.2e}")
