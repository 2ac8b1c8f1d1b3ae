"""CPU references for the gradient of the GP log-likelihood (tests/test_grad_reference.py, tests/test_gpu_grad.py).

    lnL = -1/2 (r^T K^-1 r + log det K),  r = fl - mu_GP,
    K_ij = sum_c a_c^2 exp(p_c d_cij^2) + sigma_i^2 delta_ij,  d_cij = x_c[j] - x_c[i],  p_c = -1/2 c_kms^2 / l_c^2

With alpha = K^-1 r, Q = alpha alpha^T - K^-1 and k_cij = a_c^2 exp(p_c d_cij^2):

    dlnL/da_c    = 1/2 sum_ij Q_ij 2 k_cij / a_c
    dlnL/dl_c    = 1/2 sum_ij Q_ij k_cij c_kms^2 d_cij^2 / l_c^3
    dlnL/dx_c[i] = sum_j Q_ij k_cij (-2 p_c d_cij)
    dlnL/dmu_GP  = sum_i alpha_i

Two evaluations of the same formulas from the explicit inverse: ``grad_ext`` in np.longdouble on the long-double helpers of
the oracle, ``grad_f64`` in float64 with SciPy's ``cho_factor`` / ``cho_solve``.  Both also return, per output, the
cancellation scale S = 1/2 sum_ij |Q_ij| |dK_ij/dtheta| of its sum (sum_i |alpha_i| for mu_GP): what an error of the sum is
measured against.
"""
from __future__ import annotations

import functools
import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "oracle"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from psoap_amd import synthetic as syn  # noqa: E402

_LD = np.longdouble
MU_GP = 0.9


@dataclass(frozen=True)
class Grad:
    lnp: float
    gp: np.ndarray        # (2c,)
    lwl: np.ndarray       # (c, N)
    mu: float
    s_gp: np.ndarray      # the scales of the same shapes
    s_lwl: np.ndarray
    s_mu: float


def _contract(Q, lwls, gp, alpha, T):
    """the four formulas, and their scales, from Q in the number type ``T``"""
    c, N = lwls.shape
    ckms = T("2.99792458e5") if T is _LD else T(2.99792458e5)
    aQ = np.abs(Q)
    g_gp, s_gp = np.zeros(2 * c, dtype=T), np.zeros(2 * c, dtype=T)
    g_x, s_x = np.zeros((c, N), dtype=T), np.zeros((c, N), dtype=T)
    for k in range(c):
        a, l = T(gp[2 * k]), T(gp[2 * k + 1])
        x = np.asarray(lwls[k], dtype=T)
        D = x[None, :] - x[:, None]
        p = T(-0.5) * ckms * ckms / (l * l)
        Kc = a * a * np.exp(p * D * D)
        g_gp[2 * k] = T(0.5) * np.sum(Q * (T(2) * Kc / a))
        s_gp[2 * k] = T(0.5) * np.sum(aQ * np.abs(T(2) * Kc / a))
        dl = Kc * (ckms * ckms) * (D * D) / (l * l * l)
        g_gp[2 * k + 1] = T(0.5) * np.sum(Q * dl)
        s_gp[2 * k + 1] = T(0.5) * np.sum(aQ * np.abs(dl))
        dx = Kc * (T(-2) * p * D)
        g_x[k] = np.sum(Q * dx, axis=1)
        s_x[k] = np.sum(aQ * np.abs(dx), axis=1)
    return g_gp, g_x, np.sum(alpha), s_gp, s_x, np.sum(np.abs(alpha))


def grad_ext(lwls, fl, sigma, gp, mu_GP=1.0) -> Grad:
    """every step in long double: K, its Cholesky factor, the explicit inverse, the contraction"""
    import oracle
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    N = lwls.shape[1]
    K = oracle._sym_ext(lwls, gp)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=_LD) ** 2
    L = oracle._chol_ext(K)
    Li = oracle._fsolve_ext(L, np.eye(N, dtype=_LD))          # L^-1
    r = np.asarray(fl, dtype=_LD) - _LD(mu_GP)
    z = Li @ r
    alpha = Li.T @ z
    Kinv = Li.T @ Li
    lnp = _LD(-0.5) * (z @ z + _LD(2) * np.sum(np.log(np.diag(L))))
    g_gp, g_x, g_mu, s_gp, s_x, s_mu = _contract(np.outer(alpha, alpha) - Kinv, lwls, gp, alpha, _LD)
    return Grad(float(lnp), g_gp, g_x, g_mu, s_gp, s_x, s_mu)


def grad_f64(lwls, fl, sigma, gp, mu_GP=1.0) -> Grad:
    """the same in float64: the oracle's fill, SciPy's cho_factor, K^-1 and alpha from cho_solve"""
    import oracle
    from scipy.linalg import cho_factor, cho_solve
    lwls = np.ascontiguousarray(np.atleast_2d(lwls), dtype=np.float64)
    gp = np.asarray(gp, dtype=np.float64)
    N = lwls.shape[1]
    K = np.empty((N, N))
    oracle.fill_sym(K, lwls, gp)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=np.float64) ** 2
    factor = cho_factor(K, lower=False)
    r = np.asarray(fl, dtype=np.float64) - mu_GP
    alpha = cho_solve(factor, r)
    Kinv = cho_solve(factor, np.eye(N))
    lnp = -0.5 * (r @ alpha + np.sum(2 * np.log(np.diag(factor[0]))))
    g_gp, g_x, g_mu, s_gp, s_x, s_mu = _contract(np.outer(alpha, alpha) - Kinv, lwls, gp, alpha, np.float64)
    return Grad(float(lnp), g_gp, g_x, float(g_mu), s_gp, s_x, float(s_mu))


# ---- the cases of tests/test_gpu_grad.py ------------------------------------------------------------------------------
# (N, c, epochs, pixels per epoch before the mask): N at the edges of the 128-row tiles
CASES = ((100, 2, 4, 30), (128, 2, 5, 30), (129, 2, 5, 30), (300, 1, 6, 60), (300, 2, 6, 60), (300, 3, 6, 60), (520, 2, 8, 75))


def case_id(case):
    return f"N{case[0]}-c{case[1]}"


@functools.lru_cache(maxsize=None)
def case_chunk(case):
    """A chunk of exactly N pixels: a seeded choice of N of the epochs x pixels, so the epochs have unequal sizes."""
    N, c, ne, npx = case
    full = syn.make_chunk(c, ne, npx, seed=7000 + N + c)
    keep = np.sort(np.random.default_rng(7100 + N + c).choice(ne * npx, size=N, replace=False))
    mask = np.zeros(ne * npx, dtype=bool)
    mask[keep] = True
    return syn.SyntheticChunk(c, ne, npx, np.ascontiguousarray(full.lwl[keep]), full.velocities,
                              np.ascontiguousarray(full.lwls[:, keep]), np.ascontiguousarray(full.fl[keep]),
                              np.ascontiguousarray(full.sigma[keep]), full.seed, mask.reshape(ne, npx), full.dates)


def case_gp(case):
    return np.array(syn.GP_BASE[case[1]], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def case_ext(case) -> Grad:
    ch = case_chunk(case)
    return grad_ext(ch.lwls, ch.fl, ch.sigma, case_gp(case), MU_GP)


def rel_to_scale(got, ref, scale):
    """max |got - ref| / S over the entries of one output"""
    got, ref, scale = (np.asarray(v, dtype=_LD) for v in (got, ref, scale))
    return float(np.max(np.abs(got - ref) / scale))


def measure_f64():
    """the float64 SciPy evaluation against the long-double one on CASES: per case the error relative to S of each output"""
    rows = []
    for case in CASES:
        ch, ref = case_chunk(case), case_ext(case)
        f = grad_f64(ch.lwls, ch.fl, ch.sigma, case_gp(case), MU_GP)
        rows.append((case_id(case), rel_to_scale(f.gp, ref.gp, ref.s_gp), rel_to_scale(f.mu, ref.mu, ref.s_mu),
                     rel_to_scale(f.lwl, ref.lwl, ref.s_lwl)))
    return rows


if __name__ == "__main__":
    rows = measure_f64()
    print(f"{'case':10s} {'grad_gp':>10s} {'grad_mu':>10s} {'grad_lwl':>10s}")
    for name, a, b, c_ in rows:
        print(f"{name:10s} {a:10.2e} {b:10.2e} {c_:10.2e}")
    print(f"{'max':10s} " + " ".join(f"{max(r[k] for r in rows):10.2e}" for k in (1, 2, 3)))
