"""CPU references for the gradient of the continuum-marginalised likelihood (tests/test_marg_grad_reference.py,
tests/test_gpu_marg_grad.py).

    lnL = -1/2 (r^T Kt^-1 r + log det Kt),  Kt = K + H Lambda H^T,  r = fl - mu_GP        (tests/marg_reference.py)

H does not depend on the hyper-parameters, the rest-frame grids or mu_GP, so with alpha_m = Kt^-1 r and
Q_m = alpha_m alpha_m^T - Kt^-1 the derivatives are the four formulas of tests/grad_reference.py with Q_m and alpha_m.

``marg_grad_ext`` builds the dense Kt in np.longdouble with ``marg_reference.basis``, inverts it through the oracle's
long-double Cholesky and contracts Q_m directly: no Woodbury identity, so it is independent of the device's route.
``marg_grad_f64`` is the device's route in float64 with SciPy:

    Wi = U^-T,  Wh = U^-T Ht,  z = U^-T r,  M = I + Wh^T Wh = U_M^T U_M,  y = U_M^-T Wh^T z
    Y = Wh U_M^-1,  V = Wi^T Y,  Kt^-1 = Wi^T Wi - V V^T,  alpha_m = Wi^T (z - Y y)

Both return, per output, the cancellation scale S = 1/2 sum_ij |Q_m,ij| |dK_ij/dtheta| (sum_i |alpha_m,i| for mu_GP) of
grad_reference.  ``chain_ext`` / ``chain_f64`` carry the gradient through the orbit as tests/orbit_grad_reference.py does, with
its scale S_orb.

Run as a script it prints, per case and weight, the error of ``marg_grad_f64`` against ``marg_grad_ext`` relative to the scale,
and the same for the orbit chain: the tables from which tests/test_gpu_marg_grad.py takes its bounds.
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
import marg_reference as mr  # noqa: E402
from loo_reference import _matrix_ext  # noqa: E402

_LD = np.longdouble
DEFECTS = ("VVt_dropped", "plain_alpha", "VVt_wrong_sign", "Y_without_UM")


def marg_grad_ext(lwls, fl, sigma, gp, x, epoch_index, n_epochs, order, sd, weight=None, mu_GP=1.0) -> gr.Grad:
    """every step in long double, on the dense K + H Lambda H^T and its explicit inverse"""
    import oracle
    lwls = np.atleast_2d(lwls)
    N = lwls.shape[1]
    K = _matrix_ext(lwls, sigma, gp)
    H = mr.basis(x, epoch_index, n_epochs, order, weight, T=_LD)
    lam = np.tile(np.asarray(sd, dtype=_LD) ** 2, n_epochs)
    C = K + (H * lam[None, :]) @ H.T
    C = _LD(0.5) * (C + C.T)
    L = oracle._chol_ext(C)
    Li = oracle._fsolve_ext(L, np.eye(N, dtype=_LD))
    r = np.asarray(fl, dtype=_LD) - _LD(mu_GP)
    zc = Li @ r
    alpha = Li.T @ zc
    Cinv = Li.T @ Li
    lnp = _LD(-0.5) * (zc @ zc + _LD(2) * np.sum(np.log(np.diag(L))))
    g_gp, g_x, g_mu, s_gp, s_x, s_mu = gr._contract(np.outer(alpha, alpha) - Cinv, lwls, gp, alpha, _LD)
    return gr.Grad(lnp, g_gp, g_x, g_mu, s_gp, s_x, s_mu)


def marg_grad_f64(lwls, fl, sigma, gp, x, epoch_index, n_epochs, order, sd, weight=None, mu_GP=1.0, defect=None) -> gr.Grad:
    """the Woodbury route in float64: the oracle's fill, SciPy's cho_factor and triangular solves.  ``defect``: one of DEFECTS,
    a wrong formula a test must be able to tell from the right one"""
    import oracle
    from scipy.linalg import cho_factor, solve_triangular
    assert defect is None or defect in DEFECTS
    lwls = np.ascontiguousarray(np.atleast_2d(lwls), dtype=np.float64)
    gp = np.asarray(gp, dtype=np.float64)
    N = lwls.shape[1]
    K = np.empty((N, N))
    oracle.fill_sym(K, lwls, gp)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=np.float64) ** 2
    U = cho_factor(K, lower=False)[0]
    U = np.triu(U)
    s = np.tile(np.asarray(sd, dtype=np.float64), n_epochs)
    Ht = mr.basis(x, epoch_index, n_epochs, order, weight) * s[None, :]
    r = np.asarray(fl, dtype=np.float64) - mu_GP
    Wi = solve_triangular(U, np.eye(N), trans="T", lower=False)
    Wh = solve_triangular(U, Ht, trans="T", lower=False)
    z = solve_triangular(U, r, trans="T", lower=False)
    M = np.eye(Ht.shape[1]) + Wh.T @ Wh
    UM = np.triu(cho_factor(M, lower=False)[0])
    y = solve_triangular(UM, Wh.T @ z, trans="T", lower=False)
    Y = Wh if defect == "Y_without_UM" else solve_triangular(UM, Wh.T, trans="T", lower=False).T
    V = Wi.T @ Y
    VVt = V @ V.T
    if defect == "VVt_dropped":
        VVt = np.zeros_like(VVt)
    elif defect == "VVt_wrong_sign":
        VVt = -VVt
    Cinv = Wi.T @ Wi - VVt
    alpha = Wi.T @ (z if defect == "plain_alpha" else z - Y @ y)
    lnp = -0.5 * (((z @ z - y @ y) + 2 * np.sum(np.log(np.diag(U)))) + 2 * np.sum(np.log(np.diag(UM))))
    g_gp, g_x, g_mu, s_gp, s_x, s_mu = gr._contract(np.outer(alpha, alpha) - Cinv, lwls, gp, alpha, np.float64)
    return gr.Grad(float(lnp), g_gp, g_x, float(g_mu), s_gp, s_x, float(s_mu))


# ---- references of the cases, and the float64 table ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_ext(case, kind) -> gr.Grad:
    return marg_grad_ext(*mr._case_args(case, kind))


def errors(got, ref: gr.Grad) -> dict:
    """per output max |got - ref| / S; ``got``: anything with gp, lwl, mu"""
    return {"grad_gp": gr.rel_to_scale(got.gp, ref.gp, ref.s_gp), "grad_mu": gr.rel_to_scale(got.mu, ref.mu, ref.s_mu),
            "grad_lwl": gr.rel_to_scale(got.lwl, ref.lwl, ref.s_lwl)}


OUTPUTS = ("grad_gp", "grad_mu", "grad_lwl")


def measure_f64(defect=None):
    rows = []
    for case in mr.CASES:
        for kind in mr.WEIGHTS:
            f = marg_grad_f64(*mr._case_args(case, kind), defect=defect)
            rows.append((f"{mr.case_id(case)}-{kind}", errors(f, case_ext(case, kind))))
    return rows


# ---- through the orbit: the SB2 chunk of marg_reference.orbit_case ------------------------------------------------------------
def _orbit_args():
    ch, p_orb, gp, _, _ = mr.orbit_case()
    return ch, np.asarray(p_orb, dtype=np.float64), np.asarray(gp, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def chain_ext():
    """-> (Grad on the grids of the long-double orbit, grad_orb (n_orb,), S_orb): orbit_grad_reference.chain_from with the
    marginal gradient in the middle"""
    import orbit_ext as oe
    import orbit_grad_reference as og
    ch, p_orb, gp = _orbit_args()
    ne = len(ch.dates)
    vel = oe.velocities_ext("SB2", p_orb, ch.dates)
    g = marg_grad_ext(oe.shift_ext(ch.lwl, vel, ch.epoch_index), ch.fl, ch.sigma, gp, ch.lwl, ch.epoch_index, ne, 1, mr.PLANT_SD, None,
                      mr.MU_GP)
    ckms = _LD(oe.C_KMS)
    g_v, s_v = -og.fold(g.lwl, ch.epoch_index, ne) / ckms, og.fold(g.s_lwl, ch.epoch_index, ne) / ckms
    J, _ = og.jacobian_ext("SB2", p_orb, ch.dates)
    return g, np.einsum("ce,cek->k", g_v, J), np.einsum("ce,cek->k", s_v, np.abs(J))


def chain_f64():
    """the float64 host composition: restated device velocities, host shift, marg_grad_f64, velocity_gradient, jacobian_f64"""
    import orbit_cases as oc
    import orbit_ext as oe
    import orbit_grad_reference as og
    from psoap_amd import covariance
    ch, p_orb, gp = _orbit_args()
    ne = len(ch.dates)
    vel = oc.kernel_restated("SB2", p_orb, ch.dates)
    lwls = ch.lwl + (-vel[:, ch.epoch_index]) / oe.C_KMS
    g = marg_grad_f64(lwls, ch.fl, ch.sigma, gp, ch.lwl, ch.epoch_index, ne, 1, mr.PLANT_SD, None, mr.MU_GP)
    g_v = covariance.velocity_gradient(g.lwl, ch.epoch_index, ne)
    J, _ = og.jacobian_f64("SB2", p_orb, ch.dates)
    return np.einsum("ce,cek->k", g_v, J), g


def measure_orbit():
    ref, orb, s_orb = chain_ext()
    got_orb, g = chain_f64()
    return {"grad_orb": gr.rel_to_scale(got_orb, orb, s_orb), "grad_gp": gr.rel_to_scale(g.gp, ref.gp, ref.s_gp),
            "grad_mu": gr.rel_to_scale(g.mu, ref.mu, ref.s_mu)}


if __name__ == "__main__":
    rows = measure_f64()
    print(f"{'case':22s} " + " ".join(f"{k:>10s}" for k in OUTPUTS))
    for name, err in rows:
        print(f"{name:22s} " + " ".join(f"{err[k]:10.2e}" for k in OUTPUTS))
    print(f"{'max':22s} " + " ".join(f"{max(r[1][k] for r in rows):10.2e}" for k in OUTPUTS))
    err = measure_orbit()
    print()
    print(f"{'SB2-N240 orbit chain':22s} " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    print()
    print("seeded defects: the smallest, over the cases, of the largest error / scale over the outputs")
    for d in DEFECTS:
        print(f"{d:16s} {min(max(e.values()) for _, e in measure_f64(d)):10.2e}")
