"""CPU references for the Fisher information and the leave-one-out cross-validation of the continuum-marginalised likelihood
(tests/test_marg_fisher_reference.py, tests/test_gpu_marg_fisher.py).

    Kt = K + H Lambda H^T  (tests/marg_reference.py),   r = fl - mu_GP,   A = Kt^-1,   alpha_m = A r
    F_st = 1/2 tr(Kt^-1 K_s Kt^-1 K_t),   F_mu = 1^T Kt^-1 1            (K_t: tests/fisher_reference.py; H has no derivative)
    the pixel and epoch formulas of tests/loo_reference.py with this A and alpha_m; lnp the marginal likelihood

``fisher_ext`` and ``loo_ext`` build the dense Kt in np.longdouble with ``marg_reference.basis`` and invert it through the
oracle's long-double Cholesky: no Woodbury identity, so they share no route with the device.  ``fisher_f64`` and ``loo_f64``
are the device's route in float64 with SciPy:

    Wi = U^-T,  Wh = U^-T Ht,  M = I + Wh^T Wh = U_M^T U_M,  Vt = U_M^-T Wh^T Wi,  Kt^-1 = Wi^T Wi - Vt^T Vt,
    alpha_m = Wi^T (z - Wh M^-1 Wh^T z),  F_mu = |Wi 1|^2 - |Vt 1|^2

The cases are ``marg_reference.CASES`` with both ``WEIGHTS``; the tangents are built as ``fisher_reference.case_tangents``
builds them.  ``dropped=True`` evaluates the plain-K twin (the Vt loop left out) through the same code.

Run as a script it prints, per case, weight and output, the error of the float64 evaluation against the long-double one --
the table from which tests/test_gpu_marg_fisher.py takes its bounds -- and how far the marginal outputs lie from their plain
twins.
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
import loo_reference as lr  # noqa: E402
import marg_reference as mr  # noqa: E402
from loo_reference import _matrix_ext  # noqa: E402

_LD = np.longdouble
C_KMS = fr.C_KMS
MARGIN = 8                                   # the project's margin over the float64 table (tests/test_gpu_grad.py)
FISHER_OUTPUTS = ("F", "F_mu")
OUTPUTS = FISHER_OUTPUTS + lr.OUTPUTS + ("lnp",)

# The float64 table (python tests/marg_fisher_reference.py), its last row: the largest error of the float64 evaluation
# against the long-double one, per output.  tests/test_marg_fisher_reference.py checks that a fresh measurement does not
# exceed it; the device's tolerance is MARGIN times it.
F64_MAX = {
    "F": 1.10e-11, "F_mu": 1.14e-13, "pix_mean": 1.87e-12, "pix_var": 7.01e-11, "pix_logp": 3.57e-11, "loo_logp": 1.20e-13,
    "ep_resid": 1.91e-12, "ep_chi2": 2.17e-11, "ep_logp": 2.01e-12, "lnp": 7.30e-14,
}
TOL = {k: MARGIN * v for k, v in F64_MAX.items()}


# ---- the cases: marg_reference.CASES with tangents -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_tangents(case):
    """(tan_lwl (T, c, N), tan_gp (T, 2c)), T = 2c + 3, as ``fisher_reference.case_tangents``: the 2c hyper-parameter unit
    tangents; two velocity tangents, dx = -1/c_kms on the pixels of epoch 0 of the first component and of epoch n_epochs - 1
    of the last; one seeded random dx (normal, in units of 1 km/s)"""
    _, N, c, ne, _, _ = case
    ep = mr.case_chunk(case).epoch_index
    T = 2 * c + 3
    tan_lwl, tan_gp = np.zeros((T, c, N)), np.zeros((T, 2 * c))
    tan_gp[:2 * c] = np.eye(2 * c)
    assert np.any(ep == 0) and np.any(ep == ne - 1)
    tan_lwl[2 * c, 0, ep == 0] = -1.0 / C_KMS
    tan_lwl[2 * c + 1, c - 1, ep == ne - 1] = -1.0 / C_KMS
    tan_lwl[2 * c + 2] = np.random.default_rng(9700 + N + c).standard_normal((c, N)) / C_KMS
    tan_lwl.setflags(write=False)
    tan_gp.setflags(write=False)
    return tan_lwl, tan_gp


# ---- long double, on the dense Kt --------------------------------------------------------------------------------------------
def dense_ext(lwls, sigma, gp, x, epoch_index, n_epochs, order, sd, weight=None, dropped=False):
    """-> (C, L, Li): Kt = K + H Lambda H^T in long double (``dropped``: K alone), its lower Cholesky factor and L^-1"""
    import oracle
    lwls = np.atleast_2d(lwls)
    N = lwls.shape[1]
    C = _matrix_ext(lwls, sigma, gp)
    if not dropped:
        H = mr.basis(x, epoch_index, n_epochs, order, weight, T=_LD)
        lam = np.tile(np.asarray(sd, dtype=_LD) ** 2, n_epochs)
        C = C + (H * lam[None, :]) @ H.T
    C = _LD(0.5) * (C + C.T)
    L = oracle._chol_ext(C)
    return C, L, oracle._fsolve_ext(L, np.eye(N, dtype=_LD))


def fisher_ext(dense, lwls, gp, tan_lwl, tan_gp):
    """(F (T, T), F_mu) in long double from ``dense_ext``'s triple: X_t = Kt^-1 K_t, F_st = 1/2 sum_mn X_s[m,n] X_t[n,m]"""
    _, _, Li = dense
    N = Li.shape[0]
    G = Li.T @ Li
    X = [G @ fr.tangent_matrix(lwls, gp, dx, dgp, _LD) for dx, dgp in zip(tan_lwl, tan_gp)]
    T = len(X)
    F = np.zeros((T, T), dtype=_LD)
    for s in range(T):
        for t in range(s, T):
            F[s, t] = F[t, s] = _LD(0.5) * np.sum(X[s] * X[t].T)
    y = Li @ np.ones(N, dtype=_LD)
    return F, y @ y


def loo_ext(dense, fl, mu_GP, epoch_index, n_epochs) -> lr.Loo:
    """the leave-one-out outputs in long double from ``dense_ext``'s triple: the explicit inverse with one Newton step, as
    ``loo_reference.loo_ext`` makes it of K"""
    import oracle
    C, L, Li = dense
    N = C.shape[0]
    X = Li.T @ Li
    X = X + X @ (np.eye(N, dtype=_LD) - C @ X)
    A = _LD(0.5) * (X + X.T)
    r = np.asarray(fl, dtype=_LD) - _LD(mu_GP)
    z = Li @ r
    lnp = _LD(-0.5) * (z @ z + _LD(2) * np.sum(np.log(np.diag(L))))
    alpha = A @ r

    def solve_block(Aee, ae):
        Le = oracle._chol_ext(Aee)
        y = oracle._fsolve_ext(Le, ae)
        s = oracle._fsolve_ext(Le.T[::-1, ::-1], y[::-1])[::-1]
        return s, _LD(2) * np.sum(np.log(np.diag(Le)))

    return lr._finish(_LD, lnp, A, alpha, fl, epoch_index, n_epochs, solve_block)


# ---- float64, the device's route ---------------------------------------------------------------------------------------------
def woodbury_f64(lwls, fl, sigma, gp, x, epoch_index, n_epochs, order, sd, weight=None, mu_GP=1.0, dropped=False):
    """-> (K, Kt^-1, alpha_m, lnp, F_mu) by the device's formulas in float64 with SciPy; ``dropped``: without Vt (plain K)"""
    import oracle
    from scipy.linalg import cho_factor, solve_triangular
    lwls = np.ascontiguousarray(np.atleast_2d(lwls), dtype=np.float64)
    gp = np.asarray(gp, dtype=np.float64)
    N = lwls.shape[1]
    K = np.empty((N, N))
    oracle.fill_sym(K, lwls, gp)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=np.float64) ** 2
    U = np.triu(cho_factor(K, lower=False)[0])
    r = np.asarray(fl, dtype=np.float64) - mu_GP
    Wi = solve_triangular(U, np.eye(N), trans="T", lower=False)
    z = solve_triangular(U, r, trans="T", lower=False)
    y1 = Wi @ np.ones(N)
    ldK = 2 * np.sum(np.log(np.diag(U)))
    if dropped:
        return K, Wi.T @ Wi, Wi.T @ z, -0.5 * (z @ z + ldK), float(y1 @ y1)
    s = np.tile(np.asarray(sd, dtype=np.float64), n_epochs)
    Ht = mr.basis(x, epoch_index, n_epochs, order, weight) * s[None, :]
    Wh = solve_triangular(U, Ht, trans="T", lower=False)
    M = np.eye(Ht.shape[1]) + Wh.T @ Wh
    UM = np.triu(cho_factor(M, lower=False)[0])
    yv = solve_triangular(UM, Wh.T @ z, trans="T", lower=False)
    g = solve_triangular(UM, yv, lower=False)
    Vt = solve_triangular(UM, Wh.T @ Wi, trans="T", lower=False)
    Ainv = Wi.T @ Wi - Vt.T @ Vt
    alpha = Wi.T @ (z - Wh @ g)
    lnp = -0.5 * (((z @ z - yv @ yv) + ldK) + 2 * np.sum(np.log(np.diag(UM))))
    v1 = Vt @ np.ones(N)
    return K, Ainv, alpha, lnp, float(y1 @ y1 - v1 @ v1)


def fisher_f64(wood, lwls, gp, tan_lwl, tan_gp):
    """(F, F_mu) in float64 from ``woodbury_f64``'s tuple: G_t = 1/2 (A Z + Z^T A) with Z = K_t A, F_st = 1/2 sum K_s G_t"""
    _, A, _, _, F_mu = wood
    Kt = [fr.tangent_matrix(lwls, gp, dx, dgp) for dx, dgp in zip(tan_lwl, tan_gp)]
    G = []
    for k in Kt:
        Z = k @ A
        G.append(0.5 * (A @ Z + Z.T @ A))
    T = len(Kt)
    F = np.array([[0.5 * np.sum(Kt[s] * G[t]) for t in range(T)] for s in range(T)])
    return F, F_mu


def loo_f64(wood, fl, epoch_index, n_epochs) -> lr.Loo:
    from scipy.linalg import cho_factor, cho_solve
    _, A, alpha, lnp, _ = wood

    def solve_block(Aee, ae):
        f = cho_factor(Aee, lower=False)
        return cho_solve(f, ae), np.sum(2 * np.log(np.diag(f[0])))

    return lr._finish(np.float64, lnp, 0.5 * (A + A.T), alpha, fl, epoch_index, n_epochs, solve_block)


# ---- references of the cases ---------------------------------------------------------------------------------------------------
def _dense_args(case, kind):
    ch = mr.case_chunk(case)
    return (ch.lwls, ch.sigma, mr.case_gp(case), ch.x, ch.epoch_index, ch.n_epochs, ch.order, mr.prior_sd(ch.order),
            mr.case_weight(case, kind))


@functools.lru_cache(maxsize=None)
def case_ext(case, kind, dropped=False):
    """-> (F, F_mu, Loo) in long double; ``dropped``: the plain-K twins"""
    ch = mr.case_chunk(case)
    dense = dense_ext(*_dense_args(case, kind), dropped=dropped)
    F, F_mu = fisher_ext(dense, ch.lwls, mr.case_gp(case), *case_tangents(case))
    F.setflags(write=False)
    return F, F_mu, loo_ext(dense, ch.fl, mr.MU_GP, ch.epoch_index, ch.n_epochs)


def case_f64(case, kind, dropped=False):
    ch = mr.case_chunk(case)
    wood = woodbury_f64(*mr._case_args(case, kind), dropped=dropped)
    F, F_mu = fisher_f64(wood, ch.lwls, mr.case_gp(case), *case_tangents(case))
    return F, F_mu, loo_f64(wood, ch.fl, ch.epoch_index, ch.n_epochs)


def errors(got, ref) -> dict:
    """per output the error measures of tests/test_gpu_fisher.py (F relative to sqrt(F_ss F_tt), F_mu to itself) and of
    tests/test_gpu_loo.py (``loo_reference.errors``); lnp relative to max(1, |lnp|).  ``got``, ``ref``: (F, F_mu, loo)"""
    F, F_mu, loo = got
    F_ref, mu_ref, loo_ref = ref
    out = {"F": fr.rel_to_scale(F, F_ref), "F_mu": float(abs(_LD(F_mu) - mu_ref) / mu_ref)}
    out.update(lr.errors(loo, loo_ref))
    out["lnp"] = float(abs(_LD(loo.lnp) - loo_ref.lnp) / max(_LD(1), abs(loo_ref.lnp)))
    return out


def measure_f64():
    rows = []
    for case in mr.CASES:
        for kind in mr.WEIGHTS:
            rows.append((f"{mr.case_id(case)}-{kind}", errors(case_f64(case, kind), case_ext(case, kind))))
    return rows


def separation(case, kind) -> dict:
    """how far the long-double marginal F and pix_mean lie from their plain-K twins, in the error measures above"""
    e = errors(case_ext(case, kind, True), case_ext(case, kind))
    return {"F": e["F"], "pix_mean": e["pix_mean"]}


# ---- worker level: the SB2 N = 129 chunk of orbit_grad_reference.CHAIN_CASES[0] with a baseline ------------------------------
WORKER_BASELINE = {"order": 1, "sd": [0.05, 0.025], "weight": "one"}


def worker_fisher_ext(ch, lwls, p_orb, gp, keep, dropped=False):
    """The Fisher information of a worker in long double on the float64 grids ``lwls`` it uses: tangents
    dx_i = -J[c, epoch, i] / c_kms of the long-double Jacobian for the orbital parameters ``keep``, then the 2c unit tangents"""
    import orbit_grad_reference as ogr
    ep, ne = np.asarray(ch.epoch_index), len(ch.dates)
    c = lwls.shape[0]
    J, _ = ogr.jacobian_ext("SB2", p_orb, ch.dates)
    tan_lwl = [-np.moveaxis(J, 2, 0)[i][:, ep] / _LD(C_KMS) for i in keep] + [np.zeros((c, ch.N), dtype=_LD)] * (2 * c)
    tan_gp = np.zeros((len(keep) + 2 * c, 2 * c))
    tan_gp[len(keep):] = np.eye(2 * c)
    dense = dense_ext(lwls, ch.sigma, gp, ch.lwl, ep, ne, WORKER_BASELINE["order"], WORKER_BASELINE["sd"], None, dropped=dropped)
    return fisher_ext(dense, lwls, gp, tan_lwl, tan_gp)[0]


# ---- planted continuum offset: the same chunk, its flux a draw from its own GP plus a constant on one epoch -----------------
OFFSET_EPOCH = 2
OFFSET = 0.1                      # two standard deviations of the offset's prior (WORKER_BASELINE: 0.05)
OFFSET_SEED = 9800


@functools.lru_cache(maxsize=None)
def offset_case():
    """-> (chunk, p_orb, gp, lwls_ext): ``orbit_grad_reference.CHAIN_CASES[0]``'s chunk with fl replaced, as
    ``marg_reference.planted`` and ``loo_reference.planted`` replace it, by mu_GP + a draw from N(0, K) at the grids the
    long-double orbit gives (K with the noise on its diagonal), then OFFSET added to every pixel of epoch OFFSET_EPOCH"""
    import dataclasses
    import oracle
    import orbit_ext as oe
    import orbit_grad_reference as ogr
    case = ogr.CHAIN_CASES[0]
    ch, p_orb, gp = case.chunk, case.p_orb, case.gp
    ep = np.asarray(ch.epoch_index)
    lwls = oe.shift_ext(ch.lwl, oe.velocities_ext(case.model, p_orb, ch.dates), ep)
    L = oracle._chol_ext(_matrix_ext(lwls, ch.sigma, gp))
    draw = np.random.default_rng(OFFSET_SEED).standard_normal(ch.N)
    fl = np.asarray(_LD(mr.MU_GP) + L @ draw.astype(_LD), dtype=np.float64)
    fl[ep == OFFSET_EPOCH] += OFFSET
    return dataclasses.replace(ch, fl=np.ascontiguousarray(fl)), p_orb, gp, lwls


def offset_epoch_sf(dropped):
    """the upper-tail probabilities of every epoch's ep_chi2 (the rule of ``lnprob.loo_outliers``) on ``offset_case`` from the
    long-double reference on the grids of the long-double orbit, under WORKER_BASELINE or (``dropped``) under the plain K"""
    from scipy.stats import chi2
    ch, _, gp, lwls = offset_case()
    ep, ne = np.asarray(ch.epoch_index), len(ch.dates)
    dense = dense_ext(lwls, ch.sigma, gp, ch.lwl, ep, ne, WORKER_BASELINE["order"], WORKER_BASELINE["sd"], None, dropped=dropped)
    loo = loo_ext(dense, ch.fl, mr.MU_GP, ep, ne)
    return chi2.sf(np.asarray(loo.ep_chi2, dtype=np.float64), np.asarray(loo.ep_npix))


if __name__ == "__main__":
    rows = measure_f64()
    print(f"{'case':22s} " + " ".join(f"{k:>9s}" for k in OUTPUTS))
    for name, err in rows:
        print(f"{name:22s} " + " ".join(f"{err[k]:9.2e}" for k in OUTPUTS))
    print(f"{'max':22s} " + " ".join(f"{max(r[1][k] for r in rows):9.2e}" for k in OUTPUTS))
    print()
    print("marginal against plain K (long double), in the same measures, and in units of the device's tolerance")
    for case in mr.CASES:
        for kind in mr.WEIGHTS:
            sep = separation(case, kind)
            print(f"{mr.case_id(case)}-{kind:5s} F {sep['F']:.2e} ({sep['F'] / TOL['F']:.1e} x)   "
                  f"pix_mean {sep['pix_mean']:.2e} ({sep['pix_mean'] / TOL['pix_mean']:.1e} x)")
    print()
    print("planted offset: epoch_sf under the baseline ", np.array2string(offset_epoch_sf(False), precision=3))
    print("planted offset: epoch_sf under the plain K  ", np.array2string(offset_epoch_sf(True), precision=3))
