"""CPU references for the observed information of the epoch velocities (tests/test_vel_newton_reference.py,
tests/test_gpu_vel_newton.py; psoap_amd/csrc/vel_newton_kernels.hpp).

With G = Kt^-1 (Kt = K, or K + H Lambda H^T under a baseline), alpha = G r, C = G - alpha alpha^T and, for the velocity
s = (k, e), K_s = dK/ds, K_st = d2K/ds dt,

    g_s  = dlnL/ds = 1/2 alpha^T K_s alpha - 1/2 tr(G K_s)
    J_st = -d2 lnL / ds dt = -F_st + u_s^T G u_t + 1/2 sum_mn K_st[m, n] C[m, n],      u_s = K_s alpha,  F_st = 1/2 tr(G K_s G K_t).

``info_ext`` is that in long double, generically: the grids are x_k[i] = lwl[i] - v[k, epoch(i)] / c_kms, so the tangent of
s moves x_k by dx_s[i] = -[epoch(i) = e] / c_kms, and with d = x_k[n] - x_k[m], kappa(d) = a_k^2 exp(p_k d^2), element by
element,

    K_s[m, n]  = kappa'(d)  (dx_s[n] - dx_s[m])
    K_st[m, n] = kappa''(d) (dx_s[n] - dx_s[m]) (dx_t[n] - dx_t[m])      (same component; zero otherwise: the grids are linear in v)

with kappa' = 2 p d kappa, kappa'' = (2 p + 4 p^2 d^2) kappa.  Nothing of the structured form enters.  It is itself pinned by
central differences of the long-double gradient of grad_reference.grad_ext (baseline: marg_grad_reference.marg_grad_ext),
folded onto the velocities; ``fd_step`` derives the step and the bound.

``info_f64`` is the float64 twin of the device's structured form (U, B, T; vel_newton_kernels.hpp) with SciPy, and takes the
seeded defects.  ``cpu_newton`` runs psoap_amd.lnprob.velocity_newton on it: the CPU twin of epoch_velocities(method="newton").

Run as a script it prints the finite-difference pin, the float64 table from which tests/test_gpu_vel_newton.py takes its
bounds, and the per-seed table of the two fits.
"""
from __future__ import annotations

import dataclasses
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
import marg_fisher_reference as mfr  # noqa: E402
import marg_grad_reference as mgr  # noqa: E402
import marg_reference as mr  # noqa: E402
import vel_fisher_reference as vr  # noqa: E402

_LD = np.longdouble
C_KMS = fr.C_KMS
MU_GP = gr.MU_GP
OUTPUTS = ("lnp", "grad", "F", "J")
# Seeded defects of the structured form, each of which must leave the bound
DEFECTS = ("T_dropped", "T_offdiag_sign", "plus_F", "aat_dropped", "UGU_halved", "Y_sign")
# Keeping the within-epoch block of W_k is NO defect: T_k = diag(rowsum(B_k)) - B_k takes B_k[e, e] in and out again, as the
# within-epoch block of Dv_k cancelled in F (vel_fisher_reference.NOT_A_DEFECT).
NOT_A_DEFECT = "within_epoch_kept"
BASELINES = (None, 0, 2)                     # plain, and a baseline of order 0 and 2 (marg_reference.prior_sd)


@dataclasses.dataclass(frozen=True)
class Shape:
    """a chunk of the GPU test with its epoch index: gr.case_chunk(case), then its pixels permuted (``perm_seed``) or its whole
    epochs put in the order ``block_order`` (every epoch stays contiguous), and its epochs renumbered through ``relabel``
    (n_epochs grows to max + 1: unused ids are empty epochs)"""
    name: str
    case: tuple
    perm_seed: int | None = None
    relabel: tuple | None = None
    block_order: tuple | None = None


SHAPES = tuple(Shape(fr.case_id(case), case) for case in fr.CASES) + (
    Shape("cE33", vr.CASE_33), Shape("cE36", vr.CASE_36),
    Shape("N300-empty", fr.CASES[4], relabel=(0, 2, 3, 4, 5, 6)),          # unequal epochs (the mask's), epoch 1 of 7 empty
    Shape("N300-perm", fr.CASES[4], perm_seed=8300),                       # pixels in no epoch order
    # whole epochs of unequal length, contiguous but not in id order and across tile edges: a tile's column slots (ascending
    # epoch id) are not in column order, and a baseline can be set
    Shape("N300-blocks", fr.CASES[4], block_order=(3, 0, 5, 2, 4, 1)),
)


@dataclasses.dataclass(frozen=True)
class Problem:
    lwl: np.ndarray
    lwls: np.ndarray
    fl: np.ndarray
    sigma: np.ndarray
    gp: np.ndarray
    ep: np.ndarray
    E: int
    c: int


@functools.lru_cache(maxsize=None)
def problem(shape: Shape) -> Problem:
    ch, gp = gr.case_chunk(shape.case), gr.case_gp(shape.case)
    ep, E = np.asarray(ch.epoch_index), shape.case[2]
    idx = np.arange(ch.N) if shape.perm_seed is None else np.random.default_rng(shape.perm_seed).permutation(ch.N)
    if shape.block_order is not None:
        idx = np.concatenate([np.flatnonzero(ep == e) for e in shape.block_order])
    if shape.relabel is not None:
        ep, E = np.asarray(shape.relabel)[ep], max(shape.relabel) + 1
    c = lambda a: np.ascontiguousarray(a)      # noqa: E731
    return Problem(c(ch.lwl[idx]), c(ch.lwls[:, idx]), c(ch.fl[idx]), c(ch.sigma[idx]), gp, c(ep[idx]), E, shape.case[1])


def baseline_args(pr: Problem, order):
    """(x, epoch_index, n_epochs, order, sd, weight) as marg_reference takes them: the worker's choice x = lwl, weight one"""
    return pr.lwl, pr.ep, pr.E, order, mr.prior_sd(order), None


# ---- long double, generic -------------------------------------------------------------------------------------------------
def _sparse_left(G, M):
    """G @ M for an M whose rows are mostly zero outside a few columns: the product over the non-zero rows and columns only
    (the terms left out are exact zeros)"""
    rows = np.flatnonzero(np.any(M != 0, axis=1))
    dense = rows[np.count_nonzero(M[rows], axis=1) > M.shape[1] // 2] if rows.size else rows
    out = np.zeros_like(G)
    if dense.size:
        out += G[:, dense] @ M[dense, :]
    rest = np.setdiff1d(rows, dense)
    if rest.size:
        cols = np.flatnonzero(np.any(M[rest] != 0, axis=0))
        out[:, cols] += G[:, rest] @ M[np.ix_(rest, cols)]
    return out


def info_ext(lwls, fl, sigma, gp, ep, E, mu_GP=MU_GP, order=None, x=None):
    """-> (lnp, g (c E), F, J) in long double, generically (module docstring); ``order``: under the baseline of that order"""
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    c, N = lwls.shape
    ep = np.asarray(ep)
    sd = mr.prior_sd(0 if order is None else order)
    Kt, L, Li = mfr.dense_ext(lwls, sigma, gp, x, ep, E, 0 if order is None else order, sd, None, dropped=order is None)
    G = Li.T @ Li
    r = np.asarray(fl, dtype=_LD) - _LD(mu_GP)
    z = Li @ r
    alpha = Li.T @ z
    lnp = _LD(-0.5) * (z @ z + _LD(2) * np.sum(np.log(np.diag(L))))
    C = G - np.outer(alpha, alpha)
    ckms = _LD("2.99792458e5")
    T = c * E
    dx = np.zeros((E, N), dtype=_LD)                   # the tangent of the grid of a component for the velocity at epoch e
    for e in range(E):
        dx[e, ep == e] = _LD(-1) / ckms
    dd = dx[:, None, :] - dx[:, :, None]               # (E, m, n): dx_s[n] - dx_s[m]
    g = np.zeros(T, dtype=_LD)
    X, Uc = [], np.zeros((N, T), dtype=_LD)
    Tm = np.zeros((T, T), dtype=_LD)
    for k in range(c):
        a, l = _LD(gp[2 * k]), _LD(gp[2 * k + 1])
        xk = np.asarray(lwls[k], dtype=_LD)
        d = xk[None, :] - xk[:, None]
        p = _LD(-0.5) * ckms * ckms / (l * l)
        kap = a * a * np.exp(p * d * d)
        k1 = _LD(2) * p * d * kap
        k2 = (_LD(2) * p + _LD(4) * p * p * d * d) * kap
        for e in range(E):
            s = k * E + e
            Ks = k1 * dd[e]
            X.append(_sparse_left(G, Ks))
            Uc[:, s] = Ks @ alpha
            g[s] = _LD(-0.5) * np.sum(Ks * C)
            for f in range(e + 1):
                Tm[s, k * E + f] = Tm[k * E + f, s] = _LD(0.5) * np.sum(k2 * dd[e] * dd[f] * C)
    F = np.zeros((T, T), dtype=_LD)
    for s in range(T):
        for t in range(s, T):
            F[s, t] = F[t, s] = _LD(0.5) * np.sum(X[s] * X[t].T)
    J = -F + Uc.T @ G @ Uc + Tm
    return lnp, g, F, J


@functools.lru_cache(maxsize=None)
def shape_ext(shape: Shape, order=None):
    pr = problem(shape)
    out = info_ext(pr.lwls, pr.fl, pr.sigma, pr.gp, pr.ep, pr.E, MU_GP, order, pr.lwl)
    for a in out[1:]:
        a.setflags(write=False)
    return out


# ---- the pin of the long-double J: central differences of the long-double gradient ---------------------------------------
def grad_vel_ext(pr: Problem, vel, order=None, mu_GP=MU_GP):
    """dlnL/dv (c E) in long double at the table ``vel`` (c, E) of offsets from the problem's grids: grad_reference.grad_ext
    (marg_grad_reference.marg_grad_ext), folded -- code that shares nothing with info_ext but the fill"""
    lw = pr.lwls + (-np.asarray(vel, dtype=np.float64)[:, pr.ep]) / C_KMS
    if order is None:
        gx = gr.grad_ext(lw, pr.fl, pr.sigma, pr.gp, mu_GP).lwl
    else:
        gx = mgr.marg_grad_ext(lw, pr.fl, pr.sigma, pr.gp, *baseline_args(pr, order), mu_GP=mu_GP).lwl
    out = np.zeros((pr.c, pr.E), dtype=_LD)
    for e in range(pr.E):
        out[:, e] = -np.sum(np.asarray(gx, dtype=_LD)[:, pr.ep == e], axis=1) / _LD(C_KMS)
    return out.reshape(-1)


def fd_step(gp):
    """The step h (km/s) and the bound on |J_fd - J| / sqrt(F_ss F_tt) of a central difference of the gradient.  The velocity
    enters through d / l_k only, so with h' = h / min l the truncation error is h'^2 / 6 times a third derivative of O(10) in
    those units: 2 h'^2.  The grids are float64 numbers: lwl - (v +- h) / c_kms is rounded to 2^-53 |lwl| ~ 1e-15, i.e.
    1e-15 c_kms / min l = 3e-10 / min l of the step's own unit -- a relative perturbation 3e-10 / (min l  h') of the
    difference, far above long double's own rounding.  h' = 1e-3 balances the two within a factor of a few (2e-6 against
    3e-7 / min l with l of a few km/s); the bound is their sum times 4."""
    lmin = float(min(gp[1::2]))
    hp = 1e-3
    return hp * lmin, 4.0 * (2.0 * hp * hp + 3e-10 / (lmin * hp))


def fd_pin(shape: Shape, order=None):
    """-> (max |J_fd - J| / sqrt(F_ss F_tt), bound, h)"""
    pr = problem(shape)
    h, bound = fd_step(pr.gp)
    _, _, F, J = shape_ext(shape, order)
    T = pr.c * pr.E
    Jfd = np.zeros((T, T), dtype=_LD)
    for t in range(T):
        v = np.zeros(T)
        v[t] = h
        gp_, gm_ = grad_vel_ext(pr, v.reshape(pr.c, pr.E), order), grad_vel_ext(pr, -v.reshape(pr.c, pr.E), order)
        Jfd[:, t] = -(gp_ - gm_) / (_LD(2) * _LD(h))
    return rel_to_scale(Jfd, J, F), bound, h


def rel_to_scale(got, ref, F):
    """max |got - ref| / sqrt(F_ss F_tt) for a (c E, c E) matrix, / sqrt(F_ss) for a gradient; rows of empty epochs (F_ss = 0)
    count with scale 1: they must be exact zeros"""
    d = np.sqrt(np.abs(np.diag(np.asarray(F, dtype=_LD))))
    d[d == 0] = 1
    got, ref = np.asarray(got, dtype=_LD), np.asarray(ref, dtype=_LD)
    if got.ndim == 2 and got.shape[0] == got.shape[1] == d.size:
        return float(np.max(np.abs(got - ref) / np.outer(d, d)))
    return float(np.max(np.abs(got.reshape(-1) - ref.reshape(-1)) / d))


# ---- float64, the device's structured form ------------------------------------------------------------------------------------
def w_matrices(lwls, gp, ep, defect=None):
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    ep = np.asarray(ep)
    cross = ep[:, None] != ep[None, :]
    out = []
    for k in range(lwls.shape[0]):
        a, l = float(gp[2 * k]), float(gp[2 * k + 1])
        p = -0.5 * C_KMS * C_KMS / (l * l)
        D = lwls[k][None, :] - lwls[k][:, None]
        W = a * a * (2.0 * p + 4.0 * p * p * D * D) * np.exp(p * D * D) / (C_KMS * C_KMS)
        out.append(W if defect == NOT_A_DEFECT else W * cross)
    return out


def info_from_inverse(G, alpha, lwls, gp, ep, E, defect=None):
    """(g (c E), F, J, parts) by the structured form from G and alpha; parts = (U, [B_k], [T_k])"""
    lwls = np.atleast_2d(lwls)
    c, N = lwls.shape
    ep = np.asarray(ep)
    Dv = vr.dv_matrices(lwls, gp, ep)
    Wk = w_matrices(lwls, gp, ep, defect)
    F = vr.vel_fisher_from_inverse(G, Dv, ep, E)
    P = np.zeros((N, E))
    P[np.arange(N), ep] = 1.0
    C = G if defect == "aat_dropped" else G - np.outer(alpha, alpha)
    U, g = np.zeros((N, c * E)), np.zeros(c * E)
    Tm = np.zeros((c * E, c * E))
    Bs, Ts = [], []
    for k in range(c):
        Y = (Dv[k] * alpha[None, :]) @ P
        q = Y.sum(axis=1)
        U[:, k * E:(k + 1) * E] = P * q[:, None] + Y if defect == "Y_sign" else P * q[:, None] - Y
        g[k * E:(k + 1) * E] = -(P.T @ (Dv[k] * C) @ P).sum(axis=1)
        B = P.T @ (Wk[k] * C) @ P
        Tk = np.diag(B.sum(axis=1)) + B - 2.0 * np.diag(np.diag(B)) if defect == "T_offdiag_sign" else np.diag(B.sum(axis=1)) - B
        if defect == "T_dropped":
            Tk = np.zeros_like(Tk)
        Tm[k * E:(k + 1) * E, k * E:(k + 1) * E] = Tk
        Bs.append(B)
        Ts.append(Tk)
    UGU = U.T @ (G @ U)
    if defect == "UGU_halved":
        UGU = 0.5 * UGU
    J = (F if defect == "plus_F" else -F) + UGU + Tm
    return g, F, 0.5 * (J + J.T), (U, Bs, Ts)


def info_f64(lwls, fl, sigma, gp, ep, E, mu_GP=MU_GP, order=None, x=None, defect=None):
    """-> (lnp, g (c E), F, J) in float64 by the device's route: marg_fisher_reference.woodbury_f64 for Kt^-1, alpha (alpha_m)
    and the value, then the structured form"""
    sd = mr.prior_sd(0 if order is None else order)
    _, G, alpha, lnp, _ = mfr.woodbury_f64(lwls, fl, sigma, gp, x, ep, E, 0 if order is None else order, sd, None, mu_GP,
                                           dropped=order is None)
    g, F, J, _ = info_from_inverse(0.5 * (G + G.T), alpha, lwls, gp, ep, E, defect)
    return float(lnp), g, F, J


def shape_f64(shape: Shape, order=None, defect=None):
    pr = problem(shape)
    return info_f64(pr.lwls, pr.fl, pr.sigma, pr.gp, pr.ep, pr.E, MU_GP, order, pr.lwl, defect)


def errors(got, ref) -> dict:
    """lnp: |got - ref| / max(1, |ref|); grad / sqrt(F_ss); F and J / sqrt(F_ss F_tt), F the reference's"""
    Fr = ref[2]
    return {"lnp": float(abs(_LD(got[0]) - ref[0]) / max(_LD(1), abs(ref[0]))), "grad": rel_to_scale(got[1], ref[1], Fr),
            "F": rel_to_scale(got[2], Fr, Fr), "J": rel_to_scale(got[3], ref[3], Fr)}


def measure_f64(shapes=SHAPES, orders=BASELINES):
    return [(f"{sh.name}-{'plain' if o is None else 'b%d' % o}", errors(shape_f64(sh, o), shape_ext(sh, o)))
            for sh in shapes for o in orders]


# The float64 table (python tests/vel_newton_reference.py), its last row: the largest error of the float64 twin against the
# long-double reference over SHAPES x BASELINES.  tests/test_gpu_vel_newton.py bounds the device by MARGIN times these.
MARGIN = 8
F64_MAX = {"lnp": 6.54e-14, "grad": 5.22e-12, "F": 2.37e-12, "J": 6.31e-13}      # (the order-2 baselines set every one of them)
F64_MAX_AT = {"lnp": ("N128-c2", 2), "grad": ("N129-c2", 2), "F": ("N100-c2", 2), "J": ("N100-c2", 2)}      # (shape, order) of each maximum
TOL = {k: MARGIN * v for k, v in F64_MAX.items()}


# ---- the fit ----------------------------------------------------------------------------------------------------------------
FIT_SEEDS = tuple(range(7903, 7925))
FIT_BASELINE = {"order": 0, "sd": [0.05]}
OFFSET_SEED = 8400


@functools.lru_cache(maxsize=None)
def fit_chunk(seed=vr.FIT_SEED):
    """vel_fisher_reference.fit_chunk's recipe at any seed (seed = FIT_SEED: that very chunk)"""
    import oracle
    from psoap_amd import synthetic as syn
    ch = syn.make_chunk(2, 6, 50, seed=seed)
    K = np.empty((ch.N, ch.N))
    oracle.fill_sym(K, np.ascontiguousarray(ch.lwls), vr.fit_gp())
    K[np.diag_indices_from(K)] += ch.sigma ** 2
    fl = vr.FIT_MU + np.linalg.cholesky(K) @ np.random.default_rng(seed + 50).standard_normal(ch.N)
    return dataclasses.replace(ch, fl=np.ascontiguousarray(fl))


def offset_flux(ch):
    """the chunk's flux plus one continuum offset per epoch, drawn from FIT_BASELINE's prior N(0, 0.05^2) (seeded)"""
    off = FIT_BASELINE["sd"][0] * np.random.default_rng(OFFSET_SEED).standard_normal(ch.n_epochs)
    return np.ascontiguousarray(ch.fl + off[ch.epoch_index]), off


def cpu_newton(ch, gp, vel0, fl=None, order=None, mu_GP=vr.FIT_MU, max_iter=20, tol=1e-10, sd=None):
    """psoap_amd.lnprob.velocity_newton -- the loop of epoch_velocities(method="newton") -- on info_f64"""
    from psoap_amd.lnprob import velocity_newton
    ep, E = ch.epoch_index, ch.n_epochs
    fl = ch.fl if fl is None else fl
    sd = mr.prior_sd(0 if order is None else order) if sd is None else np.asarray(sd, dtype=np.float64)

    def wood(vel):
        lw = ch.lwl[None, :] + (-vel[:, ep]) / C_KMS
        return lw, mfr.woodbury_f64(lw, fl, ch.sigma, gp, ch.lwl, ep, E, 0 if order is None else order, sd, None, mu_GP,
                                    dropped=order is None)

    def value(vel):
        return float(wood(vel)[1][3])

    def info(vel):
        lw, (_, G, alpha, lnp, _) = wood(vel)
        g, F, J, _ = info_from_inverse(0.5 * (G + G.T), alpha, lw, gp, ep, E)
        return float(lnp), g.reshape(ch.n_components, E), F, J

    return velocity_newton(value, info, vel0, np.bincount(ep, minlength=E) > 0, max_iter, tol)


@functools.lru_cache(maxsize=None)
def seed_table():
    """per seed of FIT_SEEDS, from the chunk's true velocities: (seed, scoring n_iter, converged, newton n_iter, converged,
    n_fallback)"""
    rows = []
    for seed in FIT_SEEDS:
        ch = fit_chunk(seed)
        sc = vr.cpu_fit(ch, vr.fit_gp(), ch.velocities)
        nw = cpu_newton(ch, vr.fit_gp(), ch.velocities)
        rows.append((seed, sc["n_iter"], bool(sc["converged"]), nw["n_iter"], bool(nw["converged"]), nw["n_fallback"]))
    return tuple(rows)


# the seed of the second fit case: the first of FIT_SEEDS that scoring misses in 20 iterations and Newton converges on
# (seed_table(); tests/test_vel_newton_reference.py pins it)
HARD_SEED = 7903


if __name__ == "__main__":
    for sh, o in ((SHAPES[0], None), (SHAPES[0], 0), (SHAPES[0], 2)):
        err, bound, h = fd_pin(sh, o)
        print(f"fd pin {sh.name} order {o}: h = {h:.3e} km/s, |J_fd - J| = {err:.2e} (bound {bound:.2e})")
    rows = measure_f64()
    print(f"{'shape':18s} " + " ".join(f"{k:>10s}" for k in OUTPUTS))
    for name, e in rows:
        print(f"{name:18s} " + " ".join(f"{e[k]:10.2e}" for k in OUTPUTS))
    print(f"{'max':18s} " + " ".join(f"{max(r[1][k] for r in rows):10.2e}" for k in OUTPUTS))
    print("seed  scoring (iter, conv)  newton (iter, conv, fallbacks)")
    for row in seed_table():
        print("%d  %2d %-5s  %2d %-5s %d" % row)
