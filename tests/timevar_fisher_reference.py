"""CPU references for the Fisher information and the leave-one-out under the time-variable kernel
(tests/test_timevar_fisher_reference.py, tests/test_gpu_timevar_fisher.py), modelled on tests/fisher_reference.py and
tests/timevar_reference.py.

    K[m,n] = sum_c a_c^2 e + sigma_m^2 delta_mn,   e = exp(p_c d^2 + q_c dt^2),
    d = x_c[n] - x_c[m],  p_c = -1/2 c_kms^2 / l_c^2;   dt = t[n] - t[m],  q_c = -1/2 / tau_c^2

A tangent t is a direction (dx_t (c, N), da_tc, dl_tc, dtau_tc):

    K_t[m,n] = sum_c e (2 a_c da_tc + a_c^2 c_kms^2 / l_c^3 d^2 dl_tc + a_c^2 2 p_c d (dx_tc[n] - dx_tc[m])
                        + a_c^2 / tau_c^3 dt^2 dtau_tc)
    F_st     = 1/2 tr(K^-1 K_s K^-1 K_t)            F_mu = 1^T K^-1 1

``fisher_tv_ext`` in np.longdouble on ``timevar_reference.matrix_ext`` and the oracle's long-double Cholesky (P_t = L^-1 K_t
L^-T, F_st = 1/2 sum P_s P_t); ``fisher_tv_f64`` its float64 twin on ``timevar_reference.matrix_f64`` -- the device's argument
order, a = p * d * d, then a = a + q * dt * dt -- through ``fisher_reference.fisher_from_matrices``.  The twin takes a
``defect``: one of DEFECTS, a wrong formula planted in K_t or in the contraction, for the tests that show the bound rejects it.
The leave-one-out pair, ``loo_tv_ext`` and ``loo_tv_f64``, runs the closed forms of tests/loo_reference.py on the same two
matrices.

Run as a script it prints, per case, max_st |f64 - long double| / sqrt(F_ss F_tt) and |f64 - long double| / F_mu, and for the
leave-one-out the errors in the units of tests/test_gpu_loo.py: the tables from which tests/test_gpu_timevar_fisher.py takes
its bounds.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import fisher_reference as fr  # noqa: E402  (puts the oracle and the repository on the path)
import loo_reference as lr  # noqa: E402
import timevar_reference as tr  # noqa: E402

_LD = np.longdouble
C_KMS = fr.C_KMS
NB = 128
MU_GP = tr.MU_GP

# timevar_reference's cases without N = 520: one tile, exactly one tile, one tile plus one row, three tiles with a ragged edge,
# and the pixels of N = 300 in no time order with one tau = inf
CASES = tuple(case for case in tr.CASES if case[1][0] != 520)
case_id, case_data = tr.case_id, tr.case_data

DEFECTS = ("tau_squared",          # dt^2 / tau^2 in place of dt^2 / tau^3
           "wrong_component",      # the next component's tau in the temporal terms of K_t
           "static_e_tangent",     # no temporal factor in e of K_t
           "static_e_contract",    # no temporal factor in the contraction's e
           "q_without_half",       # q = -1 / tau^2
           "row_time_for_column")  # the contraction reads the column's time from the tile's row times


def _tile_row_times(t):
    """DT[m, n] of an epilogue that reads the time of column n from the ROW block of its tile (ti <= tj: the upper tiles, and
    their mirror images): t[128 ti + n - 128 tj] - t[m], 0 for an index past N"""
    N = t.shape[0]
    m, n = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    lo, hi = np.minimum(m, n), np.maximum(m, n)
    idx = NB * (lo // NB) + hi % NB
    tcol = np.where(idx < N, t[np.minimum(idx, N - 1)], 0.0)
    DT = tcol - t[lo]
    return np.where(m <= n, DT, -DT)


def tangent_matrix_tv(lwls, times, gp, tau, dx, dgp, dtau, T=np.float64, defect=None):
    """K_t (N, N) of one tangent (dx (c, N), dgp (2c,), dtau (c,)) in the number type ``T``; the argument of exp() in the
    device's order.  A component with tau = inf takes no time-scale term (its coefficient a^2 / tau^3 is 0)."""
    lwls = np.atleast_2d(lwls)
    c, N = lwls.shape
    ckms = T("2.99792458e5") if T is _LD else T(C_KMS)
    t = np.asarray(times, dtype=T)
    DT = t[None, :] - t[:, None]
    if defect == "row_time_for_column":
        DT = np.asarray(_tile_row_times(np.asarray(times, dtype=np.float64)), dtype=T)
    out = np.zeros((N, N), dtype=T)
    with np.errstate(under="ignore"):
        for k in range(c):
            a, l = T(gp[2 * k]), T(gp[2 * k + 1])
            tk = T(tau[(k + 1) % c] if defect == "wrong_component" else tau[k])
            da, dl, dtk = T(dgp[2 * k]), T(dgp[2 * k + 1]), T(dtau[k])
            x, u = np.asarray(lwls[k], dtype=T), np.asarray(dx[k], dtype=T)
            D = x[None, :] - x[:, None]
            p = T(-0.5) * ckms * ckms / (l * l)
            q = (T(-1.0) if defect == "q_without_half" else T(-0.5)) / (tk * tk)
            A = p * D * D
            if defect not in ("static_e_tangent", "static_e_contract"):
                A = A + q * DT * DT
            E = np.exp(A)
            ct = a * a / (tk * tk if defect == "tau_squared" else tk * tk * tk) * dtk
            out += E * (T(2) * a * da + a * a * (ckms * ckms) / (l * l * l) * (D * D) * dl
                        + a * a * T(2) * p * D * (u[None, :] - u[:, None]) + ct * (DT * DT))
    return out


def fisher_tv_ext(lwls, times, sigma, gp, tau, tan_lwl, tan_gp, tan_tau):
    """(F (T, T), F_mu) with every step in long double"""
    import oracle
    lwls = np.atleast_2d(np.asarray(lwls, dtype=np.float64))
    N = lwls.shape[1]
    K = tr.matrix_ext(lwls, times, gp, tau)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=_LD) ** 2
    L = oracle._chol_ext(K)
    Li = oracle._fsolve_ext(L, np.eye(N, dtype=_LD))          # L^-1
    P = [Li @ tangent_matrix_tv(lwls, times, gp, tau, dx, dgp, dtau, _LD) @ Li.T
         for dx, dgp, dtau in zip(tan_lwl, tan_gp, tan_tau)]
    T = len(P)
    F = np.zeros((T, T), dtype=_LD)
    for s in range(T):
        for t in range(s, T):
            F[s, t] = F[t, s] = _LD(0.5) * np.sum(P[s] * P[t])
    y = Li @ np.ones(N, dtype=_LD)
    return F, y @ y


# where each defect sits: in the K_t that is filled and multiplied by K^-1 from both sides, or in the derivative the product
# is contracted with
_IN_CONTRACTION = ("static_e_contract", "row_time_for_column")


def fisher_tv_f64(lwls, times, sigma, gp, tau, tan_lwl, tan_gp, tan_tau, defect=None):
    """the same in float64: ``timevar_reference.matrix_f64``, then ``fisher_reference.fisher_from_matrices``.  With a
    ``defect`` of the contraction, F_st = 1/2 sum K_s G_t takes its K_s from the defective formula and G_t from the sound one,
    as a device whose epilogue alone is wrong would."""
    assert defect is None or defect in DEFECTS
    lwls = np.ascontiguousarray(np.atleast_2d(lwls), dtype=np.float64)
    K = tr.matrix_f64(lwls, times, gp, tau, sigma)
    tans = list(zip(tan_lwl, tan_gp, tan_tau))
    fill_defect = None if defect in _IN_CONTRACTION else defect
    Kt = [tangent_matrix_tv(lwls, times, gp, tau, dx, dgp, dtau, defect=fill_defect) for dx, dgp, dtau in tans]
    F, F_mu = fr.fisher_from_matrices(K, Kt)
    if defect in _IN_CONTRACTION:
        from scipy.linalg import cho_factor, cho_solve
        Kinv = cho_solve(cho_factor(K, lower=False), np.eye(K.shape[0]))
        Ks = [tangent_matrix_tv(lwls, times, gp, tau, dx, dgp, dtau, defect=defect) for dx, dgp, dtau in tans]
        F = np.array([[0.5 * np.sum(ks * (Kinv @ kt @ Kinv)) for kt in Kt] for ks in Ks])
    return F, F_mu


# ---- the leave-one-out on a given K ------------------------------------------------------------------------------------
def loo_tv_ext(lwls, times, fl, sigma, gp, tau, mu_GP=1.0, epoch_index=None, n_epochs=None) -> lr.Loo:
    """``loo_reference.loo_ext`` on ``timevar_reference.matrix_ext``: every step in long double"""
    import oracle
    K = tr.matrix_ext(lwls, times, gp, tau)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=_LD) ** 2
    N = K.shape[0]
    L = oracle._chol_ext(K)
    Li = oracle._fsolve_ext(L, np.eye(N, dtype=_LD))
    X = Li.T @ Li
    X = X + X @ (np.eye(N, dtype=_LD) - K @ X)          # Newton: the residual of the inverse squared
    A = _LD(0.5) * (X + X.T)
    r = np.asarray(fl, dtype=_LD) - _LD(mu_GP)
    z = Li @ r
    lnp = _LD(-0.5) * (z @ z + _LD(2) * np.sum(np.log(np.diag(L))))

    def solve_block(Aee, ae):
        Le = oracle._chol_ext(Aee)
        y = oracle._fsolve_ext(Le, ae)
        s = oracle._fsolve_ext(Le.T[::-1, ::-1], y[::-1])[::-1]
        return s, _LD(2) * np.sum(np.log(np.diag(Le)))

    if epoch_index is not None and n_epochs is None:
        n_epochs = int(np.max(epoch_index)) + 1
    return lr._finish(_LD, lnp, A, A @ r, fl, epoch_index, n_epochs, solve_block)


def loo_tv_f64(lwls, times, fl, sigma, gp, tau, mu_GP=1.0, epoch_index=None, n_epochs=None) -> lr.Loo:
    """``loo_reference.loo_f64`` on ``timevar_reference.matrix_f64``"""
    from scipy.linalg import cho_factor, cho_solve
    K = tr.matrix_f64(lwls, times, gp, tau, sigma)
    N = K.shape[0]
    factor = cho_factor(K, lower=False)
    r = np.asarray(fl, dtype=np.float64) - mu_GP
    alpha = cho_solve(factor, r)
    A = cho_solve(factor, np.eye(N))
    lnp = -0.5 * (r @ alpha + np.sum(2 * np.log(np.diag(factor[0]))))

    def solve_block(Aee, ae):
        f = cho_factor(Aee, lower=False)
        return cho_solve(f, ae), np.sum(2 * np.log(np.diag(f[0])))

    if epoch_index is not None and n_epochs is None:
        n_epochs = int(np.max(epoch_index)) + 1
    return lr._finish(np.float64, lnp, A, alpha, fl, epoch_index, n_epochs, solve_block)


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _permutation(case):
    """the pixel order of ``timevar_reference.case_data`` (None: as generated)"""
    _name, shape, _mult, permuted = case
    return np.random.default_rng(7200 + shape[0] + shape[1]).permutation(shape[0]) if permuted else None


@functools.lru_cache(maxsize=None)
def case_tangents(case):
    """(tan_lwl (T, c, N), tan_gp (T, 2c), tan_tau (T, c)), T = 3c + 3: the 2c unit tangents of gp, the c of tau, the three
    grid tangents of ``fisher_reference.case_tangents`` (in the case's pixel order)"""
    _name, shape, _mult, _permuted = case
    N, c = shape[:2]
    g_lwl, g_gp = fr.case_tangents(shape)
    perm = _permutation(case)
    grid = g_lwl[2 * c:] if perm is None else g_lwl[2 * c:][:, :, perm]
    T = 3 * c + 3
    tan_lwl, tan_gp, tan_tau = np.zeros((T, c, N)), np.zeros((T, 2 * c)), np.zeros((T, c))
    tan_gp[:2 * c] = np.eye(2 * c)
    tan_tau[2 * c:3 * c] = np.eye(c)
    tan_lwl[3 * c:] = grid
    assert np.all(g_gp[2 * c:] == 0.0)
    for a in (tan_lwl, tan_gp, tan_tau):
        a.setflags(write=False)
    return tan_lwl, tan_gp, tan_tau


@functools.lru_cache(maxsize=None)
def case_epochs(case):
    """(epoch_index (N,), n_epochs) for the leave-one-out: the contiguous runs of the chunk as generated.  On the permuted
    case they are runs of positions in the permuted order -- groups of pixels from every date: the library asks for
    contiguous runs, not for runs of one date."""
    _name, shape, _mult, _permuted = case
    import grad_reference as gr
    ch = gr.case_chunk(shape)
    ep = np.ascontiguousarray(ch.epoch_index, dtype=np.int32)
    ep.setflags(write=False)
    return ep, int(shape[2])


@functools.lru_cache(maxsize=None)
def case_ext(case):
    d = case_data(case)
    F, F_mu = fisher_tv_ext(d.lwls, d.times, d.sigma, d.gp, d.tau, *case_tangents(case))
    F.setflags(write=False)
    return F, F_mu


@functools.lru_cache(maxsize=None)
def case_loo_ext(case) -> lr.Loo:
    d = case_data(case)
    ep, ne = case_epochs(case)
    return loo_tv_ext(d.lwls, d.times, d.fl, d.sigma, d.gp, d.tau, MU_GP, ep, ne)


def rel_to_scale(got, ref):
    """max_st |got - ref| / sqrt(ref_ss ref_tt) over the tangents with ref_ss > 0.  A tangent with ref_ss = 0 -- nothing but
    the time scale of a component with tau = inf -- has an exactly-zero row and column in the reference: ``got`` must be
    exactly zero there, or the result is inf."""
    got, ref = np.asarray(got, dtype=_LD), np.asarray(ref, dtype=_LD)
    d = np.sqrt(np.diag(ref))
    live = d > 0
    dead = ~live
    if np.any(got[dead, :] != 0) or np.any(got[:, dead] != 0) or np.any(ref[dead, :] != 0):
        return float("inf")
    return float(np.max(np.abs(got - ref)[np.ix_(live, live)] / np.outer(d[live], d[live])))


def measure_f64():
    rows = []
    for case in CASES:
        d = case_data(case)
        F, F_mu = case_ext(case)
        f, f_mu = fisher_tv_f64(d.lwls, d.times, d.sigma, d.gp, d.tau, *case_tangents(case))
        rows.append((case_id(case), rel_to_scale(f, F), float(abs(_LD(f_mu) - F_mu) / F_mu)))
    return rows


LOO_CASES = tuple(case for case in CASES if case_id(case) in ("N129-c2", "N300-c2-perm"))


def measure_loo_f64():
    rows = []
    for case in LOO_CASES:
        d = case_data(case)
        ep, ne = case_epochs(case)
        f = loo_tv_f64(d.lwls, d.times, d.fl, d.sigma, d.gp, d.tau, MU_GP, ep, ne)
        rows.append((case_id(case), lr.errors(f, case_loo_ext(case))))
    return rows


# ---- planted variability: N300-c2 with its flux redrawn from the time-variable K ---------------------------------------------
PLANT_SEED = 4
PLANT_TAU = 0.25          # of the span of the dates, on BOTH components: every line of the drawn spectrum drifts


@functools.lru_cache(maxsize=None)
def planted():
    """-> (case data of N300-c2 with fl = mu_GP + a draw from N(0, K_tv) (``synthetic.draw_timevar_flux``), tau (2,),
    epoch_index, n_epochs, the epoch farthest in time from the others)"""
    from psoap_amd import synthetic as syn
    import grad_reference as gr
    case = next(c for c in CASES if case_id(c) == "N300-c2")
    d = case_data(case)
    ep, ne = case_epochs(case)
    tau = np.full(2, PLANT_TAU * d.span)
    fl = syn.draw_timevar_flux(d.lwls, d.times, d.sigma, d.gp, tau, MU_GP, PLANT_SEED)
    dates = gr.case_chunk(case[1]).dates
    gap = [np.min(np.abs(np.delete(dates, e) - dates[e])) for e in range(ne)]
    return d, fl, tau, ep, ne, int(np.argmax(gap))


if __name__ == "__main__":
    rows = measure_f64()
    print(f"{'case':13s} {'F':>10s} {'F_mu':>10s}")
    for name, a, b in rows:
        print(f"{name:13s} {a:10.2e} {b:10.2e}")
    print(f"{'max':13s} " + " ".join(f"{max(r[k] for r in rows):10.2e}" for k in (1, 2)))
    print()
    rows = measure_loo_f64()
    print(f"{'case':13s} " + " ".join(f"{k:>10s}" for k in lr.OUTPUTS))
    for name, err in rows:
        print(f"{name:13s} " + " ".join(f"{err[k]:10.2e}" for k in lr.OUTPUTS))
    print(f"{'max':13s} " + " ".join(f"{max(r[1][k] for r in rows):10.2e}" for k in lr.OUTPUTS))
    print()
    d, fl, tau, ep, ne, far = planted()
    npix = np.bincount(ep, minlength=ne)
    tv = loo_tv_f64(d.lwls, d.times, fl, d.sigma, d.gp, tau, MU_GP, ep, ne)
    st = lr.loo_f64(d.lwls, fl, d.sigma, d.gp, MU_GP, ep, ne)
    print(f"planted variability, seed {PLANT_SEED}, epoch {far} ({npix[far]} pixels): chi2 / npix "
          f"{tv.ep_chi2[far] / npix[far]:.4f} under the time-variable K, {st.ep_chi2[far] / npix[far]:.4f} under the static K")
