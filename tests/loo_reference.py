"""CPU references for leave-one-out cross-validation of the GP likelihood (tests/test_loo_reference.py, tests/test_gpu_loo.py).

    r = fl - mu_GP,  A = K^-1,  alpha = A r,  K as the likelihood builds it (noise on the diagonal)

    pixel i          pix_mean = fl[i] - alpha[i] / A[i][i],  pix_var = 1 / A[i][i],
                     pix_logp = 1/2 log A[i][i] - alpha[i]^2 / (2 A[i][i]) - 1/2 log(2 pi)
    epoch e (I_e)    s_e = A[I_e,I_e]^-1 alpha[I_e] -> ep_resid,  ep_chi2 = alpha[I_e] . s_e,
                     ep_logp = -1/2 ep_chi2 + 1/2 log det A[I_e,I_e] - n_e/2 log(2 pi);  an epoch without pixels 0.0, 0.0, 0
    loo_logp = sum_i pix_logp[i]

Three evaluations: ``loo_ext`` in np.longdouble from an explicit inverse (the oracle's long-double Cholesky, L^-T L^-1, one
Newton step X <- X + X (I - K X), symmetrised), ``loo_f64`` in float64 with SciPy's ``cho_factor`` / ``cho_solve``, and the
brute-force route (``delete_pixel``, ``delete_epoch``) that really deletes a pixel or an epoch and conditions on the rest.

Run as a script it prints, per case and output, the error of the float64 evaluation against the long-double one: the table
from which tests/test_gpu_loo.py takes its bounds.
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

from psoap_amd import synthetic as syn  # noqa: E402

_LD = np.longdouble
MU_GP = 0.9
SIGMA = 0.02
_HALF_LOG_2PI = _LD(0.5) * np.log(_LD(8) * np.arctan(_LD(1)))

OUTPUTS = ("pix_mean", "pix_var", "pix_logp", "loo_logp", "ep_resid", "ep_chi2", "ep_logp")


@dataclass
class Loo:
    lnp: object
    loo_logp: object
    pix_mean: np.ndarray
    pix_var: np.ndarray
    pix_logp: np.ndarray
    pix_z: np.ndarray
    ep_resid: np.ndarray = None
    ep_chi2: np.ndarray = None
    ep_logp: np.ndarray = None
    ep_npix: np.ndarray = None


# ---- the cases -------------------------------------------------------------------------------------------------------
# (name, N, c, n_epochs, runs): runs = ((epoch id, pixels), ...) in flattened order.  The smallest shapes at which the band
# kernel, the scatter or the block batch can go wrong:
CASES = (
    ("a", 100, 2, 4, ((0, 25), (1, 25), (2, 25), (3, 25))),            # one tile, all blocks inside it
    ("b", 128, 1, 1, ((0, 128),)),                                     # one epoch = one full tile, no padding
    ("c", 129, 2, 2, ((0, 128), (1, 1))),                              # second tile row holds one pixel; a one-pixel epoch
    ("d", 384, 1, 3, ((0, 128), (1, 128), (2, 128))),                  # blocks aligned with tiles: band = diagonal tiles only
    ("e", 700, 3, 5, ((0, 1), (1, 299), (3, 130), (4, 270))),          # an epoch across four tiles, an empty epoch (id 2),
                                                                       # unequal padded sizes, masked tail
    ("f", 300, 2, 3, ((2, 100), (0, 100), (1, 100))),                  # runs not in id order
)


def case_id(case):
    return f"{case[0]}-N{case[1]}-c{case[2]}"


def case_named(name):
    return next(c for c in CASES if c[0] == name)


def case_gp(case):
    return np.array(syn.GP_BASE[case[2]], dtype=np.float64)


@dataclass(frozen=True)
class LooChunk:
    lwls: np.ndarray          # (c, N) rest-frame grids
    fl: np.ndarray
    sigma: np.ndarray
    epoch_index: np.ndarray   # (N,) int
    n_epochs: int


@functools.lru_cache(maxsize=None)
def case_chunk(case) -> LooChunk:
    """Grids and flux of ``synthetic.make_chunk`` (its seeded per-epoch velocities), one generated epoch per run, cut to the
    run's pixel count: the masked tail of every epoch shorter than the longest"""
    _, N, c, ne, runs = case
    width = max(n for _, n in runs)
    full = syn.make_chunk(c, len(runs), width, seed=9000 + N + c, sigma0=SIGMA)
    keep = np.zeros((len(runs), width), dtype=bool)
    for k, (_, n) in enumerate(runs):
        keep[k, :n] = True
    keep = keep.reshape(-1)
    ep = np.concatenate([np.full(n, e, dtype=np.int64) for e, n in runs])
    assert keep.sum() == N == ep.shape[0]
    out = LooChunk(np.ascontiguousarray(full.lwls[:, keep]), np.ascontiguousarray(full.fl[keep]),
                   np.ascontiguousarray(full.sigma[keep]), ep, ne)
    for a in (out.lwls, out.fl, out.sigma, out.epoch_index):
        a.setflags(write=False)
    return out


# ---- the closed forms --------------------------------------------------------------------------------------------------
def _matrix_ext(lwls, sigma, gp):
    import oracle
    lwls = np.atleast_2d(lwls)
    if lwls.dtype != _LD:
        lwls = np.asarray(lwls, dtype=np.float64)
    K = oracle._sym_ext(lwls, gp)
    K[np.diag_indices_from(K)] += np.asarray(sigma, dtype=_LD) ** 2
    return K


def _epoch_sets(epoch_index, n_epochs):
    ep = np.asarray(epoch_index)
    return [np.flatnonzero(ep == e) for e in range(n_epochs)]


def _finish(T, lnp, A, alpha, fl, epoch_index, n_epochs, solve_block):
    """the formulas from A and alpha in the number type ``T``; solve_block(A_ee, alpha_e) -> (s_e, log det A_ee)"""
    half_log_2pi = _HALF_LOG_2PI if T is _LD else T(float(_HALF_LOG_2PI))
    d = np.diag(A).copy()
    fl = np.asarray(fl, dtype=T)
    pix_logp = T(0.5) * np.log(d) - alpha * alpha / (T(2) * d) - half_log_2pi
    total = T(0)
    for v in pix_logp:
        total = total + v
    out = Loo(lnp, total, fl - alpha / d, T(1) / d, pix_logp, alpha / np.sqrt(d))
    if epoch_index is None:
        return out
    N = fl.shape[0]
    out.ep_resid = np.zeros(N, dtype=T)
    out.ep_chi2, out.ep_logp = np.zeros(n_epochs, dtype=T), np.zeros(n_epochs, dtype=T)
    out.ep_npix = np.zeros(n_epochs, dtype=np.int32)
    for e, I in enumerate(_epoch_sets(epoch_index, n_epochs)):
        if I.size == 0:
            continue
        s, logdet = solve_block(A[np.ix_(I, I)], alpha[I])
        out.ep_resid[I] = s
        out.ep_chi2[e] = alpha[I] @ s
        out.ep_logp[e] = T(-0.5) * out.ep_chi2[e] + T(0.5) * logdet - T(I.size) * half_log_2pi
        out.ep_npix[e] = I.size
    return out


def loo_ext(lwls, fl, sigma, gp, mu_GP=1.0, epoch_index=None, n_epochs=None) -> Loo:
    """every step in long double: K, its Cholesky factor, the explicit inverse with one Newton step, the closed forms"""
    import oracle
    K = _matrix_ext(lwls, sigma, gp)
    N = K.shape[0]
    L = oracle._chol_ext(K)
    Li = oracle._fsolve_ext(L, np.eye(N, dtype=_LD))
    X = Li.T @ Li
    X = X + X @ (np.eye(N, dtype=_LD) - K @ X)          # Newton: the residual of the inverse squared
    A = _LD(0.5) * (X + X.T)
    r = np.asarray(fl, dtype=_LD) - _LD(mu_GP)
    z = Li @ r
    lnp = _LD(-0.5) * (z @ z + _LD(2) * np.sum(np.log(np.diag(L))))
    alpha = A @ r

    def solve_block(Aee, ae):
        Le = oracle._chol_ext(Aee)
        y = oracle._fsolve_ext(Le, ae)
        s = oracle._fsolve_ext(Le.T[::-1, ::-1], y[::-1])[::-1]        # Le^-T y by the forward routine on the flipped system
        return s, _LD(2) * np.sum(np.log(np.diag(Le)))

    if epoch_index is not None and n_epochs is None:
        n_epochs = int(np.max(epoch_index)) + 1
    return _finish(_LD, lnp, A, alpha, fl, epoch_index, n_epochs, solve_block)


def loo_f64(lwls, fl, sigma, gp, mu_GP=1.0, epoch_index=None, n_epochs=None) -> Loo:
    """the same in float64: the oracle's fill, SciPy's cho_factor, K^-1 and alpha from cho_solve, cho_factor per epoch block"""
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
    A = cho_solve(factor, np.eye(N))
    lnp = -0.5 * (r @ alpha + np.sum(2 * np.log(np.diag(factor[0]))))

    def solve_block(Aee, ae):
        f = cho_factor(Aee, lower=False)
        return cho_solve(f, ae), np.sum(2 * np.log(np.diag(f[0])))

    if epoch_index is not None and n_epochs is None:
        n_epochs = int(np.max(epoch_index)) + 1
    return _finish(np.float64, lnp, A, alpha, fl, epoch_index, n_epochs, solve_block)


# ---- brute force: delete and condition on the rest -------------------------------------------------------------------------
def _condition_ext(K, r, I):
    """residual r[I] - K[I,o] K[o,o]^-1 r[o] and the covariance K[I,I] - K[I,o] K[o,o]^-1 K[o,I] of the set I given the rest"""
    import oracle
    N = K.shape[0]
    I = np.atleast_1d(I)
    o = np.setdiff1d(np.arange(N), I)
    if o.size == 0:
        return r[I].copy(), K[np.ix_(I, I)].copy()
    L = oracle._chol_ext(K[np.ix_(o, o)])
    V = oracle._fsolve_ext(L, K[np.ix_(o, I)])          # L^-1 K[o,I]
    y = oracle._fsolve_ext(L, r[o])
    return r[I] - V.T @ y, K[np.ix_(I, I)] - V.T @ V


def delete_pixel(lwls, fl, sigma, gp, mu_GP, i):
    """(mean, var) of pixel i predicted from all the others, long double"""
    K = _matrix_ext(lwls, sigma, gp)
    r = np.asarray(fl, dtype=_LD) - _LD(mu_GP)
    resid, C = _condition_ext(K, r, [i])
    return _LD(fl[i]) - resid[0], C[0, 0]


def delete_epoch(lwls, fl, sigma, gp, mu_GP, I):
    """(resid (n_e,), chi2) of the pixels I predicted from all the others, long double"""
    import oracle
    K = _matrix_ext(lwls, sigma, gp)
    r = np.asarray(fl, dtype=_LD) - _LD(mu_GP)
    resid, C = _condition_ext(K, r, I)
    y = oracle._fsolve_ext(oracle._chol_ext(C), resid)
    return resid, y @ y


# ---- references of the cases, and the float64 table ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_ext(case) -> Loo:
    ch = case_chunk(case)
    return loo_ext(ch.lwls, ch.fl, ch.sigma, case_gp(case), MU_GP, ch.epoch_index, ch.n_epochs)


def errors(got, ref: Loo) -> dict:
    """per output the error measure of tests/test_gpu_loo.py: pix_mean and ep_resid absolute; pix_var, ep_chi2 and loo_logp
    relative; pix_logp and ep_logp relative to max(1, |value|).  Epochs without pixels are exact zeros on both sides."""
    def ld(v):
        return np.asarray(v, dtype=_LD)

    def rel(a, b, floor=None):
        scale = np.abs(ld(b)) if floor is None else np.maximum(_LD(floor), np.abs(ld(b)))
        live = scale > 0
        return float(np.max(np.abs(ld(a) - ld(b))[live] / scale[live])) if np.any(live) else 0.0

    out = {"pix_mean": float(np.max(np.abs(ld(got.pix_mean) - ref.pix_mean))),
           "pix_var": rel(got.pix_var, ref.pix_var), "pix_logp": rel(got.pix_logp, ref.pix_logp, 1.0),
           "loo_logp": rel(np.atleast_1d(got.loo_logp), np.atleast_1d(ref.loo_logp))}
    if ref.ep_resid is not None and got.ep_resid is not None:
        out.update(ep_resid=float(np.max(np.abs(ld(got.ep_resid) - ref.ep_resid))), ep_chi2=rel(got.ep_chi2, ref.ep_chi2),
                   ep_logp=rel(got.ep_logp, ref.ep_logp, 1.0))
    return out


def measure_f64():
    rows = []
    for case in CASES:
        ch = case_chunk(case)
        f = loo_f64(ch.lwls, ch.fl, ch.sigma, case_gp(case), MU_GP, ch.epoch_index, ch.n_epochs)
        rows.append((case_id(case), errors(f, case_ext(case))))
    return rows


# ---- planted outliers: an SB2 chunk whose flux is a draw from its own GP plus noise ----------------------------------------
PLANT_EPOCHS, PLANT_PIX = 6, 40
# Pixel 5 lies in epoch 0, so exactly one pixel and one epoch disagree with the model.  Epoch 0 was chosen on the long-double
# reference alone: the orbit puts epochs 2 / 3 and 4 / 5 at nearly the same velocities, each of a pair is predicted mostly from
# the other, and an offset planted in one of them drags its partner below the epoch threshold as well (the reference flags both).
PLANT_PIXEL, PLANT_EPOCH = 5, 0
PLANT_PIXEL_OFFSET, PLANT_EPOCH_OFFSET = 0.3, 0.05
PLANT_SEED = 9400


@functools.lru_cache(maxsize=None)
def planted():
    """-> (chunk, p_orb, gp, lwls_ext): the observed-frame chunk (fl replaced by mu_GP + a draw from N(0, K) at the grids the
    long-double orbit gives, K with the noise on its diagonal, then the planted offsets), the SB2 orbit of
    ``synthetic.make_orbit_proposals``, the benchmark hyper-parameters and those grids"""
    import orbit_ext as oe
    ch = syn.make_chunk(2, PLANT_EPOCHS, PLANT_PIX, seed=PLANT_SEED, sigma0=SIGMA)
    p_orb = syn.make_orbit_proposals("SB2", 2, seed=PLANT_SEED)[1]
    gp = np.array(syn.GP_BASE[2], dtype=np.float64)
    ep = ch.epoch_index
    lwls = oe.shift_ext(ch.lwl, oe.velocities_ext("SB2", p_orb, ch.dates), ep)
    import oracle
    L = oracle._chol_ext(_matrix_ext(lwls, ch.sigma, gp))
    draw = np.random.default_rng(PLANT_SEED + 1).standard_normal(ch.N)
    fl = np.asarray(_LD(MU_GP) + L @ draw.astype(_LD), dtype=np.float64)
    fl[PLANT_PIXEL] += PLANT_PIXEL_OFFSET
    fl[ep == PLANT_EPOCH] += PLANT_EPOCH_OFFSET
    ch.fl = np.ascontiguousarray(fl)
    return ch, p_orb, gp, lwls


def flag(loo, pix_sigma=5.0, epoch_p=1e-4):
    """the rule of ``lnprob.loo_outliers`` on one result -> (pixels, epochs)"""
    from scipy.stats import chi2
    z = np.asarray(loo.pix_z, dtype=np.float64)
    npix = np.asarray(loo.ep_npix)
    sf = np.where(npix > 0, chi2.sf(np.asarray(loo.ep_chi2, dtype=np.float64), np.maximum(npix, 1)), 1.0)
    return np.flatnonzero(np.abs(z) > pix_sigma), np.flatnonzero(sf < epoch_p)


if __name__ == "__main__":
    rows = measure_f64()
    print(f"{'case':12s} " + " ".join(f"{k:>10s}" for k in OUTPUTS))
    for name, err in rows:
        print(f"{name:12s} " + " ".join(f"{err[k]:10.2e}" for k in OUTPUTS))
    print(f"{'max':12s} " + " ".join(f"{max(r[1][k] for r in rows):10.2e}" for k in OUTPUTS))
