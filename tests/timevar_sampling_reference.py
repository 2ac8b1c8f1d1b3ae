"""CPU references for the time scales in ``lnprob(p)`` (tests/test_gpu_timevar_sampling.py, tests/test_timevar_vectors.py):
the batch route ``upload_orbits`` + ``set_tau`` + ``eval`` and ``lnprob_tv_grad``.

A proposal is orbital parameters, GP parameters and one time scale per component.  The reference of its value and gradient is
the long-double chain of tests/orbit_grad_reference.py with tests/timevar_reference.py's likelihood in the middle:

    velocities (oracle/orbit_ext.py, bisection)  ->  grids shifted in long double  ->  ``tv_ext`` over times = dates[epoch] - min
    grad_orb = sum_ce  (-fold(grad_lwl) / c_kms)[c, e]  J_ext[c, e, :]          grad_gp, grad_tau, grad_mu: ``tv_ext``'s own

``chain_f64`` is the float64 twin: the device's velocities restated, the host shift, ``tv_f64``, ``velocity_gradient``,
``jacobian_f64``.  Each output's error is measured against its cancellation scale S (tests/timevar_reference.py; for grad_orb
S_orb[k] = sum_ce s_v[c, e] |J[c, e, k]|).

Run as a script it prints (1) the twin's error against long double per case and output -- 8 times the largest is the device's
bound, the margin of tests/test_gpu_grad.py -- and (2) what three seeded defects of the batch route do to the values, each as
the largest relative change of lnp over the cases: tau read as (c, B) instead of (B, c), times not permuted with the pixels, and
the time scales of the previous upload kept.
"""
from __future__ import annotations

import functools
import os
import sys
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import grad_reference as gr  # noqa: E402
import orbit_cases as oc  # noqa: E402
import orbit_ext as oe  # noqa: E402
import orbit_grad_reference as ogr  # noqa: E402
import timevar_reference as tvr  # noqa: E402
from psoap_amd import synthetic as syn  # noqa: E402

_LD = np.longdouble
MU_GP = gr.MU_GP
B_MAX = 9
DEFECTS = ("tau_indexed_c_by_B", "times_not_permuted", "tau_of_previous_upload")


@dataclass(frozen=True)
class Case:
    """(model, N, epochs, pixels per epoch before the mask, pixels permuted): N = 100 a ragged tile, 129 one row past a tile,
    300 three tiles, 128 an exact tile"""
    model: str
    N: int
    n_epochs: int
    n_pix: int
    permuted: bool = False

    @property
    def c(self):
        return ogr.N_COMP[self.model]

    @property
    def id(self):
        return f"{self.model}-N{self.N}" + ("-perm" if self.permuted else "")


CASES = (Case("SB2", 100, 4, 30), Case("SB2", 129, 5, 30), Case("ST3", 300, 6, 60), Case("SB1", 128, 3, 50),
         Case("SB2", 129, 5, 30, True))


@dataclass(frozen=True)
class Data:
    lwl: np.ndarray           # (N,) observed frame
    fl: np.ndarray
    sigma: np.ndarray
    epoch_index: np.ndarray
    dates: np.ndarray
    times: np.ndarray         # dates[epoch_index] - min: what ``ChunkWorker(timevar={"times": None})`` sets
    span: float
    p_orb: np.ndarray         # (B_MAX, n_orb)
    gp: np.ndarray            # (B_MAX, 2c)
    tau: np.ndarray           # (B_MAX, c)
    perm: np.ndarray | None


@functools.lru_cache(maxsize=None)
def case_data(case: Case) -> Data:
    """The chunk of grad_reference.case_chunk and nine proposals: orbits and walkers from the seeded generators (row 0 the base
    vectors), and time scales that differ between the proposals AND between the components -- proposal b, component k has
    ``span * 0.2 * 1.35**b * (1 + 1.7 k)``, a fraction of the span of the dates up to a few spans, so that a transposed,
    stale or misplaced tau changes K by far more than rounding.  One component of one proposal is static (inf)."""
    ch = gr.case_chunk((case.N, case.c, case.n_epochs, case.n_pix))
    lwl, fl, sigma, ep = ch.lwl, ch.fl, ch.sigma, np.asarray(ch.epoch_index)
    perm = None
    if case.permuted:
        perm = np.random.default_rng(9100 + case.N).permutation(case.N)
        lwl, fl, sigma, ep = lwl[perm], fl[perm], sigma[perm], ep[perm]
    dates = np.asarray(ch.dates, dtype=np.float64)
    times = dates[ep] - dates[ep].min()
    span = float(dates.max() - dates.min())
    b, k = np.meshgrid(np.arange(B_MAX), np.arange(case.c), indexing="ij")
    tau = span * 0.2 * 1.35 ** b * (1.0 + 1.7 * k)
    tau[4, case.c - 1] = np.inf
    c_ = np.ascontiguousarray
    return Data(c_(lwl), c_(fl), c_(sigma), c_(ep), dates, c_(times), span,
                syn.make_orbit_proposals(case.model, B_MAX, seed=9200 + case.N), syn.make_walkers(case.c, B_MAX, seed=9300 + case.N),
                c_(tau), perm)


# ---- the long-double chain ----------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Chain:
    lnp: float
    orb: np.ndarray
    s_orb: np.ndarray
    grad: tvr.TvGrad          # gp, tau, mu (and lwl) on the shifted grids


def chain_from(model, p_orb, gp, tau, lwl, times, fl, sigma, epoch_index, dates, mu_GP=MU_GP) -> Chain:
    ne = len(dates)
    vel = oe.velocities_ext(model, p_orb, dates)
    g = tvr.tv_ext(oe.shift_ext(lwl, vel, epoch_index), times, fl, sigma, gp, tau, mu_GP)
    ckms = _LD(oe.C_KMS)
    g_v, s_v = -ogr.fold(g.lwl, epoch_index, ne) / ckms, ogr.fold(g.s_lwl, epoch_index, ne) / ckms
    J, _ = ogr.jacobian_ext(model, p_orb, dates)
    return Chain(g.lnp, np.einsum("ce,cek->k", g_v, J), np.einsum("ce,cek->k", s_v, np.abs(J)), g)


@functools.lru_cache(maxsize=None)
def chain_ext(case: Case, b: int) -> Chain:
    """proposal ``b`` of ``case`` in long double (computed once; the tests share it)"""
    d = case_data(case)
    return chain_from(case.model, d.p_orb[b], d.gp[b], d.tau[b], d.lwl, d.times, d.fl, d.sigma, d.epoch_index, d.dates)


def shifted_f64(case: Case, p_orb):
    """the grids as the device shifts them: its velocities restated in float64, ``lwl + (-v) / c_kms``"""
    d = case_data(case)
    vel = oc.kernel_restated(case.model, p_orb, d.dates)
    return d.lwl[None, :] + (-vel[:, d.epoch_index]) / oe.C_KMS


def chain_f64(case: Case, b: int):
    """the float64 twin of proposal ``b``: -> (grad_orb, TvGrad)"""
    from psoap_amd import covariance
    d = case_data(case)
    g = tvr.tv_f64(shifted_f64(case, d.p_orb[b]), d.times, d.fl, d.sigma, d.gp[b], d.tau[b], MU_GP)
    g_v = covariance.velocity_gradient(g.lwl, d.epoch_index, len(d.dates))
    J, _ = ogr.jacobian_f64(case.model, d.p_orb[b], d.dates)
    return np.einsum("ce,cek->k", g_v, J), g


OUTPUTS = ("orb", "gp", "tau", "mu")
GRAD_PROPOSALS = (0, 4)          # the base vectors, and the proposal with a static component


def errors(orb, g_gp, g_tau, g_mu, ref: Chain) -> dict:
    return {"orb": gr.rel_to_scale(orb, ref.orb, ref.s_orb), "gp": gr.rel_to_scale(g_gp, ref.grad.gp, ref.grad.s_gp),
            "tau": tvr.rel_tau(g_tau, ref.grad.tau, ref.grad.s_tau), "mu": gr.rel_to_scale(g_mu, ref.grad.mu, ref.grad.s_mu)}


def measure_twin():
    """the twin against long double over CASES x GRAD_PROPOSALS: rows (case, b, error / S per output)"""
    rows = []
    for case in CASES:
        for b in GRAD_PROPOSALS:
            orb, g = chain_f64(case, b)
            e = errors(orb, g.gp, g.tau, g.mu, chain_ext(case, b))
            rows.append((case.id, b) + tuple(e[k] for k in OUTPUTS))
    return rows


# ---- seeded defects of the batch route, in float64 ------------------------------------------------------------------------------
def lnp_f64(case: Case, b: int, tau, times=None):
    """lnp of proposal ``b`` in float64 at the time scales ``tau`` (c,) over ``times`` (default: the case's)"""
    from scipy.linalg import cho_factor, cho_solve
    d = case_data(case)
    K = tvr.matrix_f64(shifted_f64(case, d.p_orb[b]), d.times if times is None else times, d.gp[b], tau, d.sigma)
    factor = cho_factor(K, lower=False)
    r = d.fl - MU_GP
    return float(-0.5 * (r @ cho_solve(factor, r) + np.sum(2 * np.log(np.diag(factor[0])))))


def defect_inputs(case: Case, defect: str, B: int = B_MAX):
    """what a route with the defect would evaluate proposal b at: -> (tau (B, c), times (N,))"""
    assert defect in DEFECTS
    d = case_data(case)
    tau, times = d.tau[:B], d.times
    if defect == "tau_indexed_c_by_B":
        tau = np.ascontiguousarray(tau).reshape(case.c, B).T          # the (B, c) block read with the strides of (c, B)
    elif defect == "times_not_permuted":
        if d.perm is not None:
            times = times[np.argsort(d.perm)]                           # the times in the chunk's own order, pixels permuted
    else:
        tau = np.roll(tau, 1, axis=0) * 3.0                             # another batch's time scales: what was there before
    return np.ascontiguousarray(tau), times


def measure_defect(case: Case, defect: str, proposals=(0, 1, 8)):
    """largest |lnp_defect - lnp| / max(1, |lnp|) over ``proposals``"""
    d = case_data(case)
    tau, times = defect_inputs(case, defect)
    worst = 0.0
    for b in proposals:
        good = lnp_f64(case, b, d.tau[b])
        bad = lnp_f64(case, b, tau[b], times)
        worst = max(worst, abs(bad - good) / max(1.0, abs(good)))
    return worst


if __name__ == "__main__":
    rows = measure_twin()
    print("float64 twin against the long-double chain, error / scale")
    print(f"{'case':16s} {'b':>2s} " + " ".join(f"{'grad_' + k:>10s}" for k in OUTPUTS))
    for row in rows:
        print(f"{row[0]:16s} {row[1]:2d} " + " ".join(f"{v:10.2e}" for v in row[2:]))
    print(f"{'max':19s} " + " ".join(f"{max(r[k] for r in rows):10.2e}" for k in range(2, 6)))
    print()
    print("seeded defects: largest relative change of lnp (the value bound is 1e-10)")
    print(f"{'case':16s} " + " ".join(f"{k:>24s}" for k in DEFECTS))
    for case in CASES:
        print(f"{case.id:16s} " + " ".join(f"{measure_defect(case, k):24.2e}" for k in DEFECTS))
