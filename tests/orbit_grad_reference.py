"""CPU references for the orbit Jacobian and the chain rule of ``lnprob(p)`` (tests/test_orbit_grad_reference.py,
tests/test_gpu_orbit_grad.py).

    v[c, e] = sum of terms K (cos(w + f) + e cos w) + gamma,  w = omega_deg pi/180,  E - e sin E = M,  M = 2 pi tt / P

With D = 1 - e cos E (implicit differentiation of Kepler's equation at the converged E):

    df/dM = sqrt(1 - e^2) / D^2        df/de = sin f (2 + e cos f) / (1 - e^2)
    dM/dT0 = -2 pi / P                 dM/dP = -2 pi (t - T0) / P^2       (the unreduced t - T0)
    d/dK = cos(w + f) + e cos w        d/de = -K sin(w + f) df/de + K cos w
    d/domega_deg = -K (sin(w + f) + e sin w) pi/180
    d/dP = -K sin(w + f) df/dM dM/dP   d/dT0 = -K sin(w + f) df/dM dM/dT0       d/dgamma = 1
    K/q components (omega + 180): d/dq = -term/q, and 1/q in d/dK

``jacobian_ext`` evaluates them in np.longdouble on the anomalies of oracle/orbit_ext.py (bisection, atan2),
``jacobian_f64`` in float64 on a restatement of the device's Newton iteration.  Both return, per entry, the scale S_J: the sum
of the absolute values of the product-rule terms of that entry -- what an error of the entry is measured against.

``chain_ext`` is the whole chain in long double: grids shifted by ``orbit_ext.shift_ext``, ``grad_reference.grad_ext``, the
fold over the pixels of every epoch, the contraction with ``jacobian_ext``; its scale is
S_orb[k] = sum_c sum_e s_v[c, e] |J[c, e, k]| with s_v the fold of grad_reference's s_lwl.

Run as a script it prints the float64-against-long-double tables from which tests/test_gpu_orbit_grad.py takes its bounds.
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

import orbit_ext as oe  # noqa: E402
import grad_reference as gr  # noqa: E402
import orbit_cases as oc  # noqa: E402
from psoap_amd import synthetic as syn  # noqa: E402

_LD = np.longdouble
N_ORB = oe.N_PARAMS
N_COMP = oc.N_COMPONENTS
JAC_DEFECTS = ("reduced_phase_in_dMdP", "missing_pi_over_180", "wrong_sign_dT0", "dq_plus_term_over_q", "dfde_without_dEde",
               "st3_in_out_swapped")


# ---- anomalies ----------------------------------------------------------------------------------------------------------
def _anomalies_ext(dates, T0, P, e):
    """(f, E, t - T0) in long double; t - T0 is the double difference both sides share (orbit_ext.phase)"""
    E = oe.eccentric_anomaly(oe.mean_anomaly(dates, T0, P), e)
    f = oe.true_anomaly(dates, T0, P, e)
    return f, E, (np.asarray(dates, dtype=np.float64) - np.float64(T0)).astype(_LD)


def _anomalies_f64(dates, T0, P, e):
    """the device's arithmetic in float64 (psoap_amd/csrc/orbit_kernels.hpp: fmod + sign fix, Newton from M or pi, the tan
    half-angle formula)"""
    dt = dates - T0
    tt = np.fmod(dt, P)
    tt = np.where((tt != 0.0) & (tt < 0.0), tt + P, tt)
    M = 2 * np.pi * tt / P
    E = M.copy() if e < 0.8 else np.full_like(M, np.pi)
    done = np.zeros(M.shape, dtype=bool)
    for _ in range(64):
        dE = (E - e * np.sin(E) - M) / (1.0 - e * np.cos(E))
        E = np.where(done, E, E - dE)
        done |= np.abs(dE) <= 1e-16 * np.maximum(1.0, np.abs(E))
        if done.all():
            break
    th = 2.0 * np.arctan(np.sqrt((1.0 + e) / (1.0 - e)) * np.tan(0.5 * E))
    return np.where(E < np.pi, th, th + 2 * np.pi), E, dt


# ---- the formulas, in the number type T ---------------------------------------------------------------------------------
def _term_grad(K, e, omega_deg, f, E, dt, P, T, defect=None):
    """derivatives of K (cos(w + f) + e cos w) with respect to (K, e, omega_deg, P, T0) and their scales: (5, n), (5, n);
    also the term itself"""
    pi = oe.PI if T is _LD else T(np.pi)
    K, e, P = T(K), T(e), T(P)
    deg = T(1) if defect == "missing_pi_over_180" else pi / T(180)
    w = T(omega_deg) * pi / T(180)
    swf, cwf, sw, cw = np.sin(w + f), np.cos(w + f), np.sin(w), np.cos(w)
    D = T(1) - e * np.cos(E)
    one_e2 = (T(1) - e) * (T(1) + e)
    df_dM = np.sqrt(one_e2) / (D * D)
    if defect == "dfde_without_dEde":
        # only the explicit e of tan(f/2) = sqrt((1+e)/(1-e)) tan(E/2), E held fixed: df/de = sin f / (1 - e^2)
        df_de = np.sin(f) / one_e2
    else:
        df_de = np.sin(f) * (T(2) + e * np.cos(f)) / one_e2
    dM_dT0 = (T(1) if defect == "wrong_sign_dT0" else T(-1)) * T(2) * pi / P
    if defect == "reduced_phase_in_dMdP":
        tt = np.fmod(dt, P)
        dt = np.where(tt < 0, tt + P, tt)
    dM_dP = -T(2) * pi * dt / (P * P)
    g = np.stack([cwf + e * cw,
                  -K * swf * df_de + K * cw,
                  -K * (swf + e * sw) * deg,
                  -K * swf * df_dM * dM_dP,
                  -K * swf * df_dM * dM_dT0])
    s = np.stack([np.abs(cwf) + np.abs(e * cw),
                  np.abs(K * swf * df_de) + np.abs(K * cw),
                  np.abs(K) * (np.abs(swf) + np.abs(e * sw)) * deg,
                  np.abs(K * swf * df_dM * dM_dP),
                  np.abs(K * swf * df_dM * dM_dT0)])
    return g, s, K * (cwf + e * cw)


def _jacobian(model, p, dates, T, anomalies, defect=None):
    p = [float(x) for x in p]
    if len(p) != N_ORB[model]:
        raise ValueError(f"{model} takes {N_ORB[model]} orbital parameters")
    dates = np.atleast_1d(np.asarray(dates, dtype=np.float64))
    c, n, npar = N_COMP[model], dates.shape[0], N_ORB[model]
    J, S = np.zeros((c, n, npar), dtype=T), np.zeros((c, n, npar), dtype=T)
    sign_q = T(1) if defect == "dq_plus_term_over_q" else T(-1)

    def put(row, at, K, e, om, an, P, q=None, q_at=None):
        """the term of one orbit in component ``row``: parameters at columns at .. at + 4 (K first), q at ``q_at``"""
        Keff = T(K) if q is None else T(K) / T(q)
        g, s, term = _term_grad(Keff, e, om if q is None else om + 180.0, *an, P, T, defect)
        if q is not None:
            J[row, :, q_at], S[row, :, q_at] = sign_q * term / T(q), np.abs(term / T(q))
            g[0], s[0] = g[0] / T(q), s[0] / T(q)
        J[row, :, at:at + 5] += g.T
        S[row, :, at:at + 5] += s.T

    if model in ("SB1", "SB2"):
        o = 1 if model == "SB2" else 0
        K, e, om, P, T0 = p[o:o + 5]
        an = anomalies(dates, T0, P, e)
        put(0, o, K, e, om, an, P)
        if model == "SB2":
            put(1, o, K, e, om, an, P, q=p[0], q_at=0)
        J[:, :, o + 5] = S[:, :, o + 5] = T(1)
        return J, S
    o = 0 if model == "ST1" else 1
    oo = o + 5 + (1 if model == "ST3" else 0)
    inner, outer = p[o:o + 5], p[oo:oo + 5]
    if defect == "st3_in_out_swapped" and model == "ST3":
        inner, outer = outer, inner
    an_in = anomalies(dates, inner[4], inner[3], inner[1])
    an_out = anomalies(dates, outer[4], outer[3], outer[1])
    put(0, o, *inner[:3], an_in, inner[3])
    put(0, oo, *outer[:3], an_out, outer[3])
    if c >= 2:
        put(1, o, *inner[:3], an_in, inner[3], q=p[0], q_at=0)
        put(1, oo, *outer[:3], an_out, outer[3])
    if c == 3:
        put(2, oo, *outer[:3], an_out, outer[3], q=p[o + 5], q_at=o + 5)
    J[:, :, oo + 5] = S[:, :, oo + 5] = T(1)
    return J, S


def jacobian_ext(model, p, dates, defect=None):
    """(J, S_J), each (c, n_dates, n_orb) np.longdouble, for one orbital parameter vector (registered order up to gamma)"""
    return _jacobian(model, p, dates, _LD, _anomalies_ext, defect)


def jacobian_f64(model, p, dates):
    """the same in float64 NumPy, on the device's Newton iteration restated"""
    return _jacobian(model, p, dates, np.float64, _anomalies_f64)


def rel_to_scale(got, ref, scale):
    """max |got - ref| / S over the entries with S > 0; where S == 0 (structural zeros) got must be exactly 0"""
    got, ref, scale = (np.asarray(v, dtype=_LD) for v in (got, ref, scale))
    live = scale > 0
    assert np.all(got[~live] == 0) and np.all(ref[~live] == 0)
    return float(np.max(np.abs(got - ref)[live] / scale[live])) if live.any() else 0.0


# ---- the chain ----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ChainCase:
    model: str
    N: int
    n_epochs: int
    n_pix: int

    @property
    def c(self):
        return N_COMP[self.model]

    @property
    def id(self):
        return f"{self.model}-N{self.N}"

    @property
    def p_orb(self):
        return np.array(syn.ORBIT_BASE[self.model], dtype=np.float64)

    @property
    def gp(self):
        return np.array(syn.GP_BASE[self.c], dtype=np.float64)

    @property
    def chunk(self):
        """grad_reference's chunk of exactly N pixels with unequal epochs"""
        return gr.case_chunk((self.N, self.c, self.n_epochs, self.n_pix))


# N at the edges of the 128-row tiles, every component count, inner + outer orbits (tests/test_gpu_orbit_grad.py)
CHAIN_CASES = (ChainCase("SB2", 129, 5, 30), ChainCase("SB1", 300, 6, 60), ChainCase("SB2", 300, 6, 60),
               ChainCase("ST3", 300, 6, 60), ChainCase("ST1", 128, 5, 30))


@dataclass(frozen=True)
class Chain:
    lnp: float
    orb: np.ndarray       # (n_orb,)
    s_orb: np.ndarray
    vel: np.ndarray       # (c, n_epochs): dlnL/dv
    s_vel: np.ndarray
    grad: gr.Grad         # gp, mu (and lwl) of the likelihood on the shifted grids


def fold(g_lwl, epoch_index, n_epochs, T=_LD):
    """sum over the pixels of every epoch: (c, N) -> (c, n_epochs), without the factor -1/c_kms"""
    g = np.asarray(g_lwl, dtype=T)
    out = np.zeros((g.shape[0], n_epochs), dtype=T)
    for e in range(n_epochs):
        out[:, e] = g[:, np.asarray(epoch_index) == e].sum(axis=1)
    return out


def chain_from(model, p_orb, gp, lwl, fl, sigma, epoch_index, dates, mu_GP) -> Chain:
    ne = len(dates)
    vel = oe.velocities_ext(model, p_orb, dates)
    g = gr.grad_ext(oe.shift_ext(lwl, vel, epoch_index), fl, sigma, gp, mu_GP)
    ckms = _LD(oe.C_KMS)
    g_v, s_v = -fold(g.lwl, epoch_index, ne) / ckms, fold(g.s_lwl, epoch_index, ne) / ckms
    J, _ = jacobian_ext(model, p_orb, dates)
    return Chain(g.lnp, np.einsum("ce,cek->k", g_v, J), np.einsum("ce,cek->k", s_v, np.abs(J)), g_v, s_v, g)


@functools.lru_cache(maxsize=None)
def chain_ext(case: ChainCase) -> Chain:
    ch = case.chunk
    return chain_from(case.model, case.p_orb, case.gp, ch.lwl, ch.fl, ch.sigma, ch.epoch_index, ch.dates, gr.MU_GP)


def chain_f64(case: ChainCase):
    """the float64 host composition: restated device velocities, host shift, grad_f64, velocity_gradient, jacobian_f64"""
    from psoap_amd import covariance
    ch = case.chunk
    vel = oc.kernel_restated(case.model, case.p_orb, ch.dates)
    lwls = ch.lwl + (-vel[:, ch.epoch_index]) / oe.C_KMS
    g = gr.grad_f64(lwls, ch.fl, ch.sigma, case.gp, gr.MU_GP)
    g_v = covariance.velocity_gradient(g.lwl, ch.epoch_index, ch.n_epochs)
    J, _ = jacobian_f64(case.model, case.p_orb, ch.dates)
    return np.einsum("ce,cek->k", g_v, J), g


# ---- the measurements behind the device's bounds --------------------------------------------------------------------------
def measure_jacobian_f64(cases=None):
    """jacobian_f64 against jacobian_ext over orbit_cases.VEL_CASES: per tag the largest |f64 - ext| / S_J"""
    worst = {}
    for case in (oc.VEL_CASES if cases is None else cases):
        for p in case.P:
            Je, Se = jacobian_ext(case.model, p, case.dates)
            Jf, _ = jacobian_f64(case.model, p, case.dates)
            r = rel_to_scale(Jf, Je, Se)
            key = (case.tags[0], case.model)
            worst[key] = max(worst.get(key, 0.0), r)
    return worst


def measure_chain_f64():
    rows = []
    for case in CHAIN_CASES:
        ref = chain_ext(case)
        orb, g = chain_f64(case)
        rows.append((case.id, gr.rel_to_scale(orb, ref.orb, ref.s_orb), gr.rel_to_scale(g.gp, ref.grad.gp, ref.grad.s_gp),
                     gr.rel_to_scale(g.mu, ref.grad.mu, ref.grad.s_mu)))
    return rows


if __name__ == "__main__":
    worst = measure_jacobian_f64()
    print("jacobian_f64 against jacobian_ext, max |f64 - ext| / S_J over orbit_cases.VEL_CASES")
    tags = sorted({k[0] for k in worst})
    print(f"{'model':6s} " + " ".join(f"{t:>10s}" for t in tags))
    for m in oc.MODELS:
        print(f"{m:6s} " + " ".join(f"{worst[(t, m)]:10.2e}" for t in tags))
    print(f"{'max':6s} {max(worst.values()):10.2e}")
    print()
    print("float64 host composition against chain_ext, max error / scale")
    print(f"{'case':10s} {'grad_orb':>10s} {'grad_gp':>10s} {'grad_mu':>10s}")
    rows = measure_chain_f64()
    for name, a, b, c_ in rows:
        print(f"{name:10s} {a:10.2e} {b:10.2e} {c_:10.2e}")
    print(f"{'max':10s} " + " ".join(f"{max(r[k] for r in rows):10.2e}" for k in (1, 2, 3)))
