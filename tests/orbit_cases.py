"""The case table of the orbit and Doppler front end (tests/test_gpu_orbit_front.py on the device, tests/test_orbit_cases.py
on the CPU): parameter vectors and dates at the places where a Kepler solve or a velocity assembly goes wrong, chunks with
the epoch counts at which the device code changes shape, and one case per way a proposal can be faster than light.

Everything is deterministic: psoap_amd.synthetic plus explicit edge vectors.  The reference is oracle/orbit_ext.py
(bisection, atan2, long double)."""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))

import orbit_ext  # noqa: E402
from psoap_amd import synthetic as syn  # noqa: E402

MODELS = ("SB1", "SB2", "ST1", "ST2", "ST3")
N_COMPONENTS = {"SB1": 1, "SB2": 2, "ST1": 1, "ST2": 2, "ST3": 3}
C_KMS = syn.C_KMS

# ---- the tolerance against the extended-precision reference ("orbit tolerance") ---------------------------
# |v - v_ext| <= C * u per component, u = orbit_ext.unit(model, p): eps64 * (sum over the velocity terms of
# K_eff (1 + sqrt(1+e)/(1-e)^1.5), + |gamma|) -- the condition of parameters -> velocity (one ulp of M at periastron).
# The constant is MEASURED ON THE CPU, oracle/orbit_oracle.py (double) against orbit_ext (long double) over this table,
# never against the device: tests/test_orbit_cases.py::test_fp64_oracle_agrees_with_ext re-measures it and fails if the
# table has outgrown the figure.  What feeds it: M = 2 pi tt / P rounded near 2 pi (6 ulp-units of M), and
# omega pi / 180 rounded for omega + 180 up to 540 degrees (9 rad: up to ~4.7 units of eps K).
CPU_ORACLE_MAX_UNITS = 5.2        # measured 5.107 (MEASURED below), rounded up
GPU_BOUND_UNITS = 4.0 * CPU_ORACLE_MAX_UNITS      # the device's sin / cos / atan / sqrt within an ulp or two of glibc's
# measured figures behind the constants (units of u): the CPU oracle's worst over VEL_CASES, and the device's worst over
# the same cases on the first MI355X run of tests/test_gpu_orbit_front.py (ST3, 3066 dates; largest |v - v_ext| there
# 4.7e-14 km/s, over the whole table 3.4e-10 km/s, on the eccentricity ladder at e = 0.999 where u is 5e-11 K)
MEASURED = {"cpu_oracle_max_units": 5.107, "device_max_units": 5.23}

E_LADDER = (0.0, 1e-12, 0.5, 0.79, float(np.nextafter(0.8, 0.0)), 0.8, 0.89, 0.95, 0.99, 0.999)

# index of each named parameter per model (registered order up to gamma)
NAMES = {
    "SB1": ("K", "e", "omega", "P", "T0", "gamma"),
    "SB2": ("q", "K", "e", "omega", "P", "T0", "gamma"),
    "ST1": ("K_in", "e_in", "omega_in", "P_in", "T0_in", "K_out", "e_out", "omega_out", "P_out", "T0_out", "gamma"),
    "ST2": ("q_in", "K_in", "e_in", "omega_in", "P_in", "T0_in", "K_out", "e_out", "omega_out", "P_out", "T0_out", "gamma"),
    "ST3": ("q_in", "K_in", "e_in", "omega_in", "P_in", "T0_in", "q_out", "K_out", "e_out", "omega_out", "P_out", "T0_out",
            "gamma"),
}
# the orbits of a model: suffix of their parameter names
ORBITS = {"SB1": ("",), "SB2": ("",), "ST1": ("_in", "_out"), "ST2": ("_in", "_out"), "ST3": ("_in", "_out")}


def with_params(model, base=None, **kw):
    """the model's base vector (synthetic.ORBIT_BASE) with named parameters replaced"""
    p = np.array(syn.ORBIT_BASE[model] if base is None else base, dtype=np.float64)
    for k, v in kw.items():
        p[NAMES[model].index(k)] = v
    return p


@dataclass(frozen=True)
class VelCase:
    """orbit.velocities(model, P, dates) against velocities_ext, proposal by proposal"""
    name: str
    model: str
    P: np.ndarray           # (B, n_orb)
    dates: np.ndarray       # (n_dates,)
    tags: tuple = ()


def _edge_dates(P, T0):
    """dates around one orbit's phase edges.  With P and T0 exactly representable and k P small, T0 + k P and t - T0 are
    exact, so tt is exactly 0 (t == T0, whole periods either side), exactly P/2 (M = pi, E lands on pi), and t < T0
    exercises the sign fix after fmod.  Near T0 = 0 the dates resolve tt/P to 1e-12 of 0 and of 1."""
    d = [T0, T0 + P, T0 + 7 * P, T0 - P, T0 - 3 * P,                    # tt == 0 exactly
         T0 + 0.5 * P, T0 + 4.5 * P, T0 - 0.5 * P,                      # tt == P/2 exactly
         T0 - 0.3 * P, T0 - 2.25 * P, T0 - 1e-3 * P,                    # t < T0
         T0 + 0.25 * P, T0 + 0.75 * P, T0 + 1e-3 * P, T0 + (1 - 1e-3) * P]
    if T0 == 0.0:
        d += [P * 5e-13, P * (1 - 5e-13), -P * 5e-13, P * (3 + 5e-13),  # tt/P within 1e-12 of 0 and of 1
              2.45e6, 2.45e6 + 0.3 * P, 2455123.456789]                 # JD-sized dates: up to 4.9e6 periods from T0
    else:
        d += [np.nextafter(T0, np.inf), np.nextafter(T0, -np.inf),      # one ulp of a JD either side of T0
              T0 + 1000 * P, T0 - 1000 * P]
    return np.array(d, dtype=np.float64)


# (P, T0): periods 0.5 d .. 2000 d; T0 = 0 and JD-sized; one pair with nothing exactly representable
_PHASE_CONFIGS = ((0.5, 0.0), (23.0, 0.0), (2000.0, 0.0), (0.5, 2455010.0), (23.0, 2455010.0), (2000.0, 2455010.0),
                  (3.7123, 2455010.3217))
_PHASE_E = (0.0, 0.3, 0.85, 0.99)
_OMEGAS = (0.0, 37.0, 90.0, 135.0, 180.0, 200.0, 270.0, 315.0, 359.5)
_QS = (0.05, 0.3, 1.0)
EPOCH_COUNTS = (1, 63, 64, 65, 257)


def max_stream_epochs(lanes: int) -> int:
    """the largest n_epochs psoap_stream_open admits (include/psoap_gp.h): the dispatcher keeps 3 n_epochs velocities, 16
    parameters (doubles) and one int per lane in the tile engine's 73728 bytes of LDS"""
    return ((73728 - 4 * lanes) // 8 - 16) // 3


STREAM_LANES = 4
MAX_EPOCHS = max_stream_epochs(STREAM_LANES)             # 3066


def _build_vel_cases():
    cases = []
    jd = syn.make_dates(12, seed=31)
    # ---- eccentricity ladder: every model, inner and outer orbit in turn
    for model in MODELS:
        for orb in ORBITS[model]:
            P = np.stack([with_params(model, **{"e" + orb: e}) for e in E_LADDER])
            T0, per = P[0][NAMES[model].index("T0" + orb)], P[0][NAMES[model].index("P" + orb)]
            dates = np.concatenate([jd, _edge_dates(per, T0)])
            cases.append(VelCase(f"ecc-{model}{orb}", model, P, dates, ("ecc",)))
    # ---- phase edges
    for model in MODELS:
        for orb in ORBITS[model]:
            for k, (per, T0) in enumerate(_PHASE_CONFIGS):
                P = np.stack([with_params(model, **{"e" + orb: e, "P" + orb: per, "T0" + orb: T0}) for e in _PHASE_E])
                dates = np.concatenate([_edge_dates(per, T0), jd[:4]])
                cases.append(VelCase(f"phase-{model}{orb}-P{per:g}-T{'0' if T0 == 0 else 'jd'}{k}", model, P, dates, ("phase",)))
    # ---- parameter roles: omega through the quadrants and beyond 180, q from 0.05 to 1 (ST3: q_in and q_out apart)
    for model in MODELS:
        rows = []
        for orb in ORBITS[model]:
            for om in _OMEGAS:
                rows.append(with_params(model, **{"omega" + orb: om}))
        if model in ("SB2", "ST2"):
            rows += [with_params(model, **{NAMES[model][0]: q, NAMES[model][3]: om}) for q in _QS for om in (37.0, 200.0)]
        if model == "ST3":
            rows += [with_params(model, q_in=qi, q_out=qo, omega_in=37.0, omega_out=200.0)
                     for qi in _QS for qo in _QS if qi != qo]
        cases.append(VelCase(f"roles-{model}", model, np.stack(rows), jd, ("roles",)))
    # ---- epoch counts: the second block of the 64-wide grid, ragged last blocks, the stream's largest count
    for model in MODELS:
        P = syn.make_orbit_proposals(model, 3, seed=700)
        P[2] = with_params(model, base=P[2], **{"e" + ORBITS[model][-1]: 0.93})
        for ne in EPOCH_COUNTS + (MAX_EPOCHS,):
            cases.append(VelCase(f"epochs-{model}-{ne}", model, P[:2] if ne == MAX_EPOCHS else P,
                                 front_dates(ne, seed=710 + ne % 97), ("epochs",)))
    return tuple(cases)


def front_dates(ne: int, seed: int) -> np.ndarray:
    """``ne`` observation dates [JD], NOT sorted (the epoch order of a chunk is the order of its spectra)"""
    d = syn.make_dates(ne, seed=seed)
    return d[np.random.default_rng([seed, 7]).permutation(ne)]


# ---- chunks for the paths whose velocities cannot be read back ----------------------------------------------------------
@dataclass
class FrontChunk:
    c: int
    n_epochs: int
    lwl: np.ndarray          # (N,)
    fl: np.ndarray
    sigma: np.ndarray
    epoch_index: np.ndarray  # (N,) int, NOT monotone; ragged: epochs hold different numbers of pixels, some none
    dates: np.ndarray        # (n_epochs,)

    @property
    def N(self):
        return self.lwl.shape[0]


def front_chunk(c: int, ne: int, seed: int, n_target: int = 1000) -> FrontChunk:
    """a chunk of ``ne`` epochs with N near ``n_target``: few pixels per epoch, a ragged mask (a tenth of the pixels
    dropped; for ne > n_target two epochs in three hold no pixel at all), epoch labels permuted so that epoch_index is not
    monotone"""
    if ne <= n_target:
        npx, mf = max(1, int(round(n_target / ne))), (0.1 if ne > 1 else 0.05)
    else:
        npx, mf = 1, 1.0 - n_target / ne
    ch = syn.make_chunk(c, ne, npx, seed=seed, masked_fraction=mf)
    perm = np.random.default_rng([seed, 11]).permutation(ne)
    return FrontChunk(c, ne, ch.lwl, ch.fl, ch.sigma, perm[ch.epoch_index].astype(np.int32), front_dates(ne, seed))


def grids_from_velocities(fc: FrontChunk, vel) -> np.ndarray:
    """(..., c, N) rest-frame grids on the host, in the expression that reproduces the device's bits:
    ``lwl + (-v) / c_kms`` -- one negation (exact), one IEEE division, one addition; k_doppler_shift and the resident
    stream's dispatcher evaluate exactly this, and nothing in it can contract into a fused multiply-add."""
    vel = np.asarray(vel, dtype=np.float64)
    return fc.lwl + (-vel[..., fc.epoch_index]) / C_KMS


# ---- the -inf rule ------------------------------------------------------------------------------------------------------
FAST_MARGIN = 1.001      # by the _ext reference: some |v| >= 1.001 c in a fast proposal ...
SLOW_MARGIN = 0.999      # ... and every |v| <= 0.999 c in a slow one (and in the named slow components of a fast one)


@dataclass(frozen=True)
class FastCase:
    name: str
    model: str
    fast: np.ndarray            # the proposal that exceeds c_kms
    slow: np.ndarray            # its replacement: the same vector with the cause removed
    dates: np.ndarray
    fast_components: tuple      # which components exceed c; every other component stays slow
    fast_epochs: int = 0        # > 0: exactly this many epochs exceed c


def _one_epoch_dates(per, T0, n=16):
    """``n`` dates of which exactly one (index 5) is a periastron passage; the others keep 0.1 of a period away from one"""
    ph = np.linspace(0.1, 0.9, n)
    k = np.arange(n) % 5
    d = T0 + per * (k + ph)
    d[5] = T0 + 3 * per
    return d


def _build_fast_cases():
    jd = syn.make_dates(10, seed=41)
    out = []

    def add(name, model, comps, dates=jd, fast_epochs=0, **kw):
        base = with_params(model, **kw.pop("both", {}))
        out.append(FastCase(name, model, with_params(model, base=base, **kw), base, dates, comps, fast_epochs))

    # primary K (SB2 / ST2: q = 2.5 keeps the secondary's K/q slow)
    add("primary-K-SB1", "SB1", (0,), K=5.0e5)
    add("primary-K-SB2", "SB2", (0,), K=5.0e5, both={"q": 2.5, "e": 0.1})
    add("primary-K-ST2", "ST2", (0,), K_in=5.0e5, both={"q_in": 2.5, "e_in": 0.1})
    # the secondary alone, through a small q: K = 2e4 is slow, K/q = 4e5 is not
    add("secondary-q-SB2", "SB2", (1,), q=0.05, both={"K": 2.0e4})
    add("secondary-q-ST3", "ST3", (1,), q_in=0.05, both={"K_in": 2.0e4})
    # the tertiary alone, through a small q_out
    add("tertiary-qout-ST3", "ST3", (2,), q_out=0.05, both={"K_out": 2.0e4})
    # gamma alone: every component
    add("gamma-SB1", "SB1", (0,), gamma=-3.2e5)
    add("gamma-ST1", "ST1", (0,), gamma=3.2e5)
    add("gamma-ST3", "ST3", (0, 1, 2), gamma=3.2e5)
    # the outer term v3 alone: primary (and secondary) through K_out; ST3's tertiary K_out/q_out kept slow by q_out = 4
    add("v3-ST1", "ST1", (0,), K_out=5.0e5)
    add("v3-ST2", "ST2", (0, 1), K_out=5.0e5)
    add("v3-ST3", "ST3", (0, 1), K_out=5.0e5, both={"q_out": 4.0, "e_out": 0.05})
    # exactly one epoch out of many: e = 0.9, omega = 0 -- K (1 + e) at periastron, at most K (0.9 + cos f) elsewhere
    per, T0 = 23.0, 2455010.0
    add("one-epoch-SB1", "SB1", (0,), dates=_one_epoch_dates(per, T0), fast_epochs=1, K=1.7e5,
        both={"e": 0.9, "omega": 0.0, "P": per, "T0": T0})
    add("one-epoch-SB2", "SB2", (0,), dates=_one_epoch_dates(per, T0), fast_epochs=1, K=1.7e5,
        both={"q": 2.5, "e": 0.9, "omega": 0.0, "P": per, "T0": T0})
    return tuple(out)


VEL_CASES = _build_vel_cases()
FAST_CASES = _build_fast_cases()
FAST_POSITIONS = ("first", "middle", "last")


def fast_batch(case: FastCase, B: int, where: str, seed: int = 720):
    """(B, n_orb) slow proposals around the case's slow vector with the fast one at ``where``, the same batch with the slow
    replacement there, and the index"""
    i = {"first": 0, "middle": B // 2, "last": B - 1}[where]
    rng = np.random.default_rng([seed, B])
    slow = np.repeat(case.slow[None], B, axis=0)
    m = case.model
    for orb in ORBITS[m]:                    # a different slow orbit per row: K and omega jittered, everything else kept
        j = NAMES[m].index("omega" + orb)
        slow[:, j] += rng.uniform(-20.0, 20.0, size=B)
    fast = slow.copy()
    fast[i] = case.fast
    slow[i] = case.slow
    return fast, slow, i


# ---- seeded defects (tests/test_orbit_cases.py: every one must be rejected by the table) --------------------------------
DEFECTS = ("omega_not_plus_180", "K_times_q", "no_sign_fix", "newton_4_iterations", "st3_in_out_swapped",
           "tertiary_without_gamma", "tertiary_with_v3", "e_cos_omega_dropped")


def kernel_restated(model, p, dates, defect=None):
    """Python restatement of the device's orbit_velocities_at (psoap_amd/csrc/orbit_kernels.hpp: fmod + sign fix, Newton from
    M or pi, the tan half-angle formula), in double, with at most one seeded defect"""
    assert defect is None or defect in DEFECTS
    p = [float(x) for x in p]
    dates = np.atleast_1d(np.asarray(dates, dtype=np.float64))

    def anomaly(T0, P, e):
        tt = np.fmod(dates - T0, P)
        if defect != "no_sign_fix":
            tt = np.where((tt != 0.0) & (tt < 0.0), tt + P, tt)
        M = 2 * np.pi * tt / P
        E = M.copy() if e < 0.8 else np.full_like(M, np.pi)
        done = np.zeros(M.shape, dtype=bool)
        for _ in range(4 if defect == "newton_4_iterations" else 64):
            dE = (E - e * np.sin(E) - M) / (1.0 - e * np.cos(E))
            E = np.where(done, E, E - dE)
            done |= np.abs(dE) <= 1e-16 * np.maximum(1.0, np.abs(E))
            if done.all():
                break
        th = 2.0 * np.arctan(np.sqrt((1.0 + e) / (1.0 - e)) * np.tan(0.5 * E))
        return np.where(E < np.pi, th, th + 2 * np.pi)

    def term(K, e, om, f):
        w = om * np.pi / 180.0
        return K * (np.cos(w + f) + (0.0 if defect == "e_cos_omega_dropped" else e * np.cos(w)))

    flip = 0.0 if defect == "omega_not_plus_180" else 180.0
    ratio = (lambda K, q: K * q) if defect == "K_times_q" else (lambda K, q: K / q)
    if model == "SB1":
        K, e, om, P, T0, g = p
        return np.atleast_2d(term(K, e, om, anomaly(T0, P, e)) + g)
    if model == "SB2":
        q, K, e, om, P, T0, g = p
        f = anomaly(T0, P, e)
        return np.vstack([term(K, e, om, f) + g, term(ratio(K, q), e, om + flip, f) + g])
    q_in = q_out = None
    if model != "ST1":
        q_in, p = p[0], p[1:]
    inner, p = p[:5], p[5:]
    if model == "ST3":
        q_out, p = p[0], p[1:]
    outer, g = p[:5], p[5]
    if model == "ST3" and defect == "st3_in_out_swapped":
        inner, outer = outer, inner
    K_in, e_in, om_in, P_in, T0_in = inner
    K_out, e_out, om_out, P_out, T0_out = outer
    f_in, f_out = anomaly(T0_in, P_in, e_in), anomaly(T0_out, P_out, e_out)
    v3 = term(K_out, e_out, om_out, f_out)
    rows = [term(K_in, e_in, om_in, f_in) + v3 + g]
    if q_in is not None:
        rows.append(term(ratio(K_in, q_in), e_in, om_in + flip, f_in) + v3 + g)
    if q_out is not None:
        third = term(ratio(K_out, q_out), e_out, om_out + flip, f_out)
        if defect != "tertiary_without_gamma":
            third = third + g
        if defect == "tertiary_with_v3":
            third = third + v3
        rows.append(third)
    return np.vstack(rows)


def units_off(model, p, got, ext):
    """largest |got - ext| / u over components and dates (u per component: orbit_ext.unit)"""
    u = orbit_ext.unit(model, p)
    d = np.abs(np.asarray(got, dtype=np.longdouble) - ext)
    return float(np.max(d / u[:, None]))
