"""The case list of tests/test_gpu_forms.py: one or more cases per (form, scheme) cell of the persistent Cholesky kernel
(psoap_amd/csrc/dag_launch.hpp: the 24 built forms; the LAT and wide forms under the latency scheme 1 and the following
scheme 2), their inputs and their CPU references.  Imported by the GPU module and by the CPU checks of
tests/test_form_cases.py (coverage of the cells, sensitivity of every case)."""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))

from psoap_amd import synthetic as syn  # noqa: E402

# the tolerance contract and the bound against the long-double value (about 20x LAPACK's own worst error;
# relative to the terms lnp is formed from: lnlike_refs)
LNP_RTOL = 1e-10
LNP_EXT_RTOL = 1e-11
MU_ATOL = 1e-10
SIGMA_ATOL = 1e-9
EXT_MAX_N = 1300          # long-double references up to here; the LAPACK oracle above

FORMS = tuple([f"{kind}/C{c}/{form}" for kind in ("lnlike", "predict") for c in (1, 2, 3) for form in ("TP", "LAT", "wide")] +
              [f"stream/C{c}/{form}" for c in (1, 2, 3) for form in ("TP", "LAT")])
# throughput forms run scheme 0; every LAT and wide form runs under scheme 1 and under scheme 2
CELLS = tuple(sorted((f, s) for f in FORMS for s in ((0,) if f.endswith("/TP") else (1, 2))))

# strongly correlated covariances: length scales far above the ~2.7 km/s pixel spacing (cond 1e4 - 1e6)
GP_CORR = {1: (0.2, 400.0), 2: (0.2, 300.0, 0.1, 100.0), 3: (0.2, 300.0, 0.1, 100.0, 0.05, 60.0)}


@dataclass(frozen=True)
class Case:
    kind: str                 # "lnlike" | "predict" | "stream"
    c: int
    form: str                 # "TP" | "LAT" | "wide"
    scheme: int               # the scheme the launch must run
    ne: int                   # epochs x pixels per epoch (before the mask)
    npx: int
    seed: int
    family: str = "base"      # "base": synthetic.GP_BASE; "corr": GP_CORR
    B: int = 3                # lnlike / stream: proposals; from 3 on, the middle one is rejected (negative amplitude)
    masked: float = 0.0
    env: tuple = ()           # environment of the launch: (("PSOAP_DAG_SCHEME", "1"), ...); () -- the automatic rule
    mode: int = 0             # predict: 0 components, 1 sum, 2 predict_f
    M: int = 0                # predict: points per prediction grid
    mu: float = 0.97          # lnlike / stream: mu_GP; predict: the prior mean (mode 0: of the first component)
    split: bool = False       # lnlike: the task list must hold a split tile (a final with S >= 2)

    @property
    def cell(self):
        return (f"{self.kind}/C{self.c}/{self.form}", self.scheme)

    @property
    def name(self):
        env = ",".join(f"{k[10:] if k.startswith('PSOAP_DAG_') else k}={v}" for k, v in self.env) or "auto"
        extra = f"-m{self.mode}-M{self.M}" if self.kind == "predict" else f"-B{self.B}"
        return (f"{self.kind}-C{self.c}-{self.form}-s{self.scheme}-N{self.ne}x{self.npx}{extra}-{self.family}"
                f"{'-masked' if self.masked else ''}-{env}")

    def chunk(self):
        return syn.make_chunk(self.c, self.ne, self.npx, seed=self.seed, masked_fraction=self.masked)

    def gp(self):
        return np.array(GP_CORR[self.c] if self.family == "corr" else syn.GP_BASE[self.c], dtype=np.float64)


def _env(scheme=None, wide=None):
    e = []
    if scheme is not None:
        e.append(("PSOAP_DAG_SCHEME", str(scheme)))
    if wide is not None:
        e.append(("PSOAP_DAG_WIDE", str(wide)))
    return tuple(e)


# sizes: N mod 128 in {1, 16, 17, 127} and mostly N mod 16 != 0, 2 .. 10 block rows
_SIZES = {"A": (3, 91), "B": (5, 77), "C": (9, 71), "D": (9, 73), "E": (8, 98), "F": (13, 69), "G": (7, 167), "H": (5, 51)}


def _build_cases():
    cases = []
    sz = lambda k: _SIZES[k]                                                   # noqa: E731
    # ---- likelihood: a batch of B with one rejected proposal; TP under scheme 0, LAT with the wide forms forbidden, wide
    # where the grid is at most one workgroup per compute unit (a small batch)
    for c, (tp, lat, wide) in {1: ("C", "D", "A"), 2: ("F", "B", "C"), 3: ("D", "G", "B")}.items():
        cases.append(Case("lnlike", c, "TP", 0, *sz(tp), seed=4100 + c, env=_env(0), split=True))
        cases.append(Case("lnlike", c, "TP", 0, *sz("H"), seed=4110 + c, family="corr", masked=0.1, env=_env(0)))
        for s in (1, 2):
            cases.append(Case("lnlike", c, "LAT", s, *sz(lat), seed=4120 + 10 * s + c, env=_env(s, 0), split=True,
                              family="corr" if s == 2 else "base"))
            cases.append(Case("lnlike", c, "wide", s, *sz(wide), seed=4140 + 10 * s + c, env=_env(s), split=True,
                              family="corr" if s == 1 else "base", masked=0.1 if c == 2 else 0.0))
    cases.append(Case("lnlike", 2, "LAT", 1, *sz("E"), seed=4170, B=1, env=_env(1, 0), family="corr"))
    cases.append(Case("lnlike", 3, "wide", 2, *sz("A"), seed=4171, B=1, env=_env(2), split=True))
    # natural reach (no environment): 32 matrices, 4 per ticket queue -- 14 block rows each stay under the latency rule's
    # limit (dag_auto_scheme: LAT, scheme 1), 24 do not (throughput); the counters say which form ran
    cases.append(Case("lnlike", 2, "LAT", 1, 17, 100, seed=4180, B=32, family="base", split=True))       # N = 1700: P = 14
    cases.append(Case("lnlike", 2, "TP", 0, 29, 103, seed=4181, B=32, family="corr", split=True))        # N = 2987: P = 24
    # ---- resident stream: scheme by stream_open's argument
    for c, (k0, k1, k2) in {1: ("B", "D", "G"), 2: ("C", "A", "F"), 3: ("G", "H", "C")}.items():
        for s, k in ((0, k0), (1, k1), (2, k2)):
            cases.append(Case("stream", c, "TP" if s == 0 else "LAT", s, *sz(k), seed=4200 + 10 * s + c, B=4,
                              family="corr" if (s + c) % 2 else "base", masked=0.1 if s == 1 else 0.0))
    # ---- predict: one matrix with the cross-covariances as appended column tiles; the width as for the likelihood
    modes = {1: (2, 0, 2, 2, 2), 2: (0, 1, 0, 1, 0), 3: (0, 0, 0, 0, 0)}
    for c in (1, 2, 3):
        ms = iter(modes[c])
        for k, (form, s, env) in enumerate((("TP", 0, _env(0)), ("LAT", 1, _env(1, 0)), ("LAT", 2, _env(2, 0)),
                                            ("wide", 1, _env(1)), ("wide", 2, _env(2)))):
            size = ("B", "D", "A", "F", "C")[(k + c) % 5]
            cases.append(Case("predict", c, form, s, *sz(size), seed=4300 + 10 * k + c, mode=next(ms), env=env,
                              M=(45, 97, 130)[(k + c) % 3], mu=(0.9, 1.15, 0.97)[k % 3],
                              family="corr" if (k + c) % 2 else "base", masked=0.1 if k == 2 else 0.0))
    return tuple(cases)


CASES = _build_cases()


# ---- inputs ----------------------------------------------------------------------------------------------------------
def lnlike_inputs(case: Case):
    """chunk, (B, c, N) rest-frame grids, (B, 2c) parameters, index of the rejected proposal (or None)"""
    ch = case.chunk()
    gps = syn.make_walkers(case.c, case.B, seed=case.seed + 1)
    base = np.array(syn.GP_BASE[case.c])
    gps = gps * (case.gp() / base)[None, :]                    # the family's scale, the walkers' jitter
    lw = syn.walker_lwls(ch, syn.make_walker_velocities(ch, case.B, seed=case.seed + 2))
    rej = None
    if case.B >= 3:
        rej = case.B // 2
        gps[rej, 0] = -0.5
    return ch, lw, gps, rej


def predict_inputs(case: Case):
    """chunk, (c, M) prediction grids (evenly spaced over each component's data range), prior means"""
    ch = case.chunk()
    pred = np.stack([np.linspace(w.min(), w.max(), case.M) for w in ch.lwls])
    mus = np.array([case.mu, 0.3, -0.2][:case.c]) if case.mode == 0 else np.array([case.mu])
    return ch, pred, mus


def prediction_offset(mode, c, mus):
    """what the data's prior mean is taken to be (covariance.py: 1.0 at :140,:184,:248; the prior mean at :52,:294)"""
    return 1.0 if (mode == 0 or (mode == 1 and c == 2)) else float(mus[0])


# ---- references ------------------------------------------------------------------------------------------------------
def lnlike_refs(case: Case, ch, lw, gps, rej, ext=True):
    """per proposal: the LAPACK oracle, and (N <= EXT_MAX_N, else None) the long-double value with the scale its bound is
    relative to -- max(1, |lnp|, (|r^T K^-1 r| + |log det K|) / 2): lnp is the difference of those two terms, and where they
    nearly cancel (strongly correlated data) no double-precision factorisation resolves lnp to 1e-11 of itself (LAPACK's
    own error on such an input, N = 784: 3e-11 of |lnp| = 16, the terms 6100).  -inf for the rejected proposal."""
    import oracle
    lap, ld, scale = np.empty(case.B), np.empty(case.B), np.empty(case.B)
    use_ext = ext and ch.N <= EXT_MAX_N
    for b in range(case.B):
        if b == rej:
            lap[b] = ld[b] = -np.inf
            scale[b] = np.nan
            continue
        lap[b] = oracle.lnlike(lw[b], ch.fl, ch.sigma, gps[b], case.mu)
        if use_ext:
            v, quad, logdet = oracle.lnlike_ext(lw[b], ch.fl, ch.sigma, gps[b], case.mu, terms=True)
            ld[b] = float(v)
            scale[b] = max(1.0, abs(float(v)), 0.5 * (abs(float(quad)) + abs(float(logdet))))
    return lap, ((ld, scale) if use_ext else None)


def predict_lapack(mode, lwls, fl, sigma, pred, mus, gp):
    """(mu, Sigma) from the LAPACK oracle for a predict mode"""
    import oracle
    c = lwls.shape[0]
    if mode == 0:
        return oracle.predict_components(lwls, fl, sigma, pred, mus, gp)
    if mode == 1:
        return oracle.predict_sum(lwls, fl, sigma, pred, float(mus[0]), gp)
    assert c == 1
    return oracle.predict_f(lwls[0], fl, sigma, pred[0], gp[0], gp[1], float(mus[0]))
