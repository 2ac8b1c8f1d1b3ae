"""Extended-precision reference for the orbit models and the Doppler shift -- TEST INFRASTRUCTURE ONLY (see
oracle/oracle.py for the rules).

Written from the equations, and sharing no method with the device code or with oracle/orbit_oracle.py:

    phase       tt = (t - T0) mod P                 (in double: the specified input rounding, see below)
    mean anom.  M  = 2 pi tt / P
    Kepler      E - e sin E = M                     solved by BISECTION on [0, 2 pi]: E - e sin E is increasing for
                                                    e < 1, so there is one root and no start value to choose
    true anom.  f/2 = atan2(sqrt(1+e) sin(E/2), sqrt(1-e) cos(E/2))
                                                    (no tan, no pole at E = pi, and no "+ 2 pi" branch: the velocity
                                                    depends on f only through cos(omega + f))
    velocity    K (cos(omega + f) + e cos omega) [+ outer term] + gamma

Everything after the phase reduction is ``np.longdouble`` (64-bit mantissa on x86: eps 1.1e-19).  The phase reduction
itself is part of the function under test and is done as the modelled project defines it: ``t - T0`` rounded to double
(the one rounding both sides share), then ``mod P``, which is exact in floating point.

``have_ext()`` says whether long double is wider than double here; callers skip their comparisons where it is not
(as the callers of ``oracle.lnlike_ext`` do).
"""
import numpy as np

LD = np.longdouble
C_KMS = 2.99792458e5
EXT_EPS_NEEDED = 2e-19
N_BISECT = 96                      # 2 pi / 2**96 is far below one long-double ulp of any E in [0, 2 pi]

PI = LD("3.14159265358979323846264338327950288")
TWO_PI = 2 * PI

N_PARAMS = {"SB1": 6, "SB2": 7, "ST1": 11, "ST2": 12, "ST3": 13}


def have_ext() -> bool:
    return bool(np.finfo(LD).eps < EXT_EPS_NEEDED)


def skip_reason() -> str:
    return f"np.longdouble has eps {float(np.finfo(LD).eps):.3g} here: no extended-precision reference"


def phase(t, T0, P):
    """tt = mod(fl64(t - T0), P) in double, result in [0, P) for P > 0 (the sign of the divisor)."""
    d = np.asarray(t, dtype=np.float64) - np.float64(T0)
    tt = np.fmod(d, np.float64(P))                   # exact; sign of the dividend
    return np.where(tt < 0.0, tt + np.float64(P), tt)    # tt + P is in [0, P]: rounding can only reach P itself


def mean_anomaly(t, T0, P):
    return TWO_PI * phase(t, T0, P).astype(LD) / LD(P)


def eccentric_anomaly(M, e):
    """root of E - e sin E = M on [0, 2 pi] by bisection (M in [0, 2 pi], long double)"""
    e = LD(e)
    M = np.asarray(M, dtype=LD)
    lo = np.zeros_like(M)
    hi = np.full_like(M, TWO_PI)
    for _ in range(N_BISECT):
        mid = lo + (hi - lo) / 2
        below = (mid - e * np.sin(mid)) < M
        lo = np.where(below, mid, lo)
        hi = np.where(below, hi, mid)
    return lo + (hi - lo) / 2


def true_anomaly(t, T0, P, e):
    E = eccentric_anomaly(mean_anomaly(t, T0, P), e)
    e = LD(e)
    return 2 * np.arctan2(np.sqrt(1 + e) * np.sin(E / 2), np.sqrt(1 - e) * np.cos(E / 2))


def _term(K, e, omega_deg, f):
    w = LD(omega_deg) * PI / 180
    return LD(K) * (np.cos(w + f) + LD(e) * np.cos(w))


def velocities_ext(model, p, dates):
    """(c, n_dates) ``np.longdouble`` km/s for one orbital parameter vector (registered order up to gamma)."""
    p = [float(x) for x in p]
    if len(p) != N_PARAMS[model]:
        raise ValueError(f"{model} takes {N_PARAMS[model]} orbital parameters")
    dates = np.atleast_1d(np.asarray(dates, dtype=np.float64))
    if model in ("SB1", "SB2"):
        q = None
        if model == "SB2":
            q, p = p[0], p[1:]
        K, e, om, P, T0, g = p
        f = true_anomaly(dates, T0, P, e)
        rows = [_term(K, e, om, f) + LD(g)]
        if q is not None:
            rows.append(_term(LD(K) / LD(q), e, om + 180.0, f) + LD(g))
        return np.vstack(rows)
    q_in = q_out = None
    if model != "ST1":
        q_in, p = p[0], p[1:]
    K_in, e_in, om_in, P_in, T0_in = p[:5]
    p = p[5:]
    if model == "ST3":
        q_out, p = p[0], p[1:]
    K_out, e_out, om_out, P_out, T0_out, g = p
    f_in = true_anomaly(dates, T0_in, P_in, e_in)
    f_out = true_anomaly(dates, T0_out, P_out, e_out)
    outer = _term(K_out, e_out, om_out, f_out)           # the inner pair's centre of mass about the tertiary
    rows = [_term(K_in, e_in, om_in, f_in) + outer + LD(g)]
    if q_in is not None:
        rows.append(_term(LD(K_in) / LD(q_in), e_in, om_in + 180.0, f_in) + outer + LD(g))
    if q_out is not None:
        rows.append(_term(LD(K_out) / LD(q_out), e_out, om_out + 180.0, f_out) + LD(g))
    return np.vstack(rows)


def shift_ext(lwl, vel, epoch_index):
    """(c, N) ``np.longdouble`` rest-frame ln-wavelengths ``lwl - v[c, epoch] / c_kms`` per pixel"""
    lwl = np.asarray(lwl, dtype=np.float64).astype(LD)
    vel = np.atleast_2d(np.asarray(vel, dtype=LD))
    ep = np.asarray(epoch_index)
    return lwl[None, :] - vel[:, ep] / LD(C_KMS)


# ---- the unit of the tolerance ("orbit tolerance") -----------------------------------------------------------
EPS64 = float(np.finfo(np.float64).eps)


def _amp(K, e):
    """K (1 + max |df/dM|) = K (1 + sqrt(1+e) / (1-e)^(3/2)): what one ulp of the mean anomaly costs at periastron"""
    return abs(K) * (1.0 + np.sqrt(1.0 + e) / (1.0 - e) ** 1.5)


def unit(model, p):
    """(c,) km/s: eps64 times the condition of the map parameters -> velocity, per component: every velocity term with the
    amplitude it actually uses (K, K/q, K_out, K_out/q_out), plus |gamma|."""
    p = [float(x) for x in p]
    if model == "SB1":
        K, e, _, _, _, g = p
        return EPS64 * np.array([_amp(K, e) + abs(g)])
    if model == "SB2":
        q, K, e, _, _, _, g = p
        return EPS64 * np.array([_amp(K, e) + abs(g), _amp(K / q, e) + abs(g)])
    q_in = q_out = None
    if model != "ST1":
        q_in, p = p[0], p[1:]
    K_in, e_in = p[0], p[1]
    p = p[5:]
    if model == "ST3":
        q_out, p = p[0], p[1:]
    K_out, e_out, g = p[0], p[1], p[5]
    out = [_amp(K_in, e_in) + _amp(K_out, e_out) + abs(g)]
    if q_in is not None:
        out.append(_amp(K_in / q_in, e_in) + _amp(K_out, e_out) + abs(g))
    if q_out is not None:
        out.append(_amp(K_out / q_out, e_out) + abs(g))
    return EPS64 * np.array(out)
