"""CPU checks of the quasi-periodic kernel's references (tests/quasiperiodic_reference.py), of the table the tolerances of
tests/test_gpu_quasiperiodic.py are derived from, of the six seeded defects, of the fit's direction on the float64 twin, and of
the boundary of the two new entry points: psoap_chunk_lnlike_qp_grad, psoap_fill_sym_qp."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import quasiperiodic_reference as qp
import timevar_reference as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("psoap_chunk_lnlike_qp_grad", "psoap_fill_sym_qp")
# the last row of the table in tests/test_gpu_quasiperiodic.py (python tests/quasiperiodic_reference.py): what the twin was
# measured at when the bounds were derived.  The twin must still be there: a change of NumPy or SciPy that moves it is seen here.
RECORDED = {"gp": 6.79e-17, "tau": 5.85e-17, "gamma": 6.86e-17, "period": 9.19e-17, "mu": 5.14e-17, "lwl": 1.62e-14,
            "lnp": 8.71e-16, "fill": 2.65e-13}
# the smallest factor by which a seeded defect must leave the derived bound of the output it sits in.  (The measured factors
# are 1e12 .. 6e13, profiles/quasiperiodic.md: a wrong formula misses by its own size, the bound is a few ulp of the scale.)
DEFECT_FACTOR = 1e6
INF = float("inf")


def test_the_cases_hold_what_the_tolerances_are_to_be_derived_on():
    assert [c[0] for c in qp.CASES] == [c[0] for c in tv.CASES] and [c[1] for c in qp.CASES] == [c[1] for c in tv.CASES]
    short = long_ = zero = periodic = False
    for case in qp.CASES:
        d = qp.case_data(case)
        assert d.tau.shape == d.gamma.shape == d.period.shape == (d.lwls.shape[0],)
        short |= bool(np.any((d.period < d.span / 20) & (d.gamma > 0)))
        long_ |= bool(np.any((d.period > d.span) & (d.gamma > 0)))
        zero |= bool(np.any(d.gamma == 0.0))
        periodic |= bool(np.any(np.isinf(d.tau) & (d.gamma > 0)))
    assert short and long_ and zero and periodic


def test_twin_is_where_the_table_has_it():
    """the float64 twin against long double on every case: within the recorded row (and not an order of magnitude inside it)"""
    rows = qp.measure_f64()
    for k, recorded in RECORDED.items():
        worst = max(e[k] for _, e in rows)
        assert worst <= 1.05 * recorded, (k, worst, recorded)
        assert worst >= 0.1 * recorded, (k, worst, recorded)
    b = qp.bounds()
    assert b["lnp"] == 1e-10 and all(b[k] == qp.MARGIN * max(e[k] for _, e in rows) for k in qp.OUTPUTS + ("fill",))


@pytest.mark.parametrize("defect", list(qp.DEFECTS))
def test_a_seeded_defect_leaves_the_derived_bound(defect):
    where = {"sin-for-sin2": "gamma", "gamma-sign": "gamma", "gamma-missing": "period", "dt-missing": "period"}
    k, factor = qp.defect_factor(defect)
    print(f"{defect}: {qp.DEFECTS[defect]} -- leaves the bound of {k} by a factor of {factor:.3g}")
    assert factor >= DEFECT_FACTOR
    if defect in where:
        assert k == where[defect]
        # a defect of one finishing formula leaves every other output where it was
        clean, seeded = qp.measure_f64(), qp.measure_f64(defect)
        for (_, a), (_, b) in zip(clean, seeded):
            assert all(a[o] == b[o] for o in qp.OUTPUTS + ("lnp",) if o != k)
    else:
        # a defect of the phase is in the matrix: the value sees it too
        b = qp.bounds()
        assert max(e["lnp"] for _, e in qp.measure_f64(defect)) > b["lnp"]


def test_zero_gamma_is_the_time_variable_twin_bit_for_bit_and_same_time_pixels_see_the_static_kernel():
    """the two exact rules hold in the twin as they must on the device: (-0 * s) * s = -0 and sinpi(0) = +0"""
    d = tv.case_data(tv.CASES[5])
    c = d.lwls.shape[0]
    want = tv.matrix_f64(d.lwls, d.times, d.gp, d.tau, d.sigma)
    got = qp.matrix_f64(d.lwls, d.times, d.gp, d.tau, np.zeros(c), np.array([0.013, 0.9, 7.0]) * d.span, d.sigma)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    static = tv.matrix_f64(d.lwls, d.times, d.gp, np.full(c, INF), d.sigma)
    qpm = qp.matrix_f64(d.lwls, d.times, d.gp, np.full(c, INF), np.full(c, 2.0), np.full(c, 0.3 * d.span), d.sigma)
    same = d.times[:, None] == d.times[None, :]
    assert np.array_equal(qpm[same].view(np.int64), static[same].view(np.int64)) and not np.array_equal(qpm, static)
    g = qp.qp_f64(d.lwls, d.times, d.fl, d.sigma, d.gp, d.tau, np.zeros(c), np.full(c, 0.2 * d.span), tv.MU_GP)
    t = tv.tv_f64(d.lwls, d.times, d.fl, d.sigma, d.gp, d.tau, tv.MU_GP)
    assert g.lnp == t.lnp and np.array_equal(g.gp, t.gp) and np.array_equal(g.tau, t.tau) and np.array_equal(g.lwl, t.lwl)
    assert np.all(g.period == 0.0) and np.all(g.gamma != 0.0)


def test_sincospi_twin_reduces_exactly():
    u = np.array([0.0, 0.5, 1.0, 1.5, 2.0, -0.5, 1e6 + 0.25, 33.125, -7.75])
    s, c = qp.sincospi_f64(u)
    assert s[0] == 0.0 and not np.signbit(s[0]) and s[2] == 0.0 and s[4] == 0.0
    assert s[1] == 1.0 and s[3] == -1.0 and s[5] == -1.0
    assert abs(s[6] - np.sqrt(0.5)) <= 2e-16 and abs(c[6] - np.sqrt(0.5)) <= 2e-16
    ld = np.longdouble
    ref_s = np.sin(ld("3.14159265358979323846264338327950288") * u.astype(ld))
    assert np.max(np.abs(s - ref_s)[[7, 8]]) <= 4e-16


def test_f64_gradient_agrees_with_central_differences_of_its_own_value():
    """Gamma and P of both components of N128-c2, steps 1e-5 relative, 1e-5 relative to the larger of the derivative and its
    cancellation scale (the reasoning of tests/test_timevar_reference.py)"""
    d = qp.case_data(qp.CASES[1])
    g = qp.qp_f64(d.lwls, d.times, d.fl, d.sigma, d.gp, d.tau, d.gamma, d.period, qp.MU_GP)

    def value(gamma=d.gamma, period=d.period):
        return qp.qp_f64(d.lwls, d.times, d.fl, d.sigma, d.gp, d.tau, gamma, period, qp.MU_GP).lnp

    for k in range(2):
        for name, base, an, scale in (("gamma", d.gamma, g.gamma, g.s_gamma), ("period", d.period, g.period, g.s_period)):
            h = 1e-5 * base[k]
            up, dn = base.copy(), base.copy()
            up[k] += h
            dn[k] -= h
            fd = (value(**{name: up}) - value(**{name: dn})) / (2 * h)
            assert abs(fd - an[k]) <= 1e-5 * max(abs(an[k]), float(scale[k])), (name, k, fd, an[k])


def test_fit_direction_on_the_twin():
    """What tests/test_gpu_quasiperiodic.py may ask of the device: on the planted chunk the drivers recover P_0 to 1 %, the
    periodicity statistic is positive and the scan over the test's grid peaks at the grid point nearest P_0; on the chunk drawn
    with Gamma = 0 the fit drives Gamma to 0 and the statistic is not positive beyond delta = 1e-8 |lnp|."""
    fc = qp.fit_case(True)
    gp, tau, gamma, period, lnp, lnp0, lnp_tv, res = qp.fit_on_twin(True)
    print(f"planted: gamma {gamma} period {period} (P_0 {fc.P0:.4f}) lnp {lnp:.4f} lnp(gamma = 0) {lnp0:.4f} lnp_timevar {lnp_tv:.4f}")
    assert abs(period[0] - fc.P0) <= 0.01 * fc.P0 and gamma[0] > 0.5 and lnp - lnp_tv > 10.0 and lnp_tv >= lnp0
    vg = qp.fit_twin(fc)
    grid = fc.P0 * np.linspace(0.5, 2.0, 31)
    scan = [vg(fc.truth[0], fc.truth[1], fc.truth[2], np.array([p, 1.0]))[0] for p in grid]
    assert int(np.argmax(scan)) == int(np.argmin(np.abs(grid - fc.P0)))
    fc0 = qp.fit_case(False)
    gp, tau, gamma, period, lnp, lnp0, lnp_tv, res = qp.fit_on_twin(False)
    print(f"gamma = 0: gamma {gamma} period {period} lnp {lnp!r} lnp_timevar {lnp_tv!r} statistic {lnp - lnp_tv:.3e}")
    assert gamma[0] < 1e-3 and lnp - lnp_tv <= 1e-8 * abs(lnp)
    score = qp.fit_twin(fc0)(fc0.truth[0], fc0.truth[1], np.zeros(2), fc0.truth[3])[3]
    assert score[0] < 0


# ---- the boundary ------------------------------------------------------------------------------------------------------------
def _declaration(name):
    with open(os.path.join(ROOT, "include", "psoap_gp.h")) as fh:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", fh.read())
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_bindings_and_definitions_agree():
    from psoap_amd import _lib
    with open(os.path.join(ROOT, "psoap_amd", "csrc", "psoap_gp.hip")) as fh:
        hip = fh.read()
    for name in NAMES:
        args = _declaration(name)
        assert len(args) == len(_lib.SIGNATURES[name][1]), name
        assert re.search(r'extern "C" int ' + name + r"\(", hip), name
    grad, fill = _declaration(NAMES[0]), _declaration(NAMES[1])
    assert len(grad) == 16 and len(fill) == 11
    # the argument order follows the time-variable entries: gamma and period behind tau, their gradients behind grad_tau
    assert [a.split("*")[-1].strip() for a in grad[3:8]] == ["lwl", "gp", "tau", "gamma", "period"]
    assert [a.split("*")[-1].strip() for a in grad[9:]] == ["lnp", "grad_gp", "grad_tau", "grad_gamma", "grad_period", "grad_lwl", "grad_mu"]
    assert [a.split("*")[-1].strip() for a in fill[3:]] == ["lwl", "t", "gp", "tau", "gamma", "period", "sigma", "out"]


def test_python_signatures():
    from psoap_amd import covariance, matrix_functions, synthetic
    from psoap_amd.chunk import ChunkHandle
    params = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert params(ChunkHandle.lnlike_qp) == ["self", "lwls", "gp", "tau", "gamma", "period", "mu_GP"]
    assert params(ChunkHandle.lnlike_qp_grad) == params(ChunkHandle.lnlike_qp)
    assert params(matrix_functions.fill_V11_quasiperiodic)[:7] == ["mat", "lwls", "times", "gp", "tau", "gamma", "period"]
    assert params(covariance.lnlike_quasiperiodic) == ["lwls", "fl", "sigma", "gp", "tau", "gamma", "period", "times", "mu_GP"]
    assert params(covariance.lnlike_quasiperiodic_grad) == params(covariance.lnlike_quasiperiodic)
    assert params(covariance.optimize_GP_quasiperiodic)[:10] == ["lwls", "fl", "sigma", "gp0", "tau0", "gamma0", "period0", "times",
                                                                 "free", "period_bounds"]
    assert params(covariance.period_scan)[:9] == ["lwls", "fl", "sigma", "gp", "tau", "gamma", "times", "periods", "component"]
    assert inspect.signature(covariance.period_scan).parameters["component"].default == 0
    assert params(synthetic.draw_quasiperiodic_flux) == ["lwls", "times", "sigma", "gp", "tau", "gamma", "period", "mu_GP", "seed"]


def test_library_refuses_bad_arguments_without_a_device():
    from psoap_amd import _lib
    L = _lib.load()
    p = (ctypes.c_double * 8)()
    assert L.psoap_chunk_lnlike_qp_grad(None, 1, 1, p, p, p, p, p, 1.0, p, p, p, p, p, None, None) != 0
    assert L.psoap_last_error() == b"psoap_chunk_lnlike_qp_grad: bad arguments"
    assert L.psoap_fill_sym_qp(0, 1, 2, p, p, p, p, None, p, None, p) != 0
    assert L.psoap_last_error() == b"psoap_fill_sym_qp: bad arguments"
    assert L.psoap_fill_sym_qp(0, 1, 2, p, p, p, p, p, None, None, p) != 0
    assert L.psoap_fill_sym_qp(0, 4, 2, p, p, p, p, p, p, None, p) != 0


def test_degenerate_input_is_answered_before_the_device():
    from psoap_amd import covariance
    d = qp.case_data(qp.CASES[0])
    for gamma, period, tau in (([-1.0, 0.0], d.period, d.tau), ([np.nan, 0.0], d.period, d.tau), ([INF, 0.0], d.period, d.tau),
                               (d.gamma, [0.0, 1.0], d.tau), (d.gamma, [np.nan, 1.0], d.tau), (d.gamma, [INF, 1.0], d.tau),
                               (d.gamma, d.period, [0.0, INF])):
        assert covariance.lnlike_quasiperiodic(d.lwls, d.fl, d.sigma, d.gp, tau, gamma, period, d.times) == -np.inf
        out = covariance.lnlike_quasiperiodic_grad(d.lwls, d.fl, d.sigma, d.gp, tau, gamma, period, d.times)
        assert out[0] == -np.inf and all(np.all(np.isnan(v)) for v in out[1:]) and len(out) == 7
    with pytest.raises(ValueError):
        covariance._fit_quasiperiodic(None, 2, d.gp, d.tau, d.gamma, d.period, {"phase": [True, True]}, (1.0, 2.0), 1e-10)
    with pytest.raises(ValueError):
        covariance._fit_quasiperiodic(None, 2, d.gp, d.tau, d.gamma, d.period, None, (1e9, 2e9), 1e-10)
    # period_scan: degenerate input as lnlike_quasiperiodic, and no gamma changed behind the caller's back
    grid = np.array([3.0, 4.0])
    with pytest.raises(ValueError, match=r"\(n, c\)"):
        covariance.period_scan(d.lwls, d.fl, d.sigma, d.gp, d.tau, [1.0, 0.5], d.times, grid)
    for gp, tau, gamma in ((d.gp * [1, 1, -1, 1], d.tau, [1.0, 0.0]), (d.gp, [0.0, INF], [1.0, 0.0]), (d.gp, d.tau, [np.nan, 0.0])):
        lnp, score = covariance.period_scan(d.lwls, d.fl, d.sigma, gp, tau, gamma, d.times, grid)
        assert lnp.shape == score.shape == (2,) and np.all(np.isneginf(lnp)) and np.all(np.isnan(score))
    with pytest.raises(ZeroDivisionError):
        covariance.period_scan(d.lwls, d.fl, d.sigma, d.gp * [1, 0, 1, 1], d.tau, [1.0, 0.0], d.times, grid)
    with pytest.raises(ValueError):
        covariance.period_scan(d.lwls, np.where(np.arange(d.fl.size) == 3, np.nan, d.fl), d.sigma, d.gp, d.tau, [1.0, 0.0], d.times, grid)
    assert covariance.lnlike_quasiperiodic(d.lwls, d.fl, d.sigma, d.gp, d.tau, d.gamma, [5e-309, 1.0], d.times) == -np.inf
    lo, hi = covariance.default_period_bounds(np.array([5.0, 5.0, 7.5, 6.0, 15.0]))
    assert (lo, hi) == (2.0, 10.0)
