"""CPU checks of the time-variable kernel's references (tests/timevar_reference.py) and of the boundary of the three new
entry points: psoap_chunk_set_times, psoap_chunk_lnlike_tv_grad, psoap_fill_sym_tv."""
import ctypes
import os
import re

import numpy as np

import grad_reference as gr
import timevar_reference as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("psoap_chunk_set_times", "psoap_chunk_lnlike_tv_grad", "psoap_fill_sym_tv")


def _small():
    """N = 100, c = 2 with BOTH time scales finite (0.25 and 2 x the span of the dates)"""
    d = tv.case_data(tv.CASES[0])
    return d, np.array([0.25, 2.0]) * d.span


def test_f64_gradient_agrees_with_central_differences_of_its_own_value():
    """every gp, every tau, mu_GP and three pixels of every component's grid.  Steps h = 1e-5 relative (1e-9 absolute on the
    ln-wavelengths, 1e-6 on mu_GP): the truncation error is O(h^2) of the third derivative, the rounding error of the value
    (|lnp| ~ 1e2..1e3, float64) over 2h is ~1e-14 |lnp| / h, so 1e-5 relative to the larger of the derivative and its
    cancellation scale S leaves both an order of magnitude."""
    d, tau = _small()

    def value(gp=d.gp, tau=tau, lwls=d.lwls, mu=tv.MU_GP):
        return tv.tv_f64(lwls, d.times, d.fl, d.sigma, gp, tau, mu).lnp

    g = tv.tv_f64(d.lwls, d.times, d.fl, d.sigma, d.gp, tau, tv.MU_GP)
    assert np.all(g.s_tau > 0) and np.all(g.tau != 0.0)

    def check(fd, an, scale, what):
        assert abs(fd - an) <= 1e-5 * max(abs(an), float(scale)), (what, fd, an, float(scale))

    for k in range(4):
        h = 1e-5 * d.gp[k]
        up, dn = d.gp.copy(), d.gp.copy()
        up[k] += h
        dn[k] -= h
        check((value(gp=up) - value(gp=dn)) / (2 * h), g.gp[k], g.s_gp[k], ("gp", k))
    for k in range(2):
        h = 1e-5 * tau[k]
        up, dn = tau.copy(), tau.copy()
        up[k] += h
        dn[k] -= h
        check((value(tau=up) - value(tau=dn)) / (2 * h), g.tau[k], g.s_tau[k], ("tau", k))
    h = 1e-6
    check((value(mu=tv.MU_GP + h) - value(mu=tv.MU_GP - h)) / (2 * h), g.mu, g.s_mu, "mu")
    h = 1e-9
    for k in range(2):
        for i in (0, 37, 99):
            up, dn = d.lwls.copy(), d.lwls.copy()
            up[k, i] += h
            dn[k, i] -= h
            check((value(lwls=up) - value(lwls=dn)) / (2 * h), g.lwl[k, i], g.s_lwl[k, i], ("lwl", k, i))


def test_all_infinite_tau_is_the_static_reference_to_the_last_bit():
    """tv_ext builds K and contracts with the expressions of the oracle and of grad_reference, and at tau = inf the temporal
    term is a signed zero: the value and the gradient are grad_ext's bits, the tau derivative is exactly 0 -- in long double
    and in float64"""
    shape = gr.CASES[0]
    ch, gp = gr.case_chunk(shape), gr.case_gp(shape)
    t = ch.dates[ch.epoch_index] - ch.dates.min()
    inf = np.full(2, np.inf)
    a, b = tv.tv_ext(ch.lwls, t, ch.fl, ch.sigma, gp, inf, gr.MU_GP), gr.case_ext(shape)
    assert a.lnp == b.lnp and a.mu == b.mu
    assert np.array_equal(a.gp, b.gp) and np.array_equal(a.lwl, b.lwl)
    assert np.array_equal(a.s_gp, b.s_gp) and np.array_equal(a.s_lwl, b.s_lwl)
    assert np.all(a.tau == 0.0) and np.all(a.s_tau == 0.0)
    f = tv.tv_f64(ch.lwls, t, ch.fl, ch.sigma, gp, inf, gr.MU_GP)
    assert np.all(f.tau == 0.0)
    # the float64 matrix at tau = inf: the static arguments' bits (p * d * d alone)
    K, args = tv.matrix_f64(ch.lwls, t, gp, inf, want_args=True)
    D = ch.lwls[0][None, :] - ch.lwls[0][:, None]
    static = -0.5 * (tv.C_KMS * tv.C_KMS) / (gp[1] * gp[1]) * D * D
    assert np.array_equal(args[0].view(np.int64), static.view(np.int64))


def test_cases_cover_what_the_gpu_tests_need():
    shapes = [(c[1][0], c[1][1]) for c in tv.CASES]
    assert shapes[:7] == [s[:2] for s in gr.CASES] and tv.CASES[7][3] and shapes[7] == (300, 2)
    for case in tv.CASES:
        d = tv.case_data(case)
        finite = np.isfinite(d.tau)
        if d.lwls.shape[0] == 2:
            assert finite.sum() == 1
        if d.lwls.shape[0] == 3:
            assert sorted(d.tau / d.span) == [0.25, 2.0, np.inf]
        assert d.times.min() == 0.0 and d.times.max() == d.span
    perm = tv.case_data(tv.CASES[7]).times
    assert np.any(np.diff(perm) < 0)


def _declaration(name):
    text = open(os.path.join(ROOT, "include", "psoap_gp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/psoap_gp.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entry_points_are_declared_bound_and_exported():
    from psoap_amd import _lib, build
    L = ctypes.CDLL(build.build())
    dp, vp = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
    as_ctype = {"psoap_chunk *": vp, "int": ctypes.c_int, "double": ctypes.c_double, "const double *": dp, "double *": dp}
    for name in NAMES:
        args = _declaration(name)
        assert hasattr(L, name), f"{name} is not exported by libpsoap_gp.so"
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        declared = [as_ctype[re.sub(r"\s*\w+$", "", a).strip()] for a in args]
        assert declared == list(argtypes), (name, args)
    assert len(_declaration("psoap_chunk_lnlike_tv_grad")) == 12 and len(_declaration("psoap_fill_sym_tv")) == 9


def test_null_arguments_are_refused_without_a_device():
    from psoap_amd import _lib
    L = _lib.load()
    x = np.zeros(4)
    p = _lib.dptr(x)
    assert L.psoap_chunk_set_times(None, p) != 0
    assert L.psoap_last_error() == b"psoap_chunk_set_times: bad arguments"
    assert L.psoap_chunk_lnlike_tv_grad(None, 1, 1, p, p, p, 1.0, p, p, p, None, None) != 0
    assert L.psoap_last_error() == b"psoap_chunk_lnlike_tv_grad: bad arguments"
    assert L.psoap_fill_sym_tv(0, 1, 2, p, None, p, p, None, p) != 0
    assert L.psoap_last_error() == b"psoap_fill_sym_tv: bad arguments"
    assert L.psoap_fill_sym_tv(0, 1, 2, p, p, p, None, None, p) != 0
    assert L.psoap_fill_sym_tv(0, 4, 2, p, p, p, p, None, p) != 0


def test_python_surface_and_the_short_circuits_without_a_device():
    import inspect
    import pytest
    from psoap_amd import covariance, matrix_functions
    from psoap_amd.chunk import ChunkHandle
    for f in ("set_times", "lnlike_tv", "lnlike_tv_grad"):
        assert callable(getattr(ChunkHandle, f))
    assert list(inspect.signature(covariance.optimize_GP_timevar).parameters) == [
        "lwls", "fl", "sigma", "gp0", "tau0", "times", "free_tau", "mu_GP", "ftol", "full_output"]
    assert list(inspect.signature(covariance.lnlike_timevar).parameters) == ["lwls", "fl", "sigma", "gp", "tau", "times", "mu_GP"]
    assert list(inspect.signature(matrix_functions.fill_V11_timevar).parameters)[:5] == ["mat", "lwls", "times", "gp", "tau"]
    x = np.linspace(8.5, 8.5001, 6)
    t = np.arange(6.0)
    for tau in ([0.0, 3.0], [-1.0, 3.0], [np.nan, 3.0]):
        lnp, g_gp, g_tau, g_lwl, g_mu = covariance.lnlike_timevar_grad([x, x], x, x, [0.2, 5.0, 0.1, 7.0], tau, t)
        assert lnp == -np.inf and g_gp.shape == (4,) and g_tau.shape == (2,) and g_lwl.shape == (2, 6)
        assert np.all(np.isnan(g_gp)) and np.all(np.isnan(g_tau)) and np.all(np.isnan(g_lwl)) and np.isnan(g_mu)
        assert covariance.lnlike_timevar([x, x], x, x, [0.2, 5.0, 0.1, 7.0], tau, t) == -np.inf
    with pytest.raises(ZeroDivisionError):
        covariance.lnlike_timevar([x], x, x, [0.2, 0.0], [3.0], t)
    with pytest.raises(ValueError):
        covariance.optimize_GP_timevar([x], x, x, [0.2, 5.0], [np.inf], t, free_tau=[True])
