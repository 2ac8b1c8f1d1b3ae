"""Drop-in for ``psoap.matrix_functions`` (the reference's only native module).

Same names, positional signatures and in-place/return-None contract as
/root/reference/psoap/matrix_functions.pyx:
``fill_V11_f`` :19-59, ``fill_V12_f`` :61-96, ``fill_V11_f_g`` :99-146,
``fill_V11_f_g_h`` :149-201.  The matrix is produced by the gfx950 fill kernel
and copied into the caller's array.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import as_f64, check, dptr


def _target(mat, shape):
    if not isinstance(mat, np.ndarray) or mat.dtype != np.float64 or mat.ndim != 2:
        raise ValueError("Buffer dtype mismatch, expected a 2-D float64 ndarray")
    if mat.shape != tuple(shape):
        raise ValueError(f"matrix has shape {mat.shape}, expected {tuple(shape)}")
    return mat if mat.flags.c_contiguous else np.empty(shape, dtype=np.float64)


def _fill_sym(mat, lwls, gp, sigma=None, device=None):
    lwls = as_f64(lwls)
    c, n_vec = lwls.shape
    N = len(mat)                      # pyx:23  N = len(mat)
    if n_vec < N:
        raise ValueError("wavelength vector shorter than the matrix")
    lwls = as_f64(lwls[:, :N])
    gp = as_f64(gp, (2 * c,))
    out = _target(mat, (N, N))
    sig = None if sigma is None else as_f64(sigma, (N,))
    dev = _lib.default_device() if device is None else device
    check(_lib.load().psoap_fill_sym(dev, c, N, dptr(lwls), dptr(gp), None if sig is None else dptr(sig),
                                     dptr(out)), "psoap_fill_sym")
    if out is not mat:
        mat[...] = out


def fill_V11_f(mat, lwl_f, amp_f, l_f):
    _fill_sym(mat, np.stack([as_f64(lwl_f)]), [amp_f, l_f])


def fill_V11_f_g(mat, lwl_f, lwl_g, amp_f, l_f, amp_g, l_g):
    _fill_sym(mat, np.stack([as_f64(lwl_f), as_f64(lwl_g)]), [amp_f, l_f, amp_g, l_g])


def fill_V11_f_g_h(mat, lwl_f, lwl_g, lwl_h, amp_f, l_f, amp_g, l_g, amp_h, l_h):
    _fill_sym(mat, np.stack([as_f64(lwl_f), as_f64(lwl_g), as_f64(lwl_h)]),
              [amp_f, l_f, amp_g, l_g, amp_h, l_h])


def fill_V11_timevar(mat, lwls, times, gp, tau, sigma=None, device=None):
    """The symmetric fill under the time-variable kernel (not in the reference; include/psoap_gp.h: psoap_fill_sym_tv), in
    place like its siblings: ``mat[i, j] = sum_c amp_c^2 exp(p_c (lwls[c, j] - lwls[c, i])^2 - (times[j] - times[i])^2 /
    (2 tau_c^2))`` for ``lwls`` (c, N), ``times`` (N,), ``gp = (amp_0, l_0, ...)`` and ``tau`` (c,).  With every
    ``tau = inf`` the matrix is bit-identical to ``fill_V11_f`` / ``_f_g`` / ``_f_g_h``."""
    lwls = as_f64(np.atleast_2d(as_f64(lwls)))
    c, n_vec = lwls.shape
    N = len(mat)
    if n_vec < N:
        raise ValueError("wavelength vector shorter than the matrix")
    lwls = as_f64(lwls[:, :N])
    times = as_f64(as_f64(times)[:N], (N,))
    gp = as_f64(gp, (2 * c,))
    tau = as_f64(np.atleast_1d(as_f64(tau)), (c,))
    out = _target(mat, (N, N))
    sig = None if sigma is None else as_f64(sigma, (N,))
    dev = _lib.default_device() if device is None else device
    check(_lib.load().psoap_fill_sym_tv(dev, c, N, dptr(lwls), dptr(times), dptr(gp), dptr(tau),
                                        None if sig is None else dptr(sig), dptr(out)), "psoap_fill_sym_tv")
    if out is not mat:
        mat[...] = out


def fill_V11_quasiperiodic(mat, lwls, times, gp, tau, gamma, period, sigma=None, device=None):
    """The symmetric fill under the quasi-periodic kernel (not in the reference; include/psoap_gp.h: psoap_fill_sym_qp), in
    place like its siblings: ``fill_V11_timevar``'s element times ``exp(-gamma_c sin^2(pi (times[j] - times[i]) / period_c))``
    per component, inside the one exponential; ``gamma``, ``period`` (c,).  With every ``gamma = 0`` the matrix is
    bit-identical to ``fill_V11_timevar``'s."""
    lwls = as_f64(np.atleast_2d(as_f64(lwls)))
    c, n_vec = lwls.shape
    N = len(mat)
    if n_vec < N:
        raise ValueError("wavelength vector shorter than the matrix")
    lwls = as_f64(lwls[:, :N])
    times = as_f64(as_f64(times)[:N], (N,))
    gp = as_f64(gp, (2 * c,))
    tau, gamma, period = (as_f64(np.atleast_1d(as_f64(v)), (c,)) for v in (tau, gamma, period))
    out = _target(mat, (N, N))
    sig = None if sigma is None else as_f64(sigma, (N,))
    dev = _lib.default_device() if device is None else device
    check(_lib.load().psoap_fill_sym_qp(dev, c, N, dptr(lwls), dptr(times), dptr(gp), dptr(tau), dptr(gamma), dptr(period),
                                        None if sig is None else dptr(sig), dptr(out)), "psoap_fill_sym_qp")
    if out is not mat:
        mat[...] = out


def fill_V12_f(mat, lwl_f, lwl_predict, amp_f, l_f):
    lwl_f = as_f64(lwl_f)
    lwl_predict = as_f64(lwl_predict)
    M, N = len(lwl_f), len(lwl_predict)   # pyx:65-66
    out = _target(mat, (M, N))
    check(_lib.load().psoap_fill_cross(_lib.default_device(), M, N, dptr(lwl_f), dptr(lwl_predict),
                                       float(amp_f), float(l_f), dptr(out)), "psoap_fill_cross")
    if out is not mat:
        mat[...] = out
