"""Drop-in for the GP likelihood / prediction functions of ``psoap.covariance``.

Signatures, argument meaning, return types and error behaviour follow
/root/reference/psoap/covariance.py (``lnlike_f`` :299-331, ``lnlike_f_g`` :333-354,
``lnlike_f_g_h`` :356-376, ``lnlike`` :379, ``predict_f`` :25-54, ``predict_f_g``
:81-148, ``predict_f_g_sum`` :151-187, ``predict_f_g_h`` :190-251,
``predict_f_g_h_sum`` :253-297) so that ``psoap.sample_parallel``'s
``covariance.lnlike[model](self.V11, *lwls, self.fl, self.sigma, *p_GP)`` (:193)
works unchanged.  All arithmetic runs in the HIP library behind include/psoap_gp.h.

The ``V11`` argument is the caller's scratch matrix; the reference leaves
unspecified contents in it and no caller reads it back, so it is ignored here --
the matrix lives in HBM.  HIP is initialised lazily on the first call, i.e. in
the worker process after the fork.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict

import numpy as np

from . import _lib
from ._lib import as_f64, check, dptr
from .chunk import ChunkHandle

_MAX_CACHED_CHUNKS = 4
_handles: "OrderedDict[tuple, ChunkHandle]" = OrderedDict()


def _chunk_for(fl, sigma):
    """One persistent device handle per (fl, sigma) pair, keyed on the buffers and
    verified by content, so a Worker re-uses its resident chunk on every proposal."""
    fl = as_f64(fl)
    sigma = as_f64(sigma)
    key = (fl.ctypes.data, sigma.ctypes.data, fl.shape[0])
    h = _handles.get(key)
    if h is not None and np.array_equal(h.fl, fl) and np.array_equal(h.sigma, sigma):
        _handles.move_to_end(key)
        return h
    if h is not None:
        h.close()
        del _handles[key]
    from . import server as _server
    if _server.wanted():
        # PSOAP_GPU_SERVER: the chunk lives in the process that owns the GPU (psoap_amd/server.py), this worker never
        # initialises HIP -- the reference's worker-per-chunk model with dozens of workers per device
        h = _server.connect_chunk(fl.copy(), sigma.copy())
    else:
        h = ChunkHandle(fl.copy(), sigma.copy(), max_batch=1)
    _handles[key] = h
    while len(_handles) > _MAX_CACHED_CHUNKS:
        _, old = _handles.popitem(last=False)
        old.close()
    return h


def _chunk_without_baseline(fl, sigma):
    """``_chunk_for`` for the time-variable calls that take no baseline: the library's time-variable entries refuse a handle that
    has one, and a baseline cannot be taken off a handle, so a cached handle on which an earlier call of this module set one
    is closed and made again (its workspaces go with it; the next call with a baseline sets it again)."""
    h = _chunk_for(fl, sigma)
    if getattr(h, "_baseline", None) is None:
        return h
    for key in [k for k, v in _handles.items() if v is h]:
        del _handles[key]
    h.close()
    return _chunk_for(fl, sigma)


def release_handles():
    """Free every cached device chunk and the predict workspaces."""
    while _handles:
        _, h = _handles.popitem()
        h.close()
    while _predictors:
        _, p = _predictors.popitem()
        _lib.load().psoap_predictor_destroy(p)


# one reusable predict workspace per device: the retrieve loop predicts chunk after chunk
# (scripts/psoap_retrieve_ST3.py:148) and allocates only when a chunk outgrows the previous ones
_predictors: dict = {}


def _predictor():
    dev = _lib.default_device()
    p = _predictors.get(dev)
    if p is None:
        p = ctypes.c_void_p()
        check(_lib.load().psoap_predictor_create(ctypes.byref(p), dev), "psoap_predictor_create")
        _predictors[dev] = p
    return p


def last_predict_timings() -> dict:
    """Timings (ms) and algorithmic flops of the last ``predict_*`` call on the default device."""
    t = _lib.PredictTimings()
    check(_lib.load().psoap_predictor_timings(_predictor(), ctypes.byref(t)), "psoap_predictor_timings")
    return t.as_dict()


_NONFINITE = "array must not contain infs or NaNs"      # the message of scipy's check_finite


def _matrix_is_finite(lw: np.ndarray, sigma, gp) -> bool:
    """Would the reference's filled matrix (fill_V11_* + sigma**2 on the diagonal) be free of NaN / inf?  Entries are
    ``amp**2 * exp(-0.5 c**2 r**2 / l**2)`` with ``r`` a wavelength difference: a NaN wavelength, amplitude or length scale,
    an infinite amplitude, two infinite wavelengths of one sign in one component (inf - inf), or a non-finite
    uncertainty poison it; ONE infinite wavelength (exp(-inf) = 0) or an infinite length scale (exp(-0) = 1) do not."""
    if not np.all(np.isfinite(np.asarray(sigma, dtype=np.float64))):
        return False
    amps, ls = gp[0::2], gp[1::2]
    if not all(np.isfinite(a) for a in amps) or any(np.isnan(l) for l in ls):
        return False
    if np.any(np.isnan(lw)):
        return False
    if lw.shape[1] > 1 and (np.any(np.sum(np.isposinf(lw), axis=1) > 1) or np.any(np.sum(np.isneginf(lw), axis=1) > 1)):
        return False
    return True


def _lnlike(lwls, fl, sigma, gp, mu_GP):
    """Error behaviour of the reference on degenerate input, pinned by running the reference itself
    (tests/golden/make_golden_conventions.py -> golden_conventions_v1.json):

    * a negative hyper-parameter -> ``-inf`` before anything else (covariance.py:317,339,362);
    * a length scale of exactly 0 -> ``ZeroDivisionError`` (``-0.5 * c_kms2 / (l*l)`` in the Cython fills,
      matrix_functions.pyx:29,111-112,165-167: Cython checks float division);
    * anything non-finite in the covariance matrix -> ``ValueError``: ``lnlike_f`` / ``lnlike_f_g_h`` factor with
      scipy's ``check_finite`` (:325,370); ``lnlike_f_g`` factors unchecked (:348), but OpenBLAS's ``dpotrf`` does not
      stop at a NaN pivot, the factor comes back non-finite and the ``cho_solve`` that follows refuses it (:354);
    * a finite matrix that is not positive definite -> ``-inf`` (``LinAlgError`` caught, :327,350,372);
    * non-finite ``fl`` / ``mu_GP`` (the right-hand side of ``cho_solve``, :331,354,376) -> ``ValueError``.

    Behind the C ABI the device keeps its own convention (NaN in, NaN or -inf out, never an exception): include/psoap_gp.h."""
    gp = [float(g) for g in gp]
    if any(g < 0.0 for g in gp):
        return -np.inf
    if any(l == 0.0 for l in gp[1::2]):
        raise ZeroDivisionError("float division")
    lw = np.stack([as_f64(w) for w in lwls])
    if not _matrix_is_finite(lw, sigma, gp):
        raise ValueError(_NONFINITE)
    h = _chunk_for(fl, sigma)
    out = np.float64(h.lnlike(lw, gp, mu_GP))
    if np.isneginf(out):
        return out
    if not (np.all(np.isfinite(np.asarray(fl, dtype=np.float64))) and np.isfinite(mu_GP)):
        raise ValueError(_NONFINITE)
    return out


def lnlike_f(V11, wl_f, fl, sigma, amp_f, l_f, mu_GP=1.):
    return _lnlike([wl_f], fl, sigma, [amp_f, l_f], mu_GP)


def lnlike_f_g(V11, wl_f, wl_g, fl, sigma, amp_f, l_f, amp_g, l_g, mu_GP=1.):
    return _lnlike([wl_f, wl_g], fl, sigma, [amp_f, l_f, amp_g, l_g], mu_GP)


def lnlike_f_g_h(V11, wl_f, wl_g, wl_h, fl, sigma, amp_f, l_f, amp_g, l_g, amp_h, l_h, mu_GP=1.):
    return _lnlike([wl_f, wl_g, wl_h], fl, sigma, [amp_f, l_f, amp_g, l_g, amp_h, l_h], mu_GP)


# covariance.py:379
lnlike = {"SB1": lnlike_f, "SB2": lnlike_f_g, "ST1": lnlike_f, "ST2": lnlike_f_g, "ST3": lnlike_f_g_h}


def _predict(mode, lwls, fl, sigma, lwls_predict, mu_c, gp, want_sigma=True):
    lwls = np.stack([as_f64(w) for w in lwls])
    pred = np.stack([as_f64(w) for w in lwls_predict])
    c, N = lwls.shape
    M = pred.shape[1]
    fl = as_f64(fl, (N,))
    sigma = as_f64(sigma, (N,))
    mu_c = as_f64(mu_c)
    gp = as_f64(gp, (2 * c,))
    R = c * M if mode == 0 else M
    mu = np.empty(R)
    status = ctypes.c_int(0)
    if isinstance(want_sigma, str):
        if want_sigma != "diag":
            raise ValueError('want_sigma must be True, False or "diag"')
        var = np.empty(R)
        check(_lib.load().psoap_predictor_run_var(_predictor(), mode, c, N, M, dptr(lwls), dptr(fl), dptr(sigma),
                                                  dptr(pred), dptr(mu_c), dptr(gp), dptr(mu), dptr(var),
                                                  ctypes.byref(status)), "psoap_predictor_run_var")
        if status.value != 0:
            raise np.linalg.LinAlgError("data covariance matrix is not positive definite")
        return mu, var
    Sigma = np.empty((R, R)) if want_sigma else None
    check(_lib.load().psoap_predictor_run(_predictor(), mode, c, N, M, dptr(lwls), dptr(fl), dptr(sigma),
                                          dptr(pred), dptr(mu_c), dptr(gp), dptr(mu),
                                          None if Sigma is None else dptr(Sigma), ctypes.byref(status)),
          "psoap_predictor_run")
    if status.value != 0:
        # cho_factor raises here in the reference (covariance.py:113,182,222,292)
        raise np.linalg.LinAlgError("data covariance matrix is not positive definite")
    return (mu, Sigma) if want_sigma else mu


def predict_components_var(lwls, fl, sigma, lwls_predict, mus, gp):
    """Not in the reference: ``(mu, diag(Sigma))`` of ``predict_f`` / ``predict_f_g`` / ``predict_f_g_h`` (by the number
    of components) without forming ``Sigma`` -- all the retrieve scripts use of it is ``sqrt(diag(Sigma))``
    (scripts/psoap_retrieve_ST3.py:111-119).  ``lwls`` (c, N), ``lwls_predict`` (c, M), ``mus`` (c,), ``gp`` (2c,)."""
    return _predict(2 if len(lwls) == 1 else 0, lwls, fl, sigma, lwls_predict, mus, gp, want_sigma="diag")


def predict_f(lwl_known, fl_known, sigma_known, lwl_predict, amp_f, l_f, mu_GP=1.0):
    """Single-component conditional (covariance.py:25-54): mean ``mu_GP + V12^T V11^-1 (fl - mu_GP)``.  The reference
    body reads ``len(wl_predict)`` (:38), a name it does not define; with ``covariance.wl_predict = lwl_predict`` set as
    a module global it runs unmodified, and its values at several ``mu_GP`` are pinned
    (tests/golden/golden_predict_f_v1.npz).  This implements that ``N = len(lwl_predict)``."""
    return _predict(2, [lwl_known], fl_known, sigma_known, [lwl_predict], [mu_GP], [amp_f, l_f])


def predict_f_g(lwl_f, lwl_g, fl_fg, sigma_fg, lwl_f_predict, lwl_g_predict, mu_f, amp_f, l_f, mu_g, amp_g, l_g,
                get_Sigma=True):
    assert len(lwl_f) == len(lwl_g), "Input wavelengths must be the same length."
    assert len(lwl_f_predict) == len(lwl_g_predict), "Prediction wavelengths must be the same length."
    return _predict(0, [lwl_f, lwl_g], fl_fg, sigma_fg, [lwl_f_predict, lwl_g_predict], [mu_f, mu_g],
                    [amp_f, l_f, amp_g, l_g], want_sigma=bool(get_Sigma))


def predict_f_g_sum(lwl_f, lwl_g, fl_fg, sigma_fg, lwl_f_predict, lwl_g_predict, mu_fg, amp_f, l_f, amp_g, l_g):
    assert len(lwl_f) == len(lwl_g), "Input wavelengths must be the same length."
    return _predict(1, [lwl_f, lwl_g], fl_fg, sigma_fg, [lwl_f_predict, lwl_g_predict], [mu_fg],
                    [amp_f, l_f, amp_g, l_g])


def predict_f_g_h(lwl_f, lwl_g, lwl_h, fl_fgh, sigma_fgh, lwl_f_predict, lwl_g_predict, lwl_h_predict,
                  mu_f, mu_g, mu_h, amp_f, l_f, amp_g, l_g, amp_h, l_h):
    assert len(lwl_f) == len(lwl_g), "Input wavelengths must be the same length."
    assert len(lwl_f) == len(lwl_h), "Input wavelengths must be the same length."
    assert len(lwl_f_predict) == len(lwl_g_predict), "Prediction wavelengths must be the same length."
    assert len(lwl_f_predict) == len(lwl_h_predict), "Prediction wavelengths must be the same length."
    return _predict(0, [lwl_f, lwl_g, lwl_h], fl_fgh, sigma_fgh, [lwl_f_predict, lwl_g_predict, lwl_h_predict],
                    [mu_f, mu_g, mu_h], [amp_f, l_f, amp_g, l_g, amp_h, l_h])


def predict_f_g_h_sum(lwl_f, lwl_g, lwl_h, fl_fgh, sigma_fgh, lwl_f_predict, lwl_g_predict, lwl_h_predict,
                      mu_fgh, amp_f, l_f, amp_g, l_g, amp_h, l_h):
    assert len(lwl_f) == len(lwl_g), "Input wavelengths must be the same length."
    if len(lwl_f_predict) != len(lwl_f):
        # the reference fails here too: np.dot(V12.T, ...) at covariance.py:294 only conforms for M == N
        raise ValueError("shapes not aligned: predict_f_g_h_sum needs len(lwl_predict) == len(lwl) "
                         "(covariance.py:294)")
    return _predict(1, [lwl_f, lwl_g, lwl_h], fl_fgh, sigma_fgh, [lwl_f_predict, lwl_g_predict, lwl_h_predict],
                    [mu_fgh], [amp_f, l_f, amp_g, l_g, amp_h, l_h])


def optimize_GP_f(wl_known, fl_known, sigma_known, amp_f, l_f, mu_GP=1.0):
    """Nelder-Mead fit of the single-component hyper-parameters to one slice of data, starting from
    ``(amp_f, l_f)`` (covariance.py:405-422); every likelihood evaluation runs on the device."""
    from scipy.optimize import minimize
    V11 = None          # the reference passes an N x N scratch matrix; the device path ignores it

    def func(x):
        a, l = x
        return -lnlike_f(V11, wl_known, fl_known, sigma_known, a, l, mu_GP)

    return minimize(func, np.array([amp_f, l_f]), method="Nelder-Mead")["x"]


# ---- gradient of the likelihood (not in the reference) ----------------------------------------------
def lnlike_grad(lwls, fl, sigma, gp, mu_GP=1.0):
    """``(lnp, grad_gp (2c,), grad_lwl (c, N), grad_mu)``: the value of ``lnlike_f`` / ``lnlike_f_g`` / ``lnlike_f_g_h`` (by the
    number of rows of ``lwls``) and its analytic derivatives with respect to ``gp = (amp_0, l_0, ...)``, every rest-frame
    ln-wavelength and ``mu_GP``, evaluated on the device (``ChunkHandle.lnlike_grad``).

    Degenerate input follows ``_lnlike``: a negative hyper-parameter gives ``-inf`` with NaN gradients before any work,
    ``l == 0`` raises ``ZeroDivisionError``, a non-finite matrix raises ``ValueError``; a matrix that is not positive definite
    gives ``-inf`` with NaN gradients."""
    gp = [float(g) for g in gp]
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    if len(gp) != 2 * lw.shape[0]:
        raise ValueError(f"gp must hold {2 * lw.shape[0]} values for {lw.shape[0]} component(s)")
    if any(g < 0.0 for g in gp):
        return -np.inf, np.full(len(gp), np.nan), np.full(lw.shape, np.nan), np.nan
    if any(l == 0.0 for l in gp[1::2]):
        raise ZeroDivisionError("float division")
    if not _matrix_is_finite(lw, sigma, gp):
        raise ValueError(_NONFINITE)
    h = _chunk_for(fl, sigma)
    if not hasattr(h, "lnlike_grad"):
        raise _lib.PsoapError("lnlike_grad needs the device in this process (PSOAP_GPU_SERVER serves values only)")
    lnp, g_gp, g_lwl, g_mu = h.lnlike_grad(lw, gp, mu_GP)
    if not np.isneginf(lnp) and not (np.all(np.isfinite(np.asarray(fl, dtype=np.float64))) and np.isfinite(mu_GP)):
        raise ValueError(_NONFINITE)
    return np.float64(lnp), g_gp, g_lwl, np.float64(g_mu)


def fisher_information(lwls, fl, sigma, gp):
    """The ``(2c, 2c)`` Fisher information of the hyper-parameters ``(amp_0, l_0, amp_1, ...)`` of one chunk,
    ``F_st = 1/2 tr(K^-1 dK/dtheta_s K^-1 dK/dtheta_t)``, evaluated on the device (``ChunkHandle.fisher`` with unit
    tangents): its inverse is the Laplace covariance of an ``optimize_GP`` fit.  It does not depend on ``fl``, which only
    names the cached chunk, as for ``lnlike_grad``.  Degenerate input follows ``lnlike_grad``: a negative hyper-parameter
    or a matrix that is not positive definite gives NaN in every entry."""
    gp = [float(g) for g in gp]
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    if len(gp) != 2 * lw.shape[0]:
        raise ValueError(f"gp must hold {2 * lw.shape[0]} values for {lw.shape[0]} component(s)")
    if any(g < 0.0 for g in gp):
        return np.full((len(gp), len(gp)), np.nan)
    if any(l == 0.0 for l in gp[1::2]):
        raise ZeroDivisionError("float division")
    if not _matrix_is_finite(lw, sigma, gp):
        raise ValueError(_NONFINITE)
    h = _chunk_for(fl, sigma)
    if not hasattr(h, "fisher"):
        raise _lib.PsoapError("fisher_information needs the device in this process (PSOAP_GPU_SERVER serves values only)")
    return h.fisher(lw, gp, np.eye(len(gp)))


def loo(lwls, fl, sigma, gp, mu_GP=1.0, epoch_index=None):
    """Leave-one-out cross-validation of one chunk at ``gp = (amp_0, l_0, ...)``, evaluated on the device through the cached
    handle (``ChunkHandle.loo``): a ``chunk.LooResult`` with the prediction of every pixel from all the others and, with
    ``epoch_index`` (N,), of every epoch from all the other epochs.  Degenerate input follows ``lnlike_grad``: a negative
    hyper-parameter gives ``lnp = -inf`` and NaN before any work, ``l == 0`` raises ``ZeroDivisionError``, a non-finite matrix
    raises ``ValueError``; a matrix that is not positive definite gives ``-inf`` and NaN."""
    from .chunk import LooResult
    gp = [float(g) for g in gp]
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    if len(gp) != 2 * lw.shape[0]:
        raise ValueError(f"gp must hold {2 * lw.shape[0]} values for {lw.shape[0]} component(s)")
    ep = None if epoch_index is None else np.asarray(epoch_index, dtype=np.int64)
    if ep is not None and (ep.shape != lw.shape[1:] or (ep.size and ep.min() < 0)):
        raise ValueError("epoch_index must hold one non-negative epoch per pixel")
    if any(g < 0.0 for g in gp):
        return LooResult.degenerate(lw.shape[1], None if ep is None else np.bincount(ep))
    if any(l == 0.0 for l in gp[1::2]):
        raise ZeroDivisionError("float division")
    if not _matrix_is_finite(lw, sigma, gp):
        raise ValueError(_NONFINITE)
    h = _chunk_for(fl, sigma)
    if not hasattr(h, "loo"):
        raise _lib.PsoapError("loo needs the device in this process (PSOAP_GPU_SERVER serves values only)")
    res = h.loo(lw, gp, mu_GP, ep)
    if not np.isneginf(res.lnp) and not (np.all(np.isfinite(np.asarray(fl, dtype=np.float64))) and np.isfinite(mu_GP)):
        raise ValueError(_NONFINITE)
    return res


def _marginal(lwls, fl, sigma, gp, x, epoch_index, order, prior_sd, weight, mu_GP, full):
    """the shared front of ``lnlike_marginal`` and ``baseline_posterior``: the degenerate-input rules of ``lnlike_grad``, the
    cached handle of the chunk.  A sampler keeps a ``ChunkHandle`` / ``ChunkWorker`` and sets the baseline once."""
    gp = [float(g) for g in gp]
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    if len(gp) != 2 * lw.shape[0]:
        raise ValueError(f"gp must hold {2 * lw.shape[0]} values for {lw.shape[0]} component(s)")
    ep = np.asarray(epoch_index, dtype=np.int64)
    if ep.shape != lw.shape[1:] or (ep.size and ep.min() < 0):
        raise ValueError("epoch_index must hold one non-negative epoch per pixel")
    ne, N = int(ep.max()) + 1, lw.shape[1]
    q = ne * (int(order) + 1)
    nan = (np.full((ne, int(order) + 1), np.nan), np.full((q, q), np.nan), np.full(N, np.nan), -np.inf)
    if any(g < 0.0 for g in gp):
        return nan if full else -np.inf
    if any(l == 0.0 for l in gp[1::2]):
        raise ZeroDivisionError("float division")
    if not _matrix_is_finite(lw, sigma, gp):
        raise ValueError(_NONFINITE)
    h = _chunk_for(fl, sigma)
    if not hasattr(h, "lnlike_marg"):
        raise _lib.PsoapError("lnlike_marginal needs the device in this process (PSOAP_GPU_SERVER serves values only)")
    h.set_baseline(order, x, ep, ne, prior_sd, weight)      # (every call: the cached handle is shared by this module's callers)
    res = h.lnlike_marg(lw, gp, mu_GP, want_beta=full, want_cov=full, want_flux=full)
    lnp = res.lnp if full else res
    if not np.isneginf(lnp) and not (np.all(np.isfinite(np.asarray(fl, dtype=np.float64))) and np.isfinite(mu_GP)):
        raise ValueError(_NONFINITE)
    return (res.beta, res.beta_cov, res.fl_cor, np.float64(lnp)) if full else np.float64(lnp)


def lnlike_marginal(lwls, fl, sigma, gp, x, epoch_index, order, prior_sd, weight=None, mu_GP=1.0):
    """The likelihood of one chunk with a Chebyshev polynomial of degree ``order`` per epoch integrated out under the
    Gaussian prior ``prior_sd`` (order + 1,) -- ``lnlike_f`` / ``_f_g`` / ``_f_g_h`` by the rows of ``lwls``, under
    ``K + H Lambda H^T`` (``ChunkHandle.lnlike_marg``).  ``x`` (N,): observed-frame ln-wavelengths; ``epoch_index`` (N,);
    ``weight``: ``None`` (additive) or (N,), e.g. ``fl``.  ``-inf`` as ``lnlike``: a negative hyper-parameter, a matrix that is
    not positive definite."""
    return _marginal(lwls, fl, sigma, gp, x, epoch_index, order, prior_sd, weight, mu_GP, False)


def baseline_posterior(lwls, fl, sigma, gp, x, epoch_index, order, prior_sd, weight=None, mu_GP=1.0):
    """``(beta (n_epochs, order + 1), beta_cov (q, q), fl_cor (N,), lnp)`` at a fit: the posterior mean and covariance of every
    epoch's continuum coefficients, jointly, and the flux with the posterior-mean term removed -- the one-shot counterpart
    of ``cycle_calibration``, with error bars.  Arguments and ``-inf`` / NaN conventions as ``lnlike_marginal``."""
    return _marginal(lwls, fl, sigma, gp, x, epoch_index, order, prior_sd, weight, mu_GP, True)


def lnlike_marginal_grad(lwls, fl, sigma, gp, x, epoch_index, order, prior_sd, weight=None, mu_GP=1.0):
    """``(lnp, grad_gp (2c,), grad_lwl (c, N), grad_mu)``: the value of ``lnlike_marginal`` and its analytic derivatives with
    respect to ``gp``, every rest-frame ln-wavelength and ``mu_GP`` (``ChunkHandle.lnlike_marg_grad``; the basis does not
    depend on any of them, ``prior_sd`` has no derivative here).  Arguments as ``lnlike_marginal``; degenerate input as
    ``lnlike_grad``: ``-inf`` with NaN gradients."""
    gp = [float(g) for g in gp]
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    if len(gp) != 2 * lw.shape[0]:
        raise ValueError(f"gp must hold {2 * lw.shape[0]} values for {lw.shape[0]} component(s)")
    ep = np.asarray(epoch_index, dtype=np.int64)
    if ep.shape != lw.shape[1:] or (ep.size and ep.min() < 0):
        raise ValueError("epoch_index must hold one non-negative epoch per pixel")
    if any(g < 0.0 for g in gp):
        return -np.inf, np.full(len(gp), np.nan), np.full(lw.shape, np.nan), np.nan
    if any(l == 0.0 for l in gp[1::2]):
        raise ZeroDivisionError("float division")
    if not _matrix_is_finite(lw, sigma, gp):
        raise ValueError(_NONFINITE)
    h = _chunk_for(fl, sigma)
    if not hasattr(h, "lnlike_marg_grad"):
        raise _lib.PsoapError("lnlike_marginal_grad needs the device in this process (PSOAP_GPU_SERVER serves values only)")
    h.set_baseline(order, x, ep, int(ep.max()) + 1, prior_sd, weight)      # (every call, as ``_marginal``)
    lnp, g_gp, g_lwl, g_mu = h.lnlike_marg_grad(lw, gp, mu_GP)
    if not np.isneginf(lnp) and not (np.all(np.isfinite(np.asarray(fl, dtype=np.float64))) and np.isfinite(mu_GP)):
        raise ValueError(_NONFINITE)
    return np.float64(lnp), g_gp, g_lwl, np.float64(g_mu)


def _marginal_front(lwls, gp, epoch_index):
    """the shared front of ``fisher_information_marginal`` and ``loo_marginal``: shapes and the degenerate-input rules of
    ``lnlike_grad`` -> ``(gp, lw, ep, negative)``"""
    gp = [float(g) for g in gp]
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    if len(gp) != 2 * lw.shape[0]:
        raise ValueError(f"gp must hold {2 * lw.shape[0]} values for {lw.shape[0]} component(s)")
    ep = np.asarray(epoch_index, dtype=np.int64)
    if ep.shape != lw.shape[1:] or (ep.size and ep.min() < 0):
        raise ValueError("epoch_index must hold one non-negative epoch per pixel")
    negative = any(g < 0.0 for g in gp)
    if not negative and any(l == 0.0 for l in gp[1::2]):
        raise ZeroDivisionError("float division")
    return gp, lw, ep, negative


def fisher_information_marginal(lwls, fl, sigma, gp, x, epoch_index, order, prior_sd, weight=None):
    """``fisher_information`` under the baseline of ``lnlike_marginal``: the ``(2c, 2c)`` Fisher information of the
    hyper-parameters with ``K + H Lambda H^T`` in the place of ``K`` (``ChunkHandle.fisher_marg`` with unit tangents) -- its
    inverse is the Laplace covariance of an ``optimize_GP(..., baseline=...)`` fit.  Arguments as ``lnlike_marginal`` (``fl``
    names the cached chunk and is the weight of a multiplicative baseline); degenerate input as ``fisher_information``."""
    gp, lw, ep, negative = _marginal_front(lwls, gp, epoch_index)
    if negative:
        return np.full((len(gp), len(gp)), np.nan)
    if not _matrix_is_finite(lw, sigma, gp):
        raise ValueError(_NONFINITE)
    h = _chunk_for(fl, sigma)
    if not hasattr(h, "fisher_marg"):
        raise _lib.PsoapError("fisher_information_marginal needs the device in this process (PSOAP_GPU_SERVER serves values only)")
    h.set_baseline(order, x, ep, int(ep.max()) + 1, prior_sd, weight)      # (every call, as ``_marginal``)
    return h.fisher_marg(lw, gp, np.eye(len(gp)))


def loo_marginal(lwls, fl, sigma, gp, x, epoch_index, order, prior_sd, weight=None, mu_GP=1.0):
    """``loo`` under the baseline of ``lnlike_marginal`` (``ChunkHandle.loo_marg``): a ``chunk.LooResult`` with every pixel and
    every epoch of ``epoch_index`` predicted from the others under ``K + H Lambda H^T``, ``lnp`` the value of
    ``lnlike_marginal``.  Arguments as ``lnlike_marginal``; degenerate input as ``loo``."""
    from .chunk import LooResult
    gp, lw, ep, negative = _marginal_front(lwls, gp, epoch_index)
    if negative:
        return LooResult.degenerate(lw.shape[1], np.bincount(ep))
    if not _matrix_is_finite(lw, sigma, gp):
        raise ValueError(_NONFINITE)
    h = _chunk_for(fl, sigma)
    if not hasattr(h, "loo_marg"):
        raise _lib.PsoapError("loo_marginal needs the device in this process (PSOAP_GPU_SERVER serves values only)")
    h.set_baseline(order, x, ep, int(ep.max()) + 1, prior_sd, weight)      # (every call, as ``_marginal``)
    res = h.loo_marg(lw, gp, mu_GP, ep)
    if not np.isneginf(res.lnp) and not (np.all(np.isfinite(np.asarray(fl, dtype=np.float64))) and np.isfinite(mu_GP)):
        raise ValueError(_NONFINITE)
    return res


def predict_marginal(lwls, fl, sigma, lwls_predict, mus, gp, x, epoch_index, order, prior_sd, weight=None, mode=0,
                     want_sigma=True):
    """The component spectra of one chunk under the baseline of ``lnlike_marginal`` (``ChunkHandle.predict_marg``):
    ``predict_f`` / ``predict_f_g`` / ``predict_f_g_h`` (``mode`` 2 with one row of ``lwls``, else 0) or ``predict_f_g_sum``
    (``mode`` 1) with ``K + H Lambda H^T`` as the data covariance, so ``Sigma`` carries the continuum's uncertainty.
    ``lwls`` (c, N), ``lwls_predict`` (c, M), ``mus`` (c,) -- one value for modes 1 and 2 --, ``gp`` (2c,); the baseline
    arguments as ``lnlike_marginal``.  ``want_sigma``: True -> ``(mu, Sigma)``, ``"diag"`` -> ``(mu, diag(Sigma))``, False ->
    ``mu``.  ``LinAlgError`` where the plain predict raises it: a data covariance that is not positive definite."""
    gp, lw, ep, _negative = _marginal_front(lwls, gp, epoch_index)
    h = _chunk_for(fl, sigma)
    if not hasattr(h, "predict_marg"):
        raise _lib.PsoapError("predict_marginal needs the device in this process (PSOAP_GPU_SERVER serves values only)")
    h.set_baseline(order, x, ep, int(ep.max()) + 1, prior_sd, weight)      # (every call, as ``_marginal``)
    return h.predict_marg(int(mode), lw, np.stack([as_f64(w) for w in np.atleast_2d(lwls_predict)]), np.atleast_1d(mus), gp,
                          want_sigma)


def predict_draws(lwls, fl, sigma, lwls_predict, mus, gp, n_draws, seed, mode=0, nugget=1e-8, baseline=None,
                  want_sigma=True, timevar=None):
    """Not one function of the reference but the end of its reconstruction scripts (scripts/psoap_retrieve_SB2_draw.py,
    psoap_retrieve_ST3_draw.py, psoap_predict_*.py --draws: ``np.random.multivariate_normal(mu, Sigma, size=n_draws)``):
    the posterior of the component spectra and ``n_draws`` spectra drawn from it on the device, without an SVD of the
    downloaded ``Sigma`` on the host -> ``(mu, Sigma or None, draws)``, ``draws`` ``(n_draws, R)``.  The draws are from
    ``N(mu, Sigma + nugget I)`` (``ChunkHandle.predict_draw``: why the nugget is needed, what ``seed`` fixes).
    ``lwls`` (c, N), ``lwls_predict`` (c, M), ``mus`` (c,) -- one value for modes 1 and 2 --, ``gp`` (2c,); ``mode`` as
    ``ChunkHandle.predict``.  ``baseline``: a dictionary ``x``, ``epoch_index``, ``order``, ``prior_sd`` and optionally
    ``weight`` -- the arguments of ``predict_marginal``, whose posterior is then the one drawn from.  ``want_sigma=False``
    forms ``Sigma`` on the device all the same (the draws need it) and spares the download's copy to the caller.
    ``timevar``: a dictionary ``times``, ``tau``, ``t_predict`` -- the arguments of ``predict_timevar``, whose posterior is
    then the one drawn from: spectra at the dates ``t_predict`` (not together with ``baseline``)."""
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    pred = np.stack([as_f64(w) for w in np.atleast_2d(lwls_predict)])
    fl, sigma = as_f64(fl), as_f64(sigma)      # (once: the cache below is keyed on the buffers, and predict_marginal asks it again)
    h = _chunk_for(fl, sigma)
    if not hasattr(h, "predict_draw"):
        raise _lib.PsoapError("predict_draws needs the device in this process (PSOAP_GPU_SERVER serves values only)")
    if timevar is not None:
        if baseline is not None:
            raise ValueError("predict_draws takes a baseline or timevar, not both (the combination is not built)")
        if set(timevar) != {"times", "tau", "t_predict"}:
            raise ValueError(f"timevar needs 'times', 'tau' and 't_predict'; got {sorted(timevar)}")
        mu, Sigma = predict_timevar(lw, fl, sigma, pred, timevar["t_predict"], mus, gp, timevar["tau"], timevar["times"], mode=mode,
                                    want_sigma=True)
    elif baseline is None:
        mu, Sigma = h.predict(int(mode), lw, pred, np.atleast_1d(mus), as_f64(gp), True)
    else:
        unknown = set(baseline) - {"x", "epoch_index", "order", "prior_sd", "weight"}
        if unknown or not {"x", "epoch_index", "order", "prior_sd"} <= set(baseline):
            raise ValueError(f"baseline needs 'x', 'epoch_index', 'order' and 'prior_sd' (and optionally 'weight'); got {sorted(baseline)}")
        mu, Sigma = predict_marginal(lw, fl, sigma, pred, mus, gp, baseline["x"], baseline["epoch_index"], baseline["order"],
                                     baseline["prior_sd"], baseline.get("weight"), mode=mode, want_sigma=True)
    draws = h.predict_draw(n_draws, seed=seed, nugget=nugget)
    return mu, (Sigma if want_sigma else None), draws


def _baseline_args(baseline):
    unknown = set(baseline) - {"x", "epoch_index", "order", "prior_sd", "weight"}
    if unknown or not {"x", "epoch_index", "order", "prior_sd"} <= set(baseline):
        raise ValueError(f"baseline needs 'x', 'epoch_index', 'order' and 'prior_sd' (and optionally 'weight'); got {sorted(baseline)}")
    ep = np.asarray(baseline["epoch_index"], dtype=np.int64)
    return baseline["order"], baseline["x"], ep, int(ep.max()) + 1, baseline["prior_sd"], baseline.get("weight")


def predict_mixture(lwls_list, fl, sigma, lwls_predict, mus, gps, weights=None, mode=0, baseline=None, want_sigma=True,
                    draws_per_sample=0, seed=None, nugget=1e-8):
    """Not a function of the reference: the component spectra of one chunk marginalised over ``S`` samples of the orbit and
    the hyper-parameters (a thinned chain), by the law of total covariance with weights ``w_s``, ``W = sum w_s``:

        mu    = sum_s w_s mu_s / W
        Sigma = sum_s w_s Sigma_s / W  +  sum_s w_s (mu_s - mu)(mu_s - mu)^T / W          (within + between)

    ``(mu_s, Sigma_s)`` is what ``ChunkHandle.predict`` (``predict_marg`` with ``baseline``, the dictionary of
    ``predict_draws``) returns for sample ``s``; every sample is folded on the device through the chunk's cached handle
    (``ChunkHandle.mix_*``) and one ``mu`` and one ``Sigma`` are downloaded at the end.  ``lwls_list`` (S, c, N): the
    rest-frame grids of every sample; ``gps`` (S, 2c); ``lwls_predict`` (c, M) and ``mus``: ONE prediction grid and the
    prior means for all samples; ``weights`` (S,), default all one.  ``want_sigma=False`` accumulates variances only.
    Returns a dict: ``mu``, ``Sigma`` (or None), ``var_within``, ``var_between`` (``diag(Sigma)`` is their sum),
    ``n_folded``, ``skipped`` -- the indices of the samples whose data covariance was not positive definite; they are left
    out -- and, with ``draws_per_sample > 0`` (needs ``want_sigma`` and ``seed``), ``draws`` of shape
    ``(n_folded * draws_per_sample, R)``: draws from the mixture itself -- a parameter sample, then spectra from
    ``N(mu_s, Sigma_s + nugget I)`` with the generator's seed ``seed + s`` (``ChunkHandle.predict_draw``)."""
    lw = np.stack([np.stack([as_f64(w) for w in np.atleast_2d(l)]) for l in lwls_list])
    S, c = lw.shape[0], lw.shape[1]
    gps = as_f64(np.atleast_2d(gps), (S, 2 * c))
    w = np.ones(S) if weights is None else as_f64(weights, (S,))
    pred = np.stack([as_f64(p) for p in np.atleast_2d(lwls_predict)])
    n_draw = int(draws_per_sample)
    if n_draw > 0 and (seed is None or not want_sigma):
        raise ValueError("draws_per_sample > 0 needs a seed and want_sigma=True")
    fl, sigma = as_f64(fl), as_f64(sigma)
    h = _chunk_for(fl, sigma)
    if not hasattr(h, "mix_begin"):
        raise _lib.PsoapError("predict_mixture needs the device in this process (PSOAP_GPU_SERVER serves values only)")
    if baseline is not None:
        h.set_baseline(*_baseline_args(baseline))
    h.mix_begin(int(mode), pred, np.atleast_1d(mus), S, want_sigma=bool(want_sigma), marg=baseline is not None)
    skipped, draws = [], []
    try:
        for s in range(S):
            if not h.mix_add(lw[s], gps[s], w[s]):
                skipped.append(s)
            elif n_draw > 0:
                draws.append(h.predict_draw(n_draw, seed=int(seed) + s, nugget=nugget))
        out = h.mix_finish()
    finally:
        h.mix_release()
    del out["W"]
    out["skipped"] = skipped
    if n_draw > 0:
        out["draws"] = np.concatenate(draws, axis=0)
    return out


def velocity_gradient(grad_lwl, epoch_index, n_epochs):
    """``dlnL/dv[c, e]`` from ``dlnL/dlwl[c, i]``: the rest-frame grids are ``lwl - v[c, epoch]/c_kms``
    (``data.replicate_wls``), so ``dlnL/dv[c, e] = -(1/c_kms) sum_{i in epoch e} dlnL/dlwl[c, i]``.
    ``grad_lwl`` (c, N) or (B, c, N); ``epoch_index`` (N,) as from ``data.epoch_index_of``; -> (c, n_epochs) or (B, c, n_epochs)."""
    from .data import c_kms
    g = np.asarray(grad_lwl, dtype=np.float64)
    ep = np.asarray(epoch_index)
    if ep.shape != g.shape[-1:]:
        raise ValueError("epoch_index must have one entry per pixel")
    if ep.size and (ep.min() < 0 or ep.max() >= n_epochs):
        raise ValueError("epoch index out of range")
    flat = g.reshape(-1, g.shape[-1])
    out = np.zeros((flat.shape[0], int(n_epochs)))
    for k, row in enumerate(flat):
        out[k] = np.bincount(ep, weights=row, minlength=int(n_epochs))
    return (-out / c_kms).reshape(g.shape[:-1] + (int(n_epochs),))


def velocity_information(lwls, fl, sigma, gp, epoch_index):
    """The ``(c E, c E)`` Fisher information of the per-epoch radial velocities ``v[c, e]`` of one chunk, row ``c * E + e``
    (the order of ``velocity_gradient``, ``E = max(epoch_index) + 1``), evaluated on the device through the cached handle
    (``ChunkHandle.fisher_vel``): the second-order half of ``velocity_gradient``, free of any orbit model.  It is the
    information AT FIXED hyper-parameters and has ``c`` null directions, the constant shift of each component: velocities
    are determined up to one offset per component.  It does not depend on ``fl``, which only names the cached chunk.
    Degenerate input follows ``fisher_information``: a negative hyper-parameter or a matrix that is not positive definite
    gives NaN in every entry."""
    gp = [float(g) for g in gp]
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    if len(gp) != 2 * lw.shape[0]:
        raise ValueError(f"gp must hold {2 * lw.shape[0]} values for {lw.shape[0]} component(s)")
    ep = np.asarray(epoch_index, dtype=np.int64)
    if ep.shape != lw.shape[1:] or ep.size == 0 or ep.min() < 0:
        raise ValueError("epoch_index must hold one non-negative epoch per pixel")
    T = lw.shape[0] * (int(ep.max()) + 1)
    if any(g < 0.0 for g in gp):
        return np.full((T, T), np.nan)
    if any(l == 0.0 for l in gp[1::2]):
        raise ZeroDivisionError("float division")
    if not _matrix_is_finite(lw, sigma, gp):
        raise ValueError(_NONFINITE)
    h = _chunk_for(fl, sigma)
    if not hasattr(h, "fisher_vel"):
        raise _lib.PsoapError("velocity_information needs the device in this process (PSOAP_GPU_SERVER serves values only)")
    return h.fisher_vel(lw, gp, ep)


def velocity_information_observed(lwls, fl, sigma, gp, epoch_index, mu_GP=1.0, baseline=None):
    """``(lnp, grad (c, E), F, J)`` of one chunk from one factorisation on the device (``ChunkHandle.info_vel``): the value,
    ``velocity_gradient``, ``velocity_information`` and the OBSERVED information ``J = -d2 lnL / dv dv`` at the flux ``fl``,
    of which ``F`` is the expectation -- the curvature a Newton step and an error bar at the data want.  Rows as
    ``velocity_information``; ``J`` has the same ``c`` null directions and is symmetric bit for bit.  ``baseline`` (the dict
    of ``lnlike_marg``): everything under the marginalised continuum.  A negative hyper-parameter or a matrix that is not
    positive definite gives ``-inf`` and NaN in every entry."""
    gp = [float(g) for g in gp]
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    if len(gp) != 2 * lw.shape[0]:
        raise ValueError(f"gp must hold {2 * lw.shape[0]} values for {lw.shape[0]} component(s)")
    ep = np.asarray(epoch_index, dtype=np.int64)
    if ep.shape != lw.shape[1:] or ep.size == 0 or ep.min() < 0:
        raise ValueError("epoch_index must hold one non-negative epoch per pixel")
    c, E = lw.shape[0], int(ep.max()) + 1
    if any(g < 0.0 for g in gp):
        return -np.inf, np.full((c, E), np.nan), np.full((c * E, c * E), np.nan), np.full((c * E, c * E), np.nan)
    if any(l == 0.0 for l in gp[1::2]):
        raise ZeroDivisionError("float division")
    if not _matrix_is_finite(lw, sigma, gp):
        raise ValueError(_NONFINITE)
    h = _chunk_for(fl, sigma)
    if not hasattr(h, "info_vel"):
        raise _lib.PsoapError("velocity_information_observed needs the device in this process (PSOAP_GPU_SERVER serves values only)")
    if baseline is not None:
        h.set_baseline(*_baseline_args(baseline))
    return h.info_vel(lw, gp, ep, E, mu_GP, marg=baseline is not None)


GP_LOWER_BOUND = 1e-6       # optimize_GP keeps every amplitude and length scale at or above this


def optimize_GP(lwls, fl, sigma, gp0, mu_GP=1.0, ftol=1e-10, full_output=False, baseline=None):
    """L-BFGS-B fit of the ``2c`` hyper-parameters ``(amp_0, l_0, ...)`` to one chunk from ``gp0``, with the analytic
    gradient (``lnlike_grad``, ``jac=True``) and every parameter bounded below at ``GP_LOWER_BOUND``.  Returns the fitted
    vector, or SciPy's whole result with ``full_output`` (``-result.fun`` is the likelihood reached, ``result.jac`` the
    gradient of ``-lnL`` there).  ``optimize_GP_f`` is the reference's derivative-free fit.

    ``baseline = dict(x=, epoch_index=, order=, prior_sd=, weight=)`` (``weight`` optional): the objective is the likelihood
    with that per-epoch continuum integrated out (``lnlike_marginal_grad``), so no frozen calibration has to come first."""
    from scipy.optimize import minimize
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    x0 = np.maximum(as_f64(gp0, (2 * lw.shape[0],)), GP_LOWER_BOUND)
    if baseline is not None:
        unknown = set(baseline) - {"x", "epoch_index", "order", "prior_sd", "weight"}
        if unknown or not {"x", "epoch_index", "order", "prior_sd"} <= set(baseline):
            raise ValueError(f"baseline needs 'x', 'epoch_index', 'order' and 'prior_sd' (and optionally 'weight'); got {sorted(baseline)}")

    def func(x):
        if baseline is None:
            lnp, g_gp, _g_lwl, _g_mu = lnlike_grad(lw, fl, sigma, x, mu_GP)
        else:
            lnp, g_gp, _g_lwl, _g_mu = lnlike_marginal_grad(lw, fl, sigma, x, baseline["x"], baseline["epoch_index"],
                                                            baseline["order"], baseline["prior_sd"], baseline.get("weight"), mu_GP)
        if not np.isfinite(lnp):
            return np.inf, np.zeros_like(x)
        return -lnp, -g_gp

    res = minimize(func, x0, jac=True, method="L-BFGS-B", bounds=[(GP_LOWER_BOUND, None)] * x0.size,
                   options={"ftol": ftol})
    return res if full_output else res["x"]


# ---- time-variable component spectra (not in the reference) ------------------------------------
def _timevar(lwls, fl, sigma, gp, tau, times, mu_GP, want_grad, baseline=None):
    """the front of ``lnlike_timevar`` and ``lnlike_timevar_grad``: the degenerate input of ``lnlike_grad``, ``tau <= 0`` or NaN
    like a negative hyper-parameter, the cached handle with ``times - min(times)`` on it; with ``baseline`` that baseline on
    the handle as well and the entries under it (``ChunkHandle.lnlike_marg_tv`` / ``lnlike_marg_tv_grad``)"""
    base = None if baseline is None else _baseline_args(baseline)
    gp = [float(g) for g in gp]
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    c, N = lw.shape
    if len(gp) != 2 * c:
        raise ValueError(f"gp must hold {2 * c} values for {c} component(s)")
    tau = as_f64(np.atleast_1d(as_f64(tau)), (c,))
    t = as_f64(times, (N,))
    if not np.all(np.isfinite(t)):
        raise ValueError(_NONFINITE)
    if any(g < 0.0 for g in gp) or not np.all(tau > 0.0):
        if not want_grad:
            return -np.inf
        return -np.inf, np.full(len(gp), np.nan), np.full(c, np.nan), np.full(lw.shape, np.nan), np.nan
    if any(l == 0.0 for l in gp[1::2]):
        raise ZeroDivisionError("float division")
    if not _matrix_is_finite(lw, sigma, gp):
        raise ValueError(_NONFINITE)
    h = _chunk_for(fl, sigma) if base is not None else _chunk_without_baseline(fl, sigma)
    if not hasattr(h, "lnlike_tv_grad"):
        raise _lib.PsoapError("lnlike_timevar needs the device in this process (PSOAP_GPU_SERVER serves the static likelihood only)")
    t = t - t.min()
    if getattr(h, "_tv_times", None) is None or not np.array_equal(h._tv_times, t):
        h.set_times(t)
        h._tv_times = t
    if base is None:
        res = h.lnlike_tv_grad(lw, gp, tau, mu_GP) if want_grad else (h.lnlike_tv(lw, gp, tau, mu_GP),)
    else:
        h.set_baseline(*base)      # (every call, as ``_marginal``: the cached handle is shared by this module's callers)
        res = h.lnlike_marg_tv_grad(lw, gp, tau, mu_GP) if want_grad else (h.lnlike_marg_tv(lw, gp, tau, mu_GP),)
    if not np.isneginf(res[0]) and not (np.all(np.isfinite(np.asarray(fl, dtype=np.float64))) and np.isfinite(mu_GP)):
        raise ValueError(_NONFINITE)
    if not want_grad:
        return np.float64(res[0])
    return np.float64(res[0]), res[1], res[2], res[3], np.float64(res[4])


def lnlike_timevar(lwls, fl, sigma, gp, tau, times, mu_GP=1.0):
    """The likelihood under time-variable component spectra: each component's kernel in ln-wavelength times a squared
    exponential in observation time, ``K_ij = sum_c a_c^2 exp(p_c d_cij^2 - (t_j - t_i)^2 / (2 tau_c^2)) + sigma_i^2 delta_ij``.
    ``tau`` (c,) in the unit of ``times`` (days); ``tau_c = inf`` keeps component c static, and with every ``tau = inf`` this is
    ``lnlike_f`` / ``_f_g`` / ``_f_g_h``.  ``times`` (N,): the observation time of every pixel -- ``dates[epoch_index]`` -- in
    any order; their minimum is subtracted before they go to the device.  ``tau <= 0`` or NaN gives ``-inf``; other
    degenerate input follows ``lnlike_grad``."""
    return _timevar(lwls, fl, sigma, gp, tau, times, mu_GP, False)


def lnlike_timevar_marginal(lwls, fl, sigma, gp, tau, times, baseline, mu_GP=1.0):
    """``lnlike_timevar`` with a per-epoch continuum integrated out under the same kernel, ``K_tv + H Lambda H^T``
    (``ChunkHandle.lnlike_marg_tv``).  ``baseline``: the dict of ``optimize_GP`` -- ``x``, ``epoch_index``, ``order``,
    ``prior_sd`` and optionally ``weight``.  With every ``tau = inf`` this is ``lnlike_marginal``.  (A function of its own:
    the parameter list of ``lnlike_timevar`` is fixed.)  Calls with and without a baseline on the same ``(fl, sigma)`` may
    alternate -- the variability statistic with the baseline on and off: the cached handle is made again where a call without
    one finds a baseline on it."""
    _baseline_args(baseline)
    return _timevar(lwls, fl, sigma, gp, tau, times, mu_GP, False, baseline)


def lnlike_timevar_grad(lwls, fl, sigma, gp, tau, times, mu_GP=1.0, baseline=None):
    """``(lnp, grad_gp (2c,), grad_tau (c,), grad_lwl (c, N), grad_mu)``: ``lnlike_timevar`` and its analytic derivatives on the
    device (``ChunkHandle.lnlike_tv_grad``; with ``baseline``, as ``lnlike_timevar_marginal`` takes it, ``lnlike_marg_tv_grad``).
    ``grad_tau`` is exactly 0 where ``tau = inf``."""
    return _timevar(lwls, fl, sigma, gp, tau, times, mu_GP, True, baseline)


def _timevar_handle(fl, sigma, times, N, who, baseline=False):
    """the cached handle of ``(fl, sigma)`` with ``times - min(times)`` on it, as ``lnlike_timevar`` leaves it -> (h, min(times));
    unless the caller is about to set a ``baseline``, a handle without one (``_chunk_without_baseline``)"""
    t = as_f64(times, (N,))
    if not np.all(np.isfinite(t)):
        raise ValueError(_NONFINITE)
    h = _chunk_for(fl, sigma) if baseline else _chunk_without_baseline(fl, sigma)
    if not hasattr(h, "predict_tv"):
        raise _lib.PsoapError(f"{who} needs the device in this process (PSOAP_GPU_SERVER serves the static likelihood only)")
    t0 = t.min()
    t = t - t0
    if getattr(h, "_tv_times", None) is None or not np.array_equal(h._tv_times, t):
        h.set_times(t)
        h._tv_times = t
    return h, t0


def predict_timevar(lwls, fl, sigma, lwls_predict, t_predict, mus, gp, tau, times, mode=0, want_sigma=True):
    """The component spectra of one chunk at chosen dates under the time-variable kernel of ``lnlike_timevar``
    (``ChunkHandle.predict_tv``): ``predict_f`` / ``predict_f_g`` / ``predict_f_g_h`` (``mode`` 2 with one row of ``lwls``, else
    0) or ``predict_f_g_sum`` (``mode`` 1) with the temporal factor in the data covariance, the cross-covariance and the prior.
    ``lwls`` (c, N), ``times`` (N,) the pixels' observation times; ``lwls_predict`` (c, M) with ``t_predict`` (M,), the date of
    every prediction point in the unit and from the origin of ``times`` (the minimum of ``times`` is taken off both before they
    go to the device) -- several dates are several runs, the grid repeated, and ``Sigma`` then holds the covariance between the
    dates; ``mus`` (c,) -- one value for modes 1 and 2 --, ``gp`` (2c,), ``tau`` (c,) with ``inf`` for a static component.
    ``want_sigma``: True -> ``(mu, Sigma)``, ``"diag"`` -> ``(mu, diag(Sigma))``, False -> ``mu``.  ``LinAlgError`` where the
    plain predict raises it; a ``tau <= 0`` or NaN and a ``t_predict`` that is not finite are refused (``PsoapError``)."""
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    pred = np.stack([as_f64(w) for w in np.atleast_2d(lwls_predict)])
    h, t0 = _timevar_handle(fl, sigma, times, lw.shape[1], "predict_timevar")
    t_pred = as_f64(np.atleast_1d(as_f64(t_predict)), (pred.shape[1],)) - t0
    return h.predict_tv(int(mode), lw, pred, t_pred, np.atleast_1d(mus), as_f64(gp), tau, want_sigma)


def optimize_GP_timevar(lwls, fl, sigma, gp0, tau0, times, free_tau=None, mu_GP=1.0, ftol=1e-10, full_output=False):
    """L-BFGS-B fit of the hyper-parameters and time scales of ``lnlike_timevar`` from ``(gp0, tau0)``, on the device gradient,
    in ``log amp``, ``log l`` and ``log tau``.  ``free_tau`` (c,) of booleans (default: every finite ``tau0``): a component left
    out keeps its ``tau0``, and ``inf`` is allowed there -- a free one must start finite.  Amplitudes and length scales stay at
    or above ``GP_LOWER_BOUND``.  Returns ``(gp, tau)``; with ``full_output`` ``(gp, tau, lnp, lnp_static, result)``:
    the likelihood reached, the likelihood at the same ``gp`` with every ``tau = inf``, and SciPy's result.
    ``lnp - lnp_static`` is the variability statistic: what the time-variable kernel gains over the static one."""
    return _optimize_timevar(lwls, fl, sigma, gp0, tau0, times, free_tau, mu_GP, ftol, full_output, None)


def optimize_GP_timevar_marginal(lwls, fl, sigma, gp0, tau0, times, baseline, free_tau=None, mu_GP=1.0, ftol=1e-10,
                                 full_output=False):
    """``optimize_GP_timevar`` under a baseline (the dict of ``optimize_GP``): the objective is the likelihood with that
    per-epoch continuum integrated out (``lnlike_timevar_grad(..., baseline=...)``), and ``lnp_static`` the marginal
    likelihood at ``tau = inf`` -- the statistic compares like with like, and a continuum error from epoch to epoch is no
    longer there for a finite ``tau`` to absorb.  (A function of its own: the parameter list of ``optimize_GP_timevar`` is
    fixed.)  ``timevar_laplace(..., baseline=...)`` gives the error bars of the fit."""
    _baseline_args(baseline)
    return _optimize_timevar(lwls, fl, sigma, gp0, tau0, times, free_tau, mu_GP, ftol, full_output, baseline)


def _optimize_timevar(lwls, fl, sigma, gp0, tau0, times, free_tau, mu_GP, ftol, full_output, baseline):
    """the body of ``optimize_GP_timevar`` (``baseline`` None) and ``optimize_GP_timevar_marginal``"""
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    c = lw.shape[0]

    def value_grad(gp, tau):
        lnp, g_gp, g_tau, _g_lwl, _g_mu = lnlike_timevar_grad(lw, fl, sigma, gp, tau, times, mu_GP, baseline)
        return lnp, g_gp, g_tau

    gp, tau, res = _fit_timevar(value_grad, c, gp0, tau0, free_tau, ftol)
    if not full_output:
        return gp, tau
    lnp_static = _timevar(lw, fl, sigma, gp, np.full(c, np.inf), times, mu_GP, False, baseline)
    return gp, tau, -float(res["fun"]), float(lnp_static), res


def _fit_timevar(value_grad, c, gp0, tau0, free_tau, ftol):
    """The driver of ``optimize_GP_timevar``: L-BFGS-B over ``x = (log gp, log tau[free])`` on ``value_grad(gp, tau) -> (lnp,
    grad_gp, grad_tau)`` -> ``(gp, tau, SciPy's result)``.  (Apart from ``value_grad`` nothing here knows the device: the
    tests run the same driver on the float64 CPU evaluation.)"""
    from scipy.optimize import minimize
    g0 = np.maximum(as_f64(gp0, (2 * c,)), GP_LOWER_BOUND)
    t0 = as_f64(np.atleast_1d(as_f64(tau0)), (c,)).copy()
    free = np.isfinite(t0) if free_tau is None else np.asarray(free_tau, dtype=bool).reshape(c)
    if not np.all(t0 > 0.0) or not np.all(np.isfinite(t0[free])):
        raise ValueError("tau0 must be positive, and finite where free_tau is set")

    def unpack(x):
        tau = t0.copy()
        tau[free] = np.exp(x[2 * c:])
        return np.exp(x[:2 * c]), tau

    def func(x):
        gp, tau = unpack(x)
        lnp, g_gp, g_tau = value_grad(gp, tau)
        if not np.isfinite(lnp):
            return np.inf, np.zeros_like(x)
        return -lnp, -np.concatenate([g_gp * gp, g_tau[free] * tau[free]])       # d/dlog theta = theta d/dtheta

    x0 = np.concatenate([np.log(g0), np.log(t0[free])])
    bounds = [(np.log(GP_LOWER_BOUND), None)] * (2 * c) + [(None, None)] * int(free.sum())
    res = minimize(func, x0, jac=True, method="L-BFGS-B", bounds=bounds, options={"ftol": ftol})
    gp, tau = unpack(res["x"])
    return gp, tau, res


# ---- quasi-periodic temporal factor (not in the reference) -------------------------------------
def _quasiperiodic(lwls, fl, sigma, gp, tau, gamma, period, times, mu_GP, want_grad):
    """the front of ``lnlike_quasiperiodic`` and ``lnlike_quasiperiodic_grad``: ``_timevar``'s checks with ``gamma < 0``, NaN or
    inf and ``period <= 0``, NaN or inf beside ``tau <= 0`` or NaN, then the cached handle with ``times - min(times)`` on it"""
    gp = [float(g) for g in gp]
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    c, N = lw.shape
    if len(gp) != 2 * c:
        raise ValueError(f"gp must hold {2 * c} values for {c} component(s)")
    tau, gamma, period = (as_f64(np.atleast_1d(as_f64(v)), (c,)) for v in (tau, gamma, period))
    t = as_f64(times, (N,))
    if not np.all(np.isfinite(t)):
        raise ValueError(_NONFINITE)
    if any(g < 0.0 for g in gp) or not _quasiperiodic_valid(tau, gamma, period):
        if not want_grad:
            return -np.inf
        nan_c = np.full(c, np.nan)
        return -np.inf, np.full(len(gp), np.nan), nan_c, nan_c.copy(), nan_c.copy(), np.full(lw.shape, np.nan), np.nan
    _quasiperiodic_input(lw, sigma, gp)
    h = _quasiperiodic_handle(fl, sigma, t, "lnlike_quasiperiodic")
    res = h.lnlike_qp_grad(lw, gp, tau, gamma, period, mu_GP) if want_grad else (h.lnlike_qp(lw, gp, tau, gamma, period, mu_GP),)
    if not np.isneginf(res[0]) and not (np.all(np.isfinite(np.asarray(fl, dtype=np.float64))) and np.isfinite(mu_GP)):
        raise ValueError(_NONFINITE)
    if not want_grad:
        return np.float64(res[0])
    return (np.float64(res[0]),) + tuple(res[1:6]) + (np.float64(res[6]),)


def _quasiperiodic_valid(tau, gamma, period):
    """every tau is a time scale, every gamma finite and not negative, every period positive and finite with a finite
    reciprocal (qp_refused of psoap_amd/csrc/qp_plan.hpp); any shape"""
    tau, gamma, period = (np.asarray(v, dtype=np.float64) for v in (tau, gamma, period))
    with np.errstate(all="ignore"):
        return bool(np.all(tau > 0.0) and np.all((gamma >= 0.0) & np.isfinite(gamma)) and
                    np.all((period > 0.0) & np.isfinite(period) & np.isfinite(1.0 / period)))


def _quasiperiodic_input(lw, sigma, gp):
    """the input that ``lnlike_grad`` refuses with an exception, refused the same way: a zero length scale, a matrix that is
    not finite"""
    if any(l == 0.0 for l in gp[1::2]):
        raise ZeroDivisionError("float division")
    if not _matrix_is_finite(lw, sigma, gp):
        raise ValueError(_NONFINITE)


def _quasiperiodic_handle(fl, sigma, t, who):
    """the cached handle of ``(fl, sigma)`` without a baseline and with ``t - min(t)`` on it (``_timevar``'s bookkeeping)"""
    h = _chunk_without_baseline(fl, sigma)
    if not hasattr(h, "lnlike_qp_grad"):
        raise _lib.PsoapError(f"{who} needs the device in this process (PSOAP_GPU_SERVER serves the static likelihood only)")
    t = t - t.min()
    if getattr(h, "_tv_times", None) is None or not np.array_equal(h._tv_times, t):
        h.set_times(t)
        h._tv_times = t
    return h


def lnlike_quasiperiodic(lwls, fl, sigma, gp, tau, gamma, period, times, mu_GP=1.0):
    """The likelihood under quasi-periodic component spectra: ``lnlike_timevar``'s kernel times a periodic factor,
    ``K_ij = sum_c a_c^2 exp(p_c d_cij^2 - dt_ij^2 / (2 tau_c^2) - gamma_c sin^2(pi dt_ij / period_c)) + sigma_i^2 delta_ij``.
    ``gamma`` (c,) is dimensionless, ``period`` (c,) in the unit of ``times``.  ``gamma_c = 0`` is ``lnlike_timevar`` bit for
    bit whatever the period; ``tau_c = inf`` with ``gamma_c > 0`` is a purely periodic component.  ``gamma < 0``, NaN or inf,
    ``period <= 0``, NaN or inf and ``tau <= 0`` or NaN give ``-inf``; other degenerate input follows ``lnlike_timevar``."""
    return _quasiperiodic(lwls, fl, sigma, gp, tau, gamma, period, times, mu_GP, False)


def lnlike_quasiperiodic_grad(lwls, fl, sigma, gp, tau, gamma, period, times, mu_GP=1.0):
    """``(lnp, grad_gp (2c,), grad_tau (c,), grad_gamma (c,), grad_period (c,), grad_lwl (c, N), grad_mu)``:
    ``lnlike_quasiperiodic`` and its analytic derivatives on the device (``ChunkHandle.lnlike_qp_grad``).  ``grad_period`` is
    exactly 0 where ``gamma = 0``; ``grad_gamma`` there is the score of a test for periodicity at that period."""
    return _quasiperiodic(lwls, fl, sigma, gp, tau, gamma, period, times, mu_GP, True)


def default_period_bounds(times):
    """``(twice the smallest positive separation of two epochs, the span)`` of ``times``: shorter periods are not sampled,
    longer ones are not covered once"""
    t = np.unique(as_f64(times))
    if t.shape[0] < 2:
        raise ValueError("period bounds need at least two different times")
    return 2.0 * float(np.diff(t).min()), float(t[-1] - t[0])


def optimize_GP_quasiperiodic(lwls, fl, sigma, gp0, tau0, gamma0, period0, times, free=None, period_bounds=None, mu_GP=1.0,
                              ftol=1e-10, full_output=False):
    """L-BFGS-B fit of ``lnlike_quasiperiodic`` from ``(gp0, tau0, gamma0, period0)`` on the device gradient, in the logarithm
    of every parameter (``_fit_timevar``'s pattern).  ``free``: a dictionary of (c,) booleans under ``"tau"``, ``"gamma"`` and
    ``"period"``; the defaults are every finite ``tau0`` and, for both others, every ``gamma0 > 0``.  A free ``gamma`` must
    start positive.  ``period_bounds`` ``(lo, hi)`` hold every free period; ``None``: ``default_period_bounds(times)``.
    Returns ``(gp, tau, gamma, period)``; with ``full_output`` ``(gp, tau, gamma, period, lnp, lnp_gamma0, lnp_timevar,
    result)``: the likelihood reached, the likelihood at ``gamma = 0`` on the same ``(gp, tau)``, and the likelihood of the
    time-variable model re-fitted from there (``_fit_timevar`` at ``gamma = 0``).  ``lnp - lnp_timevar`` is the periodicity
    statistic: what the periodic factor gains over the best time-variable fit."""
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    c = lw.shape[0]
    if period_bounds is None:
        period_bounds = default_period_bounds(times)

    def value_grad(gp, tau, gamma, period):
        return lnlike_quasiperiodic_grad(lw, fl, sigma, gp, tau, gamma, period, times, mu_GP)[:5]

    gp, tau, gamma, period, res = _fit_quasiperiodic(value_grad, c, gp0, tau0, gamma0, period0, free, period_bounds, ftol)
    if not full_output:
        return gp, tau, gamma, period
    free_tau = None if free is None or "tau" not in free else free["tau"]
    lnp_gamma0, lnp_tv = _quasiperiodic_null(value_grad, c, gp, tau, free_tau, ftol)
    return gp, tau, gamma, period, -float(res["fun"]), lnp_gamma0, lnp_tv, res


def _fit_quasiperiodic(value_grad, c, gp0, tau0, gamma0, period0, free, period_bounds, ftol):
    """The driver of ``optimize_GP_quasiperiodic``: L-BFGS-B over ``x = (log gp, log tau[free], log gamma[free], log
    period[free])`` on ``value_grad(gp, tau, gamma, period) -> (lnp, grad_gp, grad_tau, grad_gamma, grad_period)`` ->
    ``(gp, tau, gamma, period, SciPy's result)``.  (Nothing here knows the device: the tests run it on the float64 twin.)"""
    from scipy.optimize import minimize
    g0 = np.maximum(as_f64(gp0, (2 * c,)), GP_LOWER_BOUND)
    t0, m0, p0 = (as_f64(np.atleast_1d(as_f64(v)), (c,)).copy() for v in (tau0, gamma0, period0))
    free = {} if free is None else dict(free)
    if set(free) - {"tau", "gamma", "period"}:
        raise ValueError(f"free takes 'tau', 'gamma' and 'period'; got {sorted(free)}")
    f_t = np.asarray(free.get("tau", np.isfinite(t0)), dtype=bool).reshape(c)
    f_m = np.asarray(free.get("gamma", m0 > 0.0), dtype=bool).reshape(c)
    f_p = np.asarray(free.get("period", m0 > 0.0), dtype=bool).reshape(c)
    if not np.all(t0 > 0.0) or not np.all(np.isfinite(t0[f_t])):
        raise ValueError("tau0 must be positive, and finite where free['tau'] is set")
    if not np.all((m0 >= 0.0) & np.isfinite(m0)) or not np.all(m0[f_m] > 0.0):
        raise ValueError("gamma0 must be finite and not negative, and positive where free['gamma'] is set")
    if not np.all((p0 > 0.0) & np.isfinite(p0)):
        raise ValueError("period0 must be positive and finite")
    lo, hi = float(period_bounds[0]), float(period_bounds[1])
    if not (0.0 < lo < hi) or not np.all((p0[f_p] >= lo) & (p0[f_p] <= hi)):
        raise ValueError("period_bounds must be 0 < lo < hi and hold every free period0")
    n_t, n_m = int(f_t.sum()), int(f_m.sum())

    def unpack(x):
        tau, gamma, period = t0.copy(), m0.copy(), p0.copy()
        tau[f_t] = np.exp(x[2 * c:2 * c + n_t])
        gamma[f_m] = np.exp(x[2 * c + n_t:2 * c + n_t + n_m])
        period[f_p] = np.exp(x[2 * c + n_t + n_m:])
        return np.exp(x[:2 * c]), tau, gamma, period

    def func(x):
        gp, tau, gamma, period = unpack(x)
        lnp, g_gp, g_tau, g_gamma, g_period = value_grad(gp, tau, gamma, period)
        if not np.isfinite(lnp):
            return np.inf, np.zeros_like(x)
        return -lnp, -np.concatenate([g_gp * gp, g_tau[f_t] * tau[f_t], g_gamma[f_m] * gamma[f_m], g_period[f_p] * period[f_p]])

    x0 = np.concatenate([np.log(g0), np.log(t0[f_t]), np.log(m0[f_m]), np.log(p0[f_p])])
    bounds = [(np.log(GP_LOWER_BOUND), None)] * (2 * c) + [(None, None)] * (n_t + n_m) + [(np.log(lo), np.log(hi))] * int(f_p.sum())
    res = minimize(func, x0, jac=True, method="L-BFGS-B", bounds=bounds, options={"ftol": ftol})
    gp, tau, gamma, period = unpack(res["x"])
    return gp, tau, gamma, period, res


def _quasiperiodic_null(value_grad, c, gp, tau, free_tau, ftol):
    """The two ``gamma = 0`` values of ``optimize_GP_quasiperiodic`` on ``value_grad`` (the driver's): ``lnp`` at ``(gp, tau)``
    as they are, and the maximum ``_fit_timevar`` reaches from there -> ``(lnp_gamma0, lnp_timevar)``"""
    zero, one = np.zeros(c), np.ones(c)

    def null(gp_, tau_):
        return value_grad(gp_, tau_, zero, one)[:3]

    lnp_gamma0 = float(null(np.asarray(gp, dtype=np.float64), np.asarray(tau, dtype=np.float64))[0])
    _gp, _tau, res = _fit_timevar(null, c, gp, tau, free_tau, ftol)
    return lnp_gamma0, -float(res["fun"])


def period_scan(lwls, fl, sigma, gp, tau, gamma, times, periods, component=0, mu_GP=1.0):
    """The likelihood periodogram of one component: ``lnp(P)`` of ``lnlike_quasiperiodic`` over the trial ``periods`` (n,) of
    ``component`` in ONE value-only batched call (``B = n``), every other parameter held; and the score ``d lnp / d gamma`` of
    that component at ``gamma = 0`` for every trial period, from one gradient call -- where the time-variable model is all
    there is the score is what a periodic factor of that period would gain to first order.  ``periods`` (n,) are the trial
    periods of ``component``; another component with ``gamma > 0`` needs a period of its own, and then ``periods`` must be
    (n, c), every component's (``ValueError`` otherwise: no ``gamma`` is changed behind the caller's back).  The score call
    takes every ``gamma = 0``.  Degenerate input follows ``lnlike_quasiperiodic``: a negative hyper-parameter, a ``tau`` or
    ``gamma`` that is none gives ``-inf`` and NaN throughout, a trial period that is none ``-inf`` and NaN in its place, a zero
    length scale or non-finite input the exception.  -> ``(lnp (n,), score (n,))``"""
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    c, N = lw.shape
    k = int(component)
    if not 0 <= k < c:
        raise ValueError(f"component must be in [0, {c})")
    gp, tau, gamma = as_f64(gp, (2 * c,)), as_f64(np.atleast_1d(as_f64(tau)), (c,)), as_f64(np.atleast_1d(as_f64(gamma)), (c,))
    per = as_f64(periods)
    if per.ndim == 1:
        if np.any(np.delete(gamma, k) != 0.0):
            raise ValueError("another component has gamma != 0 and needs a period of its own: give periods as (n, c)")
        trial = per
        per = np.ones((per.shape[0], c))      # (the period of a component at gamma = 0 does not enter: any)
        per[:, k] = trial
    n = per.shape[0]
    per = as_f64(per, (n, c))
    t = as_f64(times, (N,))
    if not np.all(np.isfinite(t)):
        raise ValueError(_NONFINITE)
    if np.any(gp < 0.0) or not _quasiperiodic_valid(tau, gamma, 1.0):
        return np.full(n, -np.inf), np.full(n, np.nan)
    _quasiperiodic_input(lw, sigma, [float(g) for g in gp])
    if not (np.all(np.isfinite(np.asarray(fl, dtype=np.float64))) and np.isfinite(mu_GP)):
        raise ValueError(_NONFINITE)
    h = _quasiperiodic_handle(fl, sigma, t, "period_scan")
    lws, gps, taus = np.broadcast_to(lw, (n, c, N)), np.broadcast_to(gp, (n, 2 * c)), np.broadcast_to(tau, (n, c))
    lnp = h.lnlike_qp(lws, gps, taus, np.broadcast_to(gamma, (n, c)), per, mu_GP)
    score = h.lnlike_qp_grad(lws, gps, taus, np.zeros((n, c)), per, mu_GP)[3][:, k]
    return np.asarray(lnp), np.asarray(score)


def _timevar_front(lwls, gp, tau):
    """``(lw (c, N), gp, tau (c,), degenerate)`` of a time-variable analysis call: the checks of ``_timevar`` up to the device
    -- ``degenerate``: a negative hyper-parameter or a ``tau <= 0`` or NaN, to be answered before any work"""
    gp = [float(g) for g in gp]
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    c = lw.shape[0]
    if len(gp) != 2 * c:
        raise ValueError(f"gp must hold {2 * c} values for {c} component(s)")
    tau = as_f64(np.atleast_1d(as_f64(tau)), (c,))
    return lw, gp, tau, any(g < 0.0 for g in gp) or not np.all(tau > 0.0)


def fisher_information_timevar(lwls, fl, sigma, gp, tau, times, baseline=None):
    """The ``(3c, 3c)`` Fisher information of ``(amp_0, l_0, ..., tau_0, ..., tau_{c-1})`` under the time-variable kernel of
    ``lnlike_timevar``, evaluated on the device (``ChunkHandle.fisher_tv`` with unit tangents, the cached handle with
    ``times - min(times)`` on it): what ``fisher_information`` is for the static kernel, with the time scales and their
    correlations with the amplitudes and length scales.  The row and column of a component with ``tau = inf`` are exactly
    zero.  Degenerate input follows ``lnlike_timevar``: a negative hyper-parameter, a ``tau <= 0`` or NaN or a matrix that is
    not positive definite gives NaN in every entry.  ``baseline`` (the dict of ``optimize_GP``): the information of
    ``lnlike_timevar_marginal``, under ``K_tv + H Lambda H^T`` (``ChunkHandle.fisher_marg_tv``) -- an error bar on
    ``tau`` from it carries the continuum's uncertainty."""
    base = None if baseline is None else _baseline_args(baseline)
    lw, gp, tau, degenerate = _timevar_front(lwls, gp, tau)
    c, N = lw.shape
    t = as_f64(times, (N,))
    if not np.all(np.isfinite(t)):
        raise ValueError(_NONFINITE)
    if degenerate:
        return np.full((3 * c, 3 * c), np.nan)
    if any(l == 0.0 for l in gp[1::2]):
        raise ZeroDivisionError("float division")
    if not _matrix_is_finite(lw, sigma, gp):
        raise ValueError(_NONFINITE)
    h, _t0 = _timevar_handle(fl, sigma, t, N, "fisher_information_timevar", base is not None)
    eye = np.eye(3 * c)
    if base is None:
        return h.fisher_tv(lw, gp, tau, eye[:, :2 * c], eye[:, 2 * c:])
    h.set_baseline(*base)      # (every call, as ``_marginal``)
    return h.fisher_marg_tv(lw, gp, tau, eye[:, :2 * c], eye[:, 2 * c:])


def _laplace_from_fisher(F, gp, tau, free):
    """The algebra of ``timevar_laplace`` on a given ``F (3c, 3c)`` -> ``(cov_log, sd_gp, sd_tau)``.  (Nothing here knows the
    device: the tests run it on the float64 CPU evaluation.)"""
    gp, tau = as_f64(gp), as_f64(np.atleast_1d(as_f64(tau)))
    c = tau.shape[0]
    free = np.asarray(free, dtype=bool).reshape(c)
    F = as_f64(F, (3 * c, 3 * c))
    if not np.all(np.isfinite(tau[free])):
        raise ValueError("a free tau must be finite")
    idx = np.concatenate([np.arange(2 * c), 2 * c + np.flatnonzero(free)])
    theta = np.concatenate([gp, tau])[idx]
    F_log = theta[:, None] * F[np.ix_(idx, idx)] * theta[None, :]       # d/dlog theta = theta d/dtheta
    try:
        if not np.all(np.isfinite(F_log)):
            raise np.linalg.LinAlgError
        L = np.linalg.cholesky(F_log)
    except np.linalg.LinAlgError:
        raise np.linalg.LinAlgError("timevar_laplace: the Fisher information of the free log parameters is singular") from None
    Linv = np.linalg.inv(L)
    cov_log = Linv.T @ Linv
    sd = theta * np.sqrt(np.diag(cov_log))                               # back to the parameters' own units
    sd_tau = np.full(c, np.nan)
    sd_tau[free] = sd[2 * c:]
    return cov_log, sd[:2 * c], sd_tau


def timevar_laplace(lwls, fl, sigma, gp, tau, times, free_tau=None, baseline=None):
    """The Laplace covariance of an ``optimize_GP_timevar`` fit at ``(gp, tau)``, in the parameters ``_fit_timevar`` fits in,
    ``(log gp, log tau[free])``: ``F_log = diag(theta) F diag(theta)`` of ``fisher_information_timevar`` restricted to the free
    parameters, inverted.  ``free_tau`` (c,) of booleans defaults as in ``optimize_GP_timevar``: every finite ``tau``.
    Returns ``(cov_log, sd_gp (2c,), sd_tau (c,))``: the covariance, and the standard deviations in the parameters' own units
    (``theta`` times that of ``log theta``), ``nan`` for a ``tau`` that is not free.  ``LinAlgError`` where ``F_log`` is
    singular -- also for the NaN of degenerate input.  ``baseline``: as ``fisher_information_timevar`` takes it, for a fit
    made with ``optimize_GP_timevar_marginal``."""
    tau = as_f64(np.atleast_1d(as_f64(tau)))
    free = np.isfinite(tau) if free_tau is None else np.asarray(free_tau, dtype=bool).reshape(tau.shape)
    return _laplace_from_fisher(fisher_information_timevar(lwls, fl, sigma, gp, tau, times, baseline), gp, tau, free)


def loo_timevar(lwls, fl, sigma, gp, tau, times, mu_GP=1.0, epoch_index=None):
    """``loo`` under the time-variable kernel of ``lnlike_timevar`` (``ChunkHandle.loo_tv`` through the cached handle with
    ``times - min(times)`` on it): the ``chunk.LooResult`` of the model ``optimize_GP_timevar`` fits, for the outlier search
    that matches it.  Degenerate input follows ``loo`` and ``lnlike_timevar``: a negative hyper-parameter or a ``tau <= 0`` or
    NaN gives ``lnp = -inf`` and NaN before any work."""
    from .chunk import LooResult
    lw, gp, tau, degenerate = _timevar_front(lwls, gp, tau)
    N = lw.shape[1]
    t = as_f64(times, (N,))
    if not np.all(np.isfinite(t)):
        raise ValueError(_NONFINITE)
    ep = None if epoch_index is None else np.asarray(epoch_index, dtype=np.int64)
    if ep is not None and (ep.shape != lw.shape[1:] or (ep.size and ep.min() < 0)):
        raise ValueError("epoch_index must hold one non-negative epoch per pixel")
    if degenerate:
        return LooResult.degenerate(N, None if ep is None else np.bincount(ep))
    if any(l == 0.0 for l in gp[1::2]):
        raise ZeroDivisionError("float division")
    if not _matrix_is_finite(lw, sigma, gp):
        raise ValueError(_NONFINITE)
    h, _t0 = _timevar_handle(fl, sigma, t, N, "loo_timevar")
    res = h.loo_tv(lw, gp, tau, mu_GP, ep)
    if not np.isneginf(res.lnp) and not (np.all(np.isfinite(np.asarray(fl, dtype=np.float64))) and np.isfinite(mu_GP)):
        raise ValueError(_NONFINITE)
    return res


# ---- Fisher information and leave-one-out under the quasi-periodic kernel -------------------------
def _quasiperiodic_front(lwls, gp, tau, gamma, period, times):
    """``(lw (c, N), gp, tau, gamma, period, t, degenerate)`` of a quasi-periodic analysis call: the front checks of
    ``_quasiperiodic`` up to the device -- ``degenerate``: a negative hyper-parameter or a ``tau``, ``gamma`` or ``period``
    that is none, to be answered before any work"""
    gp = [float(g) for g in gp]
    lw = np.stack([as_f64(w) for w in np.atleast_2d(lwls)])
    c, N = lw.shape
    if len(gp) != 2 * c:
        raise ValueError(f"gp must hold {2 * c} values for {c} component(s)")
    tau, gamma, period = (as_f64(np.atleast_1d(as_f64(v)), (c,)) for v in (tau, gamma, period))
    t = as_f64(times, (N,))
    if not np.all(np.isfinite(t)):
        raise ValueError(_NONFINITE)
    return lw, gp, tau, gamma, period, t, any(g < 0.0 for g in gp) or not _quasiperiodic_valid(tau, gamma, period)


def fisher_information_quasiperiodic(lwls, fl, sigma, gp, tau, gamma, period, times):
    """The ``(5c, 5c)`` Fisher information of ``(amp_0, l_0, ..., tau_*, Gamma_*, P_*)`` under the quasi-periodic kernel of
    ``lnlike_quasiperiodic``, evaluated on the device (``ChunkHandle.fisher_qp`` with unit tangents, the cached handle with
    ``times - min(times)`` on it): what ``fisher_information_timevar`` is for the time-variable kernel, with ``Gamma``, the
    periods and their correlations with everything else.  The row and column of the period of a component with
    ``gamma = 0`` are exactly zero, as are those of a ``tau = inf``.  Degenerate input follows ``lnlike_quasiperiodic``: a
    negative hyper-parameter, a ``tau``, ``gamma`` or ``period`` that is none or a matrix that is not positive definite gives
    NaN in every entry."""
    lw, gp, tau, gamma, period, t, degenerate = _quasiperiodic_front(lwls, gp, tau, gamma, period, times)
    c = lw.shape[0]
    if degenerate:
        return np.full((5 * c, 5 * c), np.nan)
    _quasiperiodic_input(lw, sigma, gp)
    h = _quasiperiodic_handle(fl, sigma, t, "fisher_information_quasiperiodic")
    eye = np.eye(5 * c)
    return h.fisher_qp(lw, gp, tau, gamma, period, eye[:, :2 * c], eye[:, 2 * c:3 * c], eye[:, 3 * c:4 * c], eye[:, 4 * c:])


def _qp_free(tau, gamma, free):
    """the free masks ``(tau, gamma, period)`` of ``_fit_quasiperiodic``: its dictionary and its defaults -- every finite
    ``tau`` and, for both others, every ``gamma > 0``"""
    c = tau.shape[0]
    free = {} if free is None else dict(free)
    if set(free) - {"tau", "gamma", "period"}:
        raise ValueError(f"free takes 'tau', 'gamma' and 'period'; got {sorted(free)}")
    return (np.asarray(free.get("tau", np.isfinite(tau)), dtype=bool).reshape(c),
            np.asarray(free.get("gamma", gamma > 0.0), dtype=bool).reshape(c),
            np.asarray(free.get("period", gamma > 0.0), dtype=bool).reshape(c))


def _laplace_from_fisher_blocks(F, theta, free, who):
    """``_laplace_from_fisher`` for any number of parameter blocks: ``F (n, n)`` over the parameters ``theta (n,)`` in their
    own units, ``free (n,)`` of booleans -> ``(cov_log, sd (n,))``: the inverse of ``F_log = diag(theta) F diag(theta)``
    restricted to the free parameters, and the standard deviations in the parameters' own units, ``nan`` where not free.
    ``LinAlgError`` where the restricted ``F_log`` is singular or not finite.  (Nothing here knows the device.)"""
    theta = as_f64(theta)
    n = theta.shape[0]
    F = as_f64(F, (n, n))
    idx = np.flatnonzero(np.asarray(free, dtype=bool).reshape(n))
    th = theta[idx]
    if not np.all(np.isfinite(th)):
        raise ValueError("a free parameter must be finite")
    F_log = th[:, None] * F[np.ix_(idx, idx)] * th[None, :]       # d/dlog theta = theta d/dtheta
    try:
        if not np.all(np.isfinite(F_log)):
            raise np.linalg.LinAlgError
        L = np.linalg.cholesky(F_log)
    except np.linalg.LinAlgError:
        raise np.linalg.LinAlgError(f"{who}: the Fisher information of the free log parameters is singular") from None
    Linv = np.linalg.inv(L)
    cov_log = Linv.T @ Linv
    sd = np.full(n, np.nan)
    sd[idx] = th * np.sqrt(np.diag(cov_log))
    return cov_log, sd


def _qp_laplace_from_fisher(F, gp, tau, gamma, period, free):
    """The algebra of ``quasiperiodic_laplace`` on a given ``F (5c, 5c)`` -> ``(cov_log, sd_gp, sd_tau, sd_gamma, sd_period)``
    (the tests run it on the float64 CPU evaluation)"""
    gp = as_f64(gp)
    tau, gamma, period = (as_f64(np.atleast_1d(as_f64(v))) for v in (tau, gamma, period))
    c = tau.shape[0]
    f_t, f_m, f_p = _qp_free(tau, gamma, free)
    mask = np.concatenate([np.ones(2 * c, dtype=bool), f_t, f_m, f_p])
    cov_log, sd = _laplace_from_fisher_blocks(F, np.concatenate([gp, tau, gamma, period]), mask, "quasiperiodic_laplace")
    return cov_log, sd[:2 * c], sd[2 * c:3 * c], sd[3 * c:4 * c], sd[4 * c:]


def quasiperiodic_laplace(lwls, fl, sigma, gp, tau, gamma, period, times, free=None):
    """The Laplace covariance of an ``optimize_GP_quasiperiodic`` fit at ``(gp, tau, gamma, period)``, in the parameters
    ``_fit_quasiperiodic`` fits in, ``(log gp, log tau[free], log gamma[free], log period[free])``: ``F_log = diag(theta) F
    diag(theta)`` of ``fisher_information_quasiperiodic`` restricted to the free parameters, inverted.  ``free`` is that
    function's dictionary with its defaults.  Returns ``(cov_log, sd_gp (2c,), sd_tau (c,), sd_gamma (c,), sd_period (c,))``:
    the covariance, and the standard deviations in the parameters' own units, ``nan`` where a parameter is not free.
    ``LinAlgError`` where ``F_log`` is singular -- a free period of a component with ``gamma = 0``, or the NaN of degenerate
    input."""
    return _qp_laplace_from_fisher(fisher_information_quasiperiodic(lwls, fl, sigma, gp, tau, gamma, period, times), gp, tau,
                                   gamma, period, free)


def loo_quasiperiodic(lwls, fl, sigma, gp, tau, gamma, period, times, mu_GP=1.0, epoch_index=None):
    """``loo_timevar`` under the quasi-periodic kernel of ``lnlike_quasiperiodic`` (``ChunkHandle.loo_qp``): the
    ``chunk.LooResult`` of the model ``optimize_GP_quasiperiodic`` fits.  Degenerate input follows ``loo_timevar`` and
    ``lnlike_quasiperiodic``: ``lnp = -inf`` and NaN before any work."""
    from .chunk import LooResult
    lw, gp, tau, gamma, period, t, degenerate = _quasiperiodic_front(lwls, gp, tau, gamma, period, times)
    N = lw.shape[1]
    ep = None if epoch_index is None else np.asarray(epoch_index, dtype=np.int64)
    if ep is not None and (ep.shape != lw.shape[1:] or (ep.size and ep.min() < 0)):
        raise ValueError("epoch_index must hold one non-negative epoch per pixel")
    if degenerate:
        return LooResult.degenerate(N, None if ep is None else np.bincount(ep))
    _quasiperiodic_input(lw, sigma, gp)
    h = _quasiperiodic_handle(fl, sigma, t, "loo_quasiperiodic")
    res = h.loo_qp(lw, gp, tau, gamma, period, mu_GP, ep)
    if not np.isneginf(res.lnp) and not (np.all(np.isfinite(np.asarray(fl, dtype=np.float64))) and np.isfinite(mu_GP)):
        raise ValueError(_NONFINITE)
    return res


def _periodicity_tangents(c, free_tau, k):
    """The ``2c + n_free + 1`` tangents of ``periodicity_score``: unit directions of ``gp``, of every free ``tau`` and, last,
    of ``Gamma`` of component ``k`` -> ``(tan_gp, tan_tau, tan_gamma)``"""
    f = np.flatnonzero(free_tau)
    T = 2 * c + f.shape[0] + 1
    tan_gp, tan_tau, tan_gamma = np.zeros((T, 2 * c)), np.zeros((T, c)), np.zeros((T, c))
    tan_gp[:2 * c] = np.eye(2 * c)
    tan_tau[2 * c + np.arange(f.shape[0]), f] = 1.0
    tan_gamma[T - 1, k] = 1.0
    return tan_gp, tan_tau, tan_gamma


def _periodicity_from_fisher(S, F):
    """The algebra of ``periodicity_score``: the score ``S`` of ``Gamma`` and the information ``F`` over (the nuisance
    parameters, ``Gamma``), ``Gamma`` last -> ``(z, S, I)`` with the efficient information ``I = F_GG - F_Gt F_tt^-1 F_tG`` and
    ``z = S / sqrt(I)``.  ``LinAlgError`` where ``F_tt`` is singular.  (Nothing here knows the device.)"""
    F = as_f64(F)
    n = F.shape[0] - 1
    if not np.all(np.isfinite(F)):
        raise np.linalg.LinAlgError("periodicity_score: the Fisher information is not finite")
    # (scaled to a unit diagonal: the parameters' units differ by many decades)
    d = 1.0 / np.sqrt(np.diag(F)[:n])
    L = np.linalg.cholesky(d[:, None] * F[:n, :n] * d[None, :])
    v = np.linalg.solve(L, d * F[:n, n])
    I = float(F[n, n] - v @ v)
    return float(S) / np.sqrt(I), float(S), I


def periodicity_score(lwls, fl, sigma, gp, tau, times, period, component=0, free_tau=None, mu_GP=1.0):
    """The score test for a periodic factor of ``component`` at the trial ``period``, evaluated at ``Gamma = 0`` on the
    time-variable fit ``(gp, tau)``: ``S = d lnp / d Gamma`` of that component (one ``lnlike_qp_grad`` call) and the Fisher
    information over ``(gp, tau[free], Gamma_component)`` (one ``fisher_qp`` call with ``2c + n_free + 1`` tangents), from
    which the efficient information ``I = F_GG - F_Gt F_tt^-1 F_tG`` discounts what a re-fit of ``(gp, tau)`` would absorb.
    -> ``(z, S, I)``, ``z = S / sqrt(I)``: asymptotically standard normal where ``(gp, tau)`` is the time-variable fit, and the
    test is one-sided (``Gamma >= 0``): a large positive ``z`` speaks for the period.  ``free_tau`` (c,) defaults to every
    finite ``tau``.  The period is no nuisance direction: at ``Gamma = 0`` its row of ``F`` is exactly zero.  Degenerate
    input follows ``lnlike_quasiperiodic`` and gives ``(nan, nan, nan)``."""
    c = np.atleast_2d(lwls).shape[0]
    k = int(component)
    if not 0 <= k < c:
        raise ValueError(f"component must be in [0, {c})")
    per = np.ones(c)      # (the period of a component at Gamma = 0 does not enter: any)
    per[k] = float(period)
    zero = np.zeros(c)
    lw, gp, tau, gamma, per, t, degenerate = _quasiperiodic_front(lwls, gp, tau, zero, per, times)
    free = np.isfinite(tau) if free_tau is None else np.asarray(free_tau, dtype=bool).reshape(c)
    if degenerate:
        return np.nan, np.nan, np.nan
    _quasiperiodic_input(lw, sigma, gp)
    if not (np.all(np.isfinite(np.asarray(fl, dtype=np.float64))) and np.isfinite(mu_GP)):
        raise ValueError(_NONFINITE)
    h = _quasiperiodic_handle(fl, sigma, t, "periodicity_score")
    S = h.lnlike_qp_grad(lw, gp, tau, gamma, per, mu_GP)[3][k]
    tan_gp, tan_tau, tan_gamma = _periodicity_tangents(c, free, k)
    F = h.fisher_qp(lw, gp, tau, gamma, per, tan_gp, tan_tau, tan_gamma)
    return _periodicity_from_fisher(S, F)


# ---- calibration ---------------------------------------------------------------
_CAL_FAIL = {1: "reference-epoch covariance B", 2: "conditional covariance C'", 3: "Chebyshev normal equations"}


def _cal_result(status, fl_cor, X):
    if status != 0:
        # cho_factor raises in the reference (covariance.py:597-601, :607, :613)
        print("Failed to solve matrix inverse. Calibration not valid.")
        raise np.linalg.LinAlgError(f"{_CAL_FAIL[status]} is not positive definite")
    return fl_cor, X


def optimize_calibration(lwl0, lwl1, lwl_cal, fl_cal, fl_fixed, A, B, C, order=1, mu_GP=1.0):
    """Chebyshev calibration of one epoch with caller-filled covariance blocks (covariance.py:560-624).

    ``A`` (M,M) and ``B`` (N,N) carry the squared uncertainties on their diagonals, ``C`` (M,N) is the
    cross block.  Returns ``(fl_cor (M,), X (order+1,))``; the two Cholesky passes run on the device.
    """
    lwl_cal = as_f64(lwl_cal)
    M = lwl_cal.shape[0]
    fl_cal = as_f64(fl_cal, (M,))
    fl_fixed = as_f64(np.asarray(fl_fixed).flatten())
    N = fl_fixed.shape[0]
    A, B, C = as_f64(A, (M, M)), as_f64(B, (N, N)), as_f64(C, (M, N))
    fl_cor, X = np.empty(M), np.empty(order + 1)
    status = ctypes.c_int(0)
    check(_lib.load().psoap_calibrate_explicit(_lib.default_device(), M, N, int(order), float(lwl0), float(lwl1),
                                               dptr(lwl_cal), dptr(fl_cal), dptr(fl_fixed), dptr(A), dptr(B), dptr(C),
                                               float(mu_GP), dptr(fl_cor), dptr(X), ctypes.byref(status)),
          "psoap_calibrate_explicit")
    return _cal_result(status.value, fl_cor, X)


def optimize_calibration_components(lwl0, lwl1, lwl_cal, lwls_cal, fl_cal, sigma_cal, lwls_fixed, fl_fixed, sigma_fixed,
                                    gp, order=1, mu_GP=1.0):
    """The per-epoch body of scripts/psoap_process_calibration_ST3.py:147-183 with the covariance blocks
    evaluated on the device: ``lwls_cal`` (c,M) / ``lwls_fixed`` (c,N) are the rest-frame grids of the epoch
    and of the reference epochs, ``gp = (amp_f, l_f[, amp_g, l_g[, amp_h, l_h]])``; ``lwl_cal`` (M,) is the
    observed-frame abscissa of the Chebyshev polynomials on [lwl0, lwl1]."""
    lwls_cal = np.ascontiguousarray(np.atleast_2d(np.asarray(lwls_cal, dtype=np.float64)))
    lwls_fixed = np.ascontiguousarray(np.atleast_2d(np.asarray(lwls_fixed, dtype=np.float64)))
    c, M = lwls_cal.shape
    N = lwls_fixed.shape[1]
    assert lwls_fixed.shape[0] == c, "epoch and reference grids need the same number of components"
    lwl_cal, fl_cal, sigma_cal = as_f64(lwl_cal, (M,)), as_f64(fl_cal, (M,)), as_f64(sigma_cal, (M,))
    fl_fixed, sigma_fixed = as_f64(np.asarray(fl_fixed).flatten(), (N,)), as_f64(np.asarray(sigma_fixed).flatten(), (N,))
    gp = as_f64(gp, (2 * c,))
    fl_cor, X = np.empty(M), np.empty(order + 1)
    status = ctypes.c_int(0)
    check(_lib.load().psoap_calibrate(_lib.default_device(), c, M, N, int(order), float(lwl0), float(lwl1), dptr(lwl_cal),
                                      dptr(lwls_cal), dptr(fl_cal), dptr(sigma_cal), dptr(lwls_fixed), dptr(fl_fixed),
                                      dptr(sigma_fixed), dptr(gp), float(mu_GP), dptr(fl_cor), dptr(X),
                                      ctypes.byref(status)),
          "psoap_calibrate")
    return _cal_result(status.value, fl_cor, X)


def optimize_calibration_static(wl0, wl1, wl_cal, fl_cal, sigma_cal, wl_fixed, fl_fixed, sigma_fixed, amp, l_f, order=1,
                                mu_GP=1.0):
    """Single-component calibration with zero relative velocities (covariance.py:628-707): the same
    vectors serve as kernel abscissa and as Chebyshev abscissa."""
    return optimize_calibration_components(wl0, wl1, wl_cal, [wl_cal], fl_cal, sigma_cal,
                                           [np.asarray(wl_fixed).flatten()], fl_fixed, sigma_fixed, [amp, l_f],
                                           order=order, mu_GP=mu_GP)


def cycle_calibration(wl, fl, sigma, amp_f, l_f, ncycles, order=1, limit_array=3, mu_GP=1.0, soften=1.0):
    """Cycle the calibration over all epochs of an (n_epochs, n_pix) block (covariance.py:710-745).

    The reference body calls ``optimize_calibration`` with ``optimize_calibration_static``'s argument
    list (:740) and cannot run; this implements that evident intent."""
    wl, sigma = np.asarray(wl, dtype=np.float64), soften * np.asarray(sigma, dtype=np.float64)
    wl0, wl1 = np.min(wl), np.max(wl)
    fl_out = np.array(fl, dtype=np.float64)
    for _ in range(ncycles):
        for i in range(len(wl)):
            wl_remain = np.delete(wl, i, axis=0)[0:limit_array]
            fl_remain = np.delete(fl_out, i, axis=0)[0:limit_array]
            sigma_remain = np.delete(sigma, i, axis=0)[0:limit_array]
            fl_out[i], _X = optimize_calibration_static(wl0, wl1, wl[i], fl_out[i], sigma[i], wl_remain.flatten(),
                                                        fl_remain.flatten(), sigma_remain.flatten(), amp_f, l_f,
                                                        order=order, mu_GP=mu_GP)
    return fl_out


def cycle_calibration_chunk(chunk, amp_f, l_f, n_cycles, order=1, limit_array=3, mu_GP=1.0, soften=1.0):
    """Mask-aware cycle over a 2-D ``Chunk``; overwrites ``chunk.fl`` (covariance.py:747-800, same stale
    call at :776).  Masked pixels are left out of the solve and corrected with the fitted polynomial.
    As in the reference, ``soften`` is computed but the un-softened ``chunk.sigma`` enters the solve."""
    from numpy.polynomial import chebyshev as npcheb
    wl0, wl1 = np.min(chunk.wl), np.max(chunk.wl)
    fl_out = np.array(chunk.fl, dtype=np.float64)
    for _ in range(n_cycles):
        for i in range(chunk.n_epochs):
            mt = chunk.mask[i]
            wl_remain = np.delete(chunk.wl, i, axis=0)[0:limit_array]
            fl_remain = np.delete(fl_out, i, axis=0)[0:limit_array]
            sigma_remain = np.delete(chunk.sigma, i, axis=0)[0:limit_array]
            mr = np.delete(chunk.mask, i, axis=0)[0:limit_array]
            _fl, X = optimize_calibration_static(wl0, wl1, chunk.wl[i][mt], fl_out[i][mt], chunk.sigma[i][mt],
                                                 wl_remain[mr], fl_remain[mr], sigma_remain[mr], amp_f, l_f,
                                                 order=order, mu_GP=mu_GP)
            u = (2.0 * chunk.wl[i] - (wl0 + wl1)) / (wl1 - wl0)
            fl_out[i] = fl_out[i] * npcheb.chebval(u, X)          # D X re-evaluated on every pixel (:781-797)
    chunk.fl[:] = fl_out
