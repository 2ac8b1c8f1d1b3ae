"""Persistent per-chunk device state and batched likelihood evaluation.

Host-side counterpart of ``Worker.initialize`` / ``Worker.lnprob``
(/root/reference/psoap/sample_parallel.py:126-198): ``fl`` and ``sigma`` stay
resident in HBM, ``max_batch`` scratch matrices replace the single ``V11``
(:163), and a whole batch of proposals is evaluated per call.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import K_NAMES, Timings, as_f64, check, dptr


class LooResult:
    """What ``ChunkHandle.loo`` returns: ``lnp``, ``loo_logp`` (the sum of ``pix_logp``); per pixel ``pix_mean``, ``pix_var``
    (of the observed flux: noise included), ``pix_logp`` and the derived ``pix_z = (fl - pix_mean) / sqrt(pix_var)``; per epoch
    ``ep_resid`` (N,), ``ep_chi2``, ``ep_logp``, ``ep_npix`` -- ``None`` when no epoch index was given."""
    __slots__ = ("lnp", "loo_logp", "pix_mean", "pix_var", "pix_logp", "pix_z", "ep_resid", "ep_chi2", "ep_logp", "ep_npix")

    def __init__(self, lnp, loo_logp, pix_mean, pix_var, pix_logp, fl, ep_resid=None, ep_chi2=None, ep_logp=None, ep_npix=None):
        self.lnp, self.loo_logp = lnp, loo_logp
        self.pix_mean, self.pix_var, self.pix_logp = pix_mean, pix_var, pix_logp
        with np.errstate(invalid="ignore"):
            self.pix_z = (np.asarray(fl, dtype=np.float64) - pix_mean) / np.sqrt(pix_var)      # = alpha_i / sqrt(A_ii)
        self.ep_resid, self.ep_chi2, self.ep_logp, self.ep_npix = ep_resid, ep_chi2, ep_logp, ep_npix

    @classmethod
    def degenerate(cls, N, ep_npix=None):
        """the ``-inf`` / NaN result of a call that never reaches the device (``ep_npix``: the epochs' pixel counts)"""
        nan = lambda n: np.full(n, np.nan)      # noqa: E731
        if ep_npix is None:
            return cls(-np.inf, np.nan, nan(N), nan(N), nan(N), nan(N))
        npix = np.asarray(ep_npix, dtype=np.int32)
        return cls(-np.inf, np.nan, nan(N), nan(N), nan(N), nan(N), nan(N), nan(npix.size), nan(npix.size), npix)


class MargResult:
    """What ``ChunkHandle.lnlike_marg`` returns when more than the value is asked for: ``lnp``; ``parts`` = (z^T z,
    log det K, the gain, log det M); ``beta`` (n_epochs, order + 1) and ``beta_cov`` (q, q), the posterior mean and covariance
    of the continuum coefficients; ``fl_cor`` (N,), the flux minus the posterior-mean continuum term.  A field that was not
    asked for is ``None``; a batched call gives every field a leading axis of B."""
    __slots__ = ("lnp", "parts", "beta", "beta_cov", "fl_cor")

    def __init__(self, lnp, parts, beta=None, beta_cov=None, fl_cor=None):
        self.lnp, self.parts, self.beta, self.beta_cov, self.fl_cor = lnp, parts, beta, beta_cov, fl_cor

    @property
    def beta_sd(self):
        """posterior standard deviations in the shape of ``beta`` (``None`` without ``beta_cov``)"""
        if self.beta_cov is None:
            return None
        d = np.sqrt(np.diagonal(self.beta_cov, axis1=-2, axis2=-1))
        return d if self.beta is None else d.reshape(np.shape(self.beta))


class ChunkHandle:
    def __init__(self, fl, sigma, max_batch: int = 1, device: int | None = None):
        self._L = _lib.load()
        self.fl = as_f64(fl)
        self.sigma = as_f64(sigma, self.fl.shape)
        if self.fl.ndim != 1:
            raise ValueError("fl and sigma must be 1-D")
        self.N = int(self.fl.shape[0])
        self.max_batch = int(max_batch)
        self.device = _lib.default_device() if device is None else int(device)
        self._h = ctypes.c_void_p()
        check(self._L.psoap_chunk_create(ctypes.byref(self._h), self.device, self.N, dptr(self.fl),
                                         dptr(self.sigma), self.max_batch), "psoap_chunk_create")
        self._B = 0
        self.n_epochs = 0
        self._sigma_rows = 0

    # -- lifetime -----------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.psoap_chunk_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- configuration --------------------------------------------------------------
    def set_data(self, fl, sigma):
        self.fl = as_f64(fl, (self.N,))
        self.sigma = as_f64(sigma, (self.N,))
        check(self._L.psoap_chunk_set_data(self._h, dptr(self.fl), dptr(self.sigma)), "psoap_chunk_set_data")

    def set_grid(self, lwl, epoch_index, n_epochs: int):
        """Observed-frame ln-wavelengths + epoch of every pixel, for device-side Doppler shifts."""
        lwl = as_f64(lwl, (self.N,))
        ep = np.ascontiguousarray(epoch_index, dtype=np.int32)
        if ep.shape != (self.N,):
            raise ValueError("epoch_index must have shape (N,)")
        check(self._L.psoap_chunk_set_grid(self._h, dptr(lwl), ep.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                           int(n_epochs)), "psoap_chunk_set_grid")
        self.n_epochs = int(n_epochs)

    def set_stream_groups(self, groups: int):
        check(self._L.psoap_chunk_set_stream_groups(self._h, int(groups)), "psoap_chunk_set_stream_groups")

    def set_mode(self, mode: str | int):
        """"dag" (default): one persistent dependency-graph kernel; "staged": three kernels per panel."""
        m = {"staged": 0, "dag": 1}.get(mode, mode)
        check(self._L.psoap_chunk_set_mode(self._h, int(m)), "psoap_chunk_set_mode")

    def set_profiling(self, enabled: bool):
        check(self._L.psoap_chunk_set_profiling(self._h, int(bool(enabled))), "psoap_chunk_set_profiling")

    # -- evaluation -----------------------------------------------------------------
    def lnlike(self, lwls, gp, mu_GP: float = 1.0) -> float:
        lwls = as_f64(np.atleast_2d(lwls))
        c = lwls.shape[0]
        lwls = as_f64(lwls, (c, self.N))
        gp = as_f64(gp, (2 * c,))
        out = np.empty(1)
        check(self._L.psoap_lnlike(self._h, c, dptr(lwls), dptr(gp), float(mu_GP), dptr(out)), "psoap_lnlike")
        return float(out[0])

    def lnlike_batch(self, lwls, gps, mu_GP: float = 1.0) -> np.ndarray:
        lwls = as_f64(lwls)
        if lwls.ndim != 3 or lwls.shape[2] != self.N:
            raise ValueError("lwls must have shape (B, c, N)")
        B, c, _ = lwls.shape
        gps = as_f64(gps, (B, 2 * c))
        out = np.empty(B)
        check(self._L.psoap_lnlike_batch(self._h, B, c, dptr(lwls), dptr(gps), float(mu_GP), dptr(out)),
              "psoap_lnlike_batch")
        return out

    def _proposals(self, lwls, gp):
        """``lwls`` (c, N) with ``gp`` (2c,), or (B, c, N) with (B, 2c) -> ``(single, B, c, lwls (B, c, N), gps (B, 2c))``"""
        lwls = as_f64(lwls)
        single = lwls.ndim <= 2
        if single:
            lwls = np.atleast_2d(lwls)[None]
        if lwls.ndim != 3 or lwls.shape[2] != self.N:
            raise ValueError("lwls must have shape (c, N) or (B, c, N)")
        B, c, _ = lwls.shape
        return single, B, c, as_f64(lwls, (B, c, self.N)), as_f64(np.atleast_2d(as_f64(gp)), (B, 2 * c))

    def _orbit_proposals(self, model_id, p_orb, gps):
        """-> ``(B, c, n_orb, p_orb (B, n_orb), gps (B, 2c))`` for the orbit model ``model_id``"""
        from .utils import MODEL_ID, N_COMPONENTS, n_params_orb
        name = {v: k for k, v in MODEL_ID.items()}.get(int(model_id))
        if name is None:
            raise ValueError(f"unknown orbit model {model_id}")
        p_orb = as_f64(np.atleast_2d(p_orb))
        B, c, n_orb = p_orb.shape[0], N_COMPONENTS[name], n_params_orb[name]
        # (the library reads exactly n_orb doubles per proposal)
        return B, c, n_orb, as_f64(p_orb, (B, n_orb)), as_f64(np.atleast_2d(as_f64(gps)), (B, 2 * c))

    def _lnlike_grad(self, entry, lwls, gp, mu_GP, *after_lnp):
        """the body of ``lnlike_grad`` and ``lnlike_marg_grad``: ``entry`` names the library's function, ``after_lnp`` is what
        it takes between ``lnp`` and the three gradients"""
        single, B, c, lwls, gps = self._proposals(lwls, gp)
        lnp, g_gp, g_lwl, g_mu = np.empty(B), np.empty((B, 2 * c)), np.empty((B, c, self.N)), np.empty(B)
        check(getattr(self._L, entry)(self._h, B, c, dptr(lwls), dptr(gps), float(mu_GP), dptr(lnp), *after_lnp, dptr(g_gp),
                                      dptr(g_lwl), dptr(g_mu)), entry)
        if single:
            return float(lnp[0]), g_gp[0], g_lwl[0], float(g_mu[0])
        return lnp, g_gp, g_lwl, g_mu

    def _lnprob_grad(self, entry, vel_last, model_id, p_orb, gps, mu_GP, want_vel, tau=None):
        """the body of ``lnprob_grad``, ``lnprob_marg_grad`` and their ``_tv`` forms: ``entry`` names the library's function,
        which takes ``grad_vel`` after ``grad_mu`` (``vel_last``) or before it and, with ``tau``, the time scales after ``gps``
        and ``grad_tau`` after ``grad_gp`` (returned there as well)"""
        B, c, n_orb, p_orb, gps = self._orbit_proposals(model_id, p_orb, gps)
        lnp, g_orb, g_gp, g_mu = np.empty(B), np.empty((B, n_orb)), np.empty((B, 2 * c)), np.empty(B)
        g_vel = np.empty((B, c, self.n_epochs)) if want_vel else None
        after_gp, after_grad_gp = (), ()
        if tau is not None:
            taus, g_tau = as_f64(np.atleast_2d(as_f64(tau)), (B, c)), np.empty((B, c))
            after_gp, after_grad_gp = (dptr(taus),), (dptr(g_tau),)
        tail = (dptr(g_mu), dptr(g_vel) if want_vel else None)
        check(getattr(self._L, entry)(self._h, B, int(model_id), dptr(p_orb), dptr(gps), *after_gp, float(mu_GP), dptr(lnp),
                                      dptr(g_orb), dptr(g_gp), *after_grad_gp, *(tail if vel_last else tail[::-1])), entry)
        out = (lnp, g_orb, g_gp) + (() if tau is None else (g_tau,)) + (g_mu,)
        return out + (g_vel,) if want_vel else out

    def lnlike_grad(self, lwls, gp, mu_GP: float = 1.0):
        """Value and analytic gradient of the likelihood (include/psoap_gp.h: psoap_chunk_lnlike_grad).

        ``lwls`` (c, N) with ``gp`` (2c,) -> ``(lnp, grad_gp (2c,), grad_lwl (c, N), grad_mu)``; ``lwls`` (B, c, N) with
        ``gp`` (B, 2c) -> the same with a leading axis of B (any B: the proposals are walked in groups through a bounded
        workspace).  A negative hyper-parameter or a matrix that is not positive definite gives ``-inf`` and NaN gradients."""
        return self._lnlike_grad("psoap_chunk_lnlike_grad", lwls, gp, mu_GP)

    def lnprob_grad(self, model_id: int, p_orb, gps, mu_GP: float = 1.0, want_vel: bool = False):
        """Value and gradient of ``lnprob`` through the Kepler solve and the Doppler shift (include/psoap_gp.h:
        psoap_chunk_lnprob_grad; needs ``set_grid`` and the dates).

        ``p_orb`` (B, n_orb), ``gps`` (B, 2c) -> ``(lnp (B,), grad_orb (B, n_orb), grad_gp (B, 2c), grad_mu (B,))``, with
        ``grad_vel (B, c, n_epochs)`` appended when ``want_vel``.  A faster-than-light proposal, a negative hyper-parameter
        or a matrix that is not positive definite gives ``-inf`` and NaN gradients for that proposal."""
        return self._lnprob_grad("psoap_chunk_lnprob_grad", False, model_id, p_orb, gps, mu_GP, want_vel)

    def grad_release(self):
        """Free the gradient workspace (16 Npad^2 bytes per matrix of a group); the next ``lnlike_grad`` allocates it again."""
        check(self._L.psoap_chunk_grad_release(self._h), "psoap_chunk_grad_release")

    # -- time-variable component spectra (include/psoap_gp.h: psoap_chunk_lnlike_tv_grad) ---------------------------
    def set_times(self, t):
        """The observation time of every pixel in days, ``(N,)``, any order; kept on the device with the handle.  Pass
        times minus a constant (their minimum): the device subtracts them from each other."""
        t = as_f64(t, (self.N,))
        check(self._L.psoap_chunk_set_times(self._h, dptr(t)), "psoap_chunk_set_times")

    def _tv(self, lwls, gp, tau, mu_GP, want_grad):
        single, B, c, lwls, gps = self._proposals(lwls, gp)
        taus = as_f64(np.atleast_2d(as_f64(tau)), (B, c))
        lnp = np.empty(B)
        if not want_grad:
            check(self._L.psoap_chunk_lnlike_tv_grad(self._h, B, c, dptr(lwls), dptr(gps), dptr(taus), float(mu_GP), dptr(lnp),
                                                     None, None, None, None), "psoap_chunk_lnlike_tv_grad")
            return float(lnp[0]) if single else lnp
        g_gp, g_tau, g_lwl, g_mu = np.empty((B, 2 * c)), np.empty((B, c)), np.empty((B, c, self.N)), np.empty(B)
        check(self._L.psoap_chunk_lnlike_tv_grad(self._h, B, c, dptr(lwls), dptr(gps), dptr(taus), float(mu_GP), dptr(lnp),
                                                 dptr(g_gp), dptr(g_tau), dptr(g_lwl), dptr(g_mu)), "psoap_chunk_lnlike_tv_grad")
        if single:
            return float(lnp[0]), g_gp[0], g_tau[0], g_lwl[0], float(g_mu[0])
        return lnp, g_gp, g_tau, g_lwl, g_mu

    def lnlike_tv(self, lwls, gp, tau, mu_GP: float = 1.0):
        """The likelihood under the time-variable kernel, ``K_ij = sum_c a_c^2 exp(p_c d^2 - dt^2 / (2 tau_c^2)) + sigma^2``
        (needs ``set_times``): ``lwls`` (c, N) with ``gp`` (2c,) and ``tau`` (c,) -> ``lnp``; (B, c, N) with (B, 2c) and
        (B, c) -> ``(B,)``.  ``tau = inf`` is the static model; ``tau <= 0`` or NaN gives ``-inf``.  The bits of ``lnp`` are
        those of ``lnlike_tv_grad``."""
        return self._tv(lwls, gp, tau, mu_GP, False)

    def lnlike_tv_grad(self, lwls, gp, tau, mu_GP: float = 1.0):
        """``lnlike_tv`` and its analytic gradient: ``(lnp, grad_gp, grad_tau, grad_lwl, grad_mu)``, shapes as
        ``lnlike_grad`` with ``grad_tau`` (c,) or (B, c).  With every ``tau = inf`` the other four outputs have the bits of
        ``lnlike_grad`` and ``grad_tau`` is exactly 0.  ``tau <= 0`` or NaN, a negative hyper-parameter or a matrix that is
        not positive definite gives ``-inf`` and NaN gradients for that proposal."""
        return self._tv(lwls, gp, tau, mu_GP, True)

    # -- quasi-periodic temporal factor (include/psoap_gp.h: psoap_chunk_lnlike_qp_grad) -------------------------------
    def _qp(self, lwls, gp, tau, gamma, period, mu_GP, want_grad):
        single, B, c, lwls, gps = self._proposals(lwls, gp)
        taus, gams, pers = (as_f64(np.atleast_2d(as_f64(v)), (B, c)) for v in (tau, gamma, period))
        lnp = np.empty(B)
        entry = "psoap_chunk_lnlike_qp_grad"
        head = (self._h, B, c, dptr(lwls), dptr(gps), dptr(taus), dptr(gams), dptr(pers), float(mu_GP), dptr(lnp))
        if not want_grad:
            check(getattr(self._L, entry)(*head, None, None, None, None, None, None), entry)
            return float(lnp[0]) if single else lnp
        g_gp, g_lwl, g_mu = np.empty((B, 2 * c)), np.empty((B, c, self.N)), np.empty(B)
        g_tau, g_gam, g_per = np.empty((B, c)), np.empty((B, c)), np.empty((B, c))
        check(getattr(self._L, entry)(*head, dptr(g_gp), dptr(g_tau), dptr(g_gam), dptr(g_per), dptr(g_lwl), dptr(g_mu)), entry)
        if single:
            return float(lnp[0]), g_gp[0], g_tau[0], g_gam[0], g_per[0], g_lwl[0], float(g_mu[0])
        return lnp, g_gp, g_tau, g_gam, g_per, g_lwl, g_mu

    def lnlike_qp(self, lwls, gp, tau, gamma, period, mu_GP: float = 1.0):
        """The likelihood under the quasi-periodic kernel, ``K_ij = sum_c a_c^2 exp(p_c d^2 - dt^2 / (2 tau_c^2) - gamma_c
        sin^2(pi dt / period_c)) + sigma^2`` (needs ``set_times``): the shapes of ``lnlike_tv`` with ``gamma`` and ``period``
        shaped as ``tau``.  ``gamma = 0`` is ``lnlike_tv`` bit for bit whatever ``period``; ``gamma < 0``, NaN or inf,
        ``period <= 0``, NaN or inf and ``tau <= 0`` or NaN give ``-inf``.  The bits of ``lnp`` are those of ``lnlike_qp_grad``."""
        return self._qp(lwls, gp, tau, gamma, period, mu_GP, False)

    def lnlike_qp_grad(self, lwls, gp, tau, gamma, period, mu_GP: float = 1.0):
        """``lnlike_qp`` and its analytic gradient: ``(lnp, grad_gp, grad_tau, grad_gamma, grad_period, grad_lwl, grad_mu)``.
        At ``gamma = 0`` the outputs ``lnlike_tv_grad`` has carry its bits, ``grad_period`` is exactly 0 and ``grad_gamma`` is
        the score of a test for periodicity.  A value that is no proposal gives ``-inf`` and NaN gradients there only."""
        return self._qp(lwls, gp, tau, gamma, period, mu_GP, True)

    def fisher(self, lwls, gp, tan_gp, tan_lwl=None, want_mu: bool = False):
        """Fisher information of the likelihood at ``lwls`` (c, N), ``gp`` (2c,) along T <= 32 tangents (include/psoap_gp.h:
        psoap_chunk_fisher): ``tan_gp`` (T, 2c) and ``tan_lwl`` (T, c, N) (``None``: zeros) -> ``F (T, T)``,
        ``F_st = 1/2 tr(K^-1 K_s K^-1 K_t)``, symmetric bit for bit; with ``want_mu`` ``(F, F_mu)``, ``F_mu = 1^T K^-1 1``.
        A negative hyper-parameter or a matrix that is not positive definite gives NaN in every entry.  Always under the
        plain ``K``, also on a handle with a baseline: ``fisher_marg`` is the form under ``K + H Lambda H^T``."""
        return self._fisher("psoap_chunk_fisher", lwls, gp, tan_gp, tan_lwl, want_mu)

    def _fisher(self, entry, lwls, gp, tan_gp, tan_lwl, want_mu, tau=None, tan_tau=None, qp=None):
        """the body of ``fisher``, ``fisher_marg``, ``fisher_tv``, ``fisher_marg_tv`` and ``fisher_qp``: ``entry`` names the library's function, which with ``tau``
        takes it after ``gp`` and ``tan_tau`` after ``tan_gp``, and with ``qp = (gamma, period, tan_gamma, tan_period)`` the first
        two behind ``tau`` and the other two behind ``tan_tau``"""
        lwls = as_f64(np.atleast_2d(lwls))
        c = lwls.shape[0]
        lwls = as_f64(lwls, (c, self.N))
        gp = as_f64(gp, (2 * c,))
        tan_gp = as_f64(np.atleast_2d(as_f64(tan_gp)))
        T = tan_gp.shape[0]
        tan_gp = as_f64(tan_gp, (T, 2 * c))
        if tan_lwl is not None:
            tan_lwl = as_f64(tan_lwl, (T, c, self.N))
        after_gp, after_tan_gp = (), ()
        if tau is not None:
            tau = as_f64(np.atleast_1d(as_f64(tau)), (c,))
            if tan_tau is not None:
                tan_tau = as_f64(np.atleast_2d(as_f64(tan_tau)), (T, c))
            after_gp, after_tan_gp = (dptr(tau),), (None if tan_tau is None else dptr(tan_tau),)
        if qp is not None:
            hyper = [as_f64(np.atleast_1d(as_f64(v)), (c,)) for v in qp[:2]]
            tans = [None if v is None else as_f64(np.atleast_2d(as_f64(v)), (T, c)) for v in qp[2:]]
            after_gp += tuple(dptr(v) for v in hyper)
            after_tan_gp += tuple(None if v is None else dptr(v) for v in tans)
        F, mu = np.empty((T, T)), np.empty(1)
        check(getattr(self._L, entry)(self._h, c, dptr(lwls), dptr(gp), *after_gp, T, None if tan_lwl is None else dptr(tan_lwl),
                                      dptr(tan_gp), *after_tan_gp, dptr(F), dptr(mu) if want_mu else None), entry)
        return (F, float(mu[0])) if want_mu else F

    def fisher_tv(self, lwls, gp, tau, tan_gp, tan_tau=None, tan_lwl=None, want_mu: bool = False):
        """``fisher`` under the time-variable kernel of ``lnlike_tv`` (include/psoap_gp.h: psoap_chunk_fisher_tv; needs
        ``set_times``): ``tau`` (c,), and a tangent has a time-scale part, ``tan_tau`` (T, c) (``None``: zeros), beside
        ``tan_gp`` (T, 2c) and ``tan_lwl`` (T, c, N).  ``F (T, T)`` symmetric bit for bit; with every ``tau = inf`` it has
        the bits of ``fisher`` whatever ``tan_tau`` holds, and a tangent with nothing but a time-scale part gives an
        exactly-zero row and column.  ``tau <= 0`` or NaN, a negative hyper-parameter or a matrix that is not positive
        definite gives NaN in every entry; a handle with a baseline is refused."""
        return self._fisher("psoap_chunk_fisher_tv", lwls, gp, tan_gp, tan_lwl, want_mu, tau, tan_tau)

    def fisher_qp(self, lwls, gp, tau, gamma, period, tan_gp, tan_tau=None, tan_gamma=None, tan_period=None, tan_lwl=None,
                  want_mu: bool = False):
        """``fisher_tv`` under the quasi-periodic kernel of ``lnlike_qp`` (include/psoap_gp.h: psoap_chunk_fisher_qp; needs
        ``set_times``): ``gamma`` and ``period`` (c,) behind ``tau``, and a tangent has a ``Gamma`` and a period part,
        ``tan_gamma`` and ``tan_period`` (T, c) (``None``: zeros), behind ``tan_tau``.  ``F (T, T)`` symmetric bit for bit; with
        every ``gamma = 0`` and ``tan_gamma`` zero it has the bits of ``fisher_tv`` whatever ``period`` and ``tan_period`` hold,
        and a tangent with nothing but the period of a component with ``gamma = 0`` gives an exactly-zero row and column.  A
        ``tau``, ``gamma`` or ``period`` that is no proposal (``lnlike_qp``), a negative hyper-parameter or a matrix that is not
        positive definite gives NaN in every entry; a handle with a baseline is refused."""
        return self._fisher("psoap_chunk_fisher_qp", lwls, gp, tan_gp, tan_lwl, want_mu, tau, tan_tau,
                            (gamma, period, tan_gamma, tan_period))

    def fisher_marg(self, lwls, gp, tan_gp, tan_lwl=None, want_mu: bool = False):
        """``fisher`` under the baseline of ``set_baseline`` (include/psoap_gp.h: psoap_chunk_fisher_marg): the same arguments,
        ``F_st = 1/2 tr(Kt^-1 K_s Kt^-1 K_t)`` and ``F_mu = 1^T Kt^-1 1`` with ``Kt = K + H Lambda H^T`` -- the information of
        the likelihood ``lnlike_marg`` returns (the basis does not depend on any parameter: ``K_t`` is the plain one).  A
        negative hyper-parameter, a ``K`` that is not positive definite or an ``M`` that does not factor gives NaN in every
        entry."""
        if getattr(self, "_baseline", None) is None:
            raise _lib.PsoapError("fisher_marg: call set_baseline first")
        return self._fisher("psoap_chunk_fisher_marg", lwls, gp, tan_gp, tan_lwl, want_mu)

    def fisher_release(self):
        """Free the Fisher workspace (24 Npad^2 bytes); the next ``fisher`` allocates it again."""
        check(self._L.psoap_chunk_fisher_release(self._h), "psoap_chunk_fisher_release")

    def fisher_vel(self, lwls, gp, epoch_index, n_epochs: int | None = None) -> np.ndarray:
        """Fisher information of the per-epoch radial velocities at ``lwls`` (c, N), ``gp`` (2c,) (include/psoap_gp.h:
        psoap_chunk_fisher_vel): ``epoch_index`` (N,) with values in ``[0, n_epochs)``, any pixel order (``n_epochs``
        defaults to ``max(epoch_index) + 1``) -> ``F (c E, c E)``, row ``k * E + e`` as ``grad_vel``, symmetric bit for bit:
        what ``fisher`` gives for the ``c E`` tangents ``dx = -1/c_kms`` on component k, epoch e, for any number of epochs.
        The information of the velocities AT FIXED hyper-parameters; it has ``c`` null directions, the constant shift of
        each component; an epoch without pixels gives an exactly-zero row and column.  A negative hyper-parameter or a
        matrix that is not positive definite gives NaN in every entry.  Always under the plain ``K``, also on a handle with
        a baseline."""
        lwls = as_f64(np.atleast_2d(lwls))
        c = lwls.shape[0]
        lwls = as_f64(lwls, (c, self.N))
        gp = as_f64(gp, (2 * c,))
        ep = np.ascontiguousarray(epoch_index, dtype=np.int32)
        if ep.shape != (self.N,):
            raise ValueError("epoch_index must have shape (N,)")
        ne = int(ep.max()) + 1 if n_epochs is None else int(n_epochs)
        F = np.empty((c * max(ne, 0),) * 2)
        check(self._L.psoap_chunk_fisher_vel(self._h, c, dptr(lwls), dptr(gp), ne, ep.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                             dptr(F)), "psoap_chunk_fisher_vel")
        return F

    def fisher_vel_release(self):
        """Free the workspace of ``fisher_vel`` beyond the Fisher workspace's K^-1 (16 c Npad^2 bytes and the bin sums) and
        that of ``info_vel``; the next call allocates it again."""
        check(self._L.psoap_chunk_fisher_vel_release(self._h), "psoap_chunk_fisher_vel_release")

    def info_vel(self, lwls, gp, epoch_index, n_epochs: int | None = None, mu_GP: float = 1.0, marg: bool = False):
        """Value, gradient, expected and OBSERVED information of the per-epoch radial velocities from one factorisation
        (include/psoap_gp.h: psoap_chunk_info_vel), arguments as ``fisher_vel`` -> ``(lnp, grad (c, E), F (c E, c E),
        J (c E, c E))``: ``lnp`` as ``lnlike``, ``grad = dlnL/dv`` (``covariance.velocity_gradient`` of ``lnlike_grad``),
        ``F`` the bits of ``fisher_vel`` and ``J = -d2 lnL / dv dv`` at the handle's flux, ``E[J] = F``, symmetric bit for
        bit, with the ``c`` null directions of ``F``.  ``marg``: everything under the baseline of ``set_baseline`` (``lnp``
        as ``lnlike_marg``).  A negative hyper-parameter or a matrix that is not positive definite gives ``-inf`` and NaN in
        every entry of the three arrays."""
        lwls = as_f64(np.atleast_2d(lwls))
        c = lwls.shape[0]
        lwls = as_f64(lwls, (c, self.N))
        gp = as_f64(gp, (2 * c,))
        ep = np.ascontiguousarray(epoch_index, dtype=np.int32)
        if ep.shape != (self.N,):
            raise ValueError("epoch_index must have shape (N,)")
        if marg and getattr(self, "_baseline", None) is None:
            raise _lib.PsoapError("info_vel: call set_baseline first")
        ne = int(ep.max()) + 1 if n_epochs is None else int(n_epochs)
        T = c * max(ne, 0)
        lnp, g, F, J = np.empty(1), np.empty(T), np.empty((T, T)), np.empty((T, T))
        check(self._L.psoap_chunk_info_vel(self._h, int(bool(marg)), c, dptr(lwls), dptr(gp), float(mu_GP), ne,
                                           ep.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), dptr(lnp), dptr(g), dptr(F), dptr(J)),
              "psoap_chunk_info_vel")
        return float(lnp[0]), g.reshape(c, max(ne, 0)), F, J

    def loo(self, lwls, gp, mu_GP: float = 1.0, epoch_index=None, n_epochs: int | None = None) -> "LooResult":
        """Leave-one-out cross-validation of the likelihood at ``lwls`` (c, N), ``gp`` (2c,) (include/psoap_gp.h:
        psoap_chunk_loo): every pixel predicted from all the others and, with ``epoch_index`` (N,), every epoch from all the
        other epochs.  Every epoch's pixels must be one contiguous run (the order of ``Chunk.apply_mask``); ``n_epochs``
        defaults to ``max(epoch_index) + 1``.  A negative hyper-parameter or a matrix that is not positive definite gives
        ``lnp = -inf`` and NaN in every other floating field.  Always under the plain ``K``, also on a handle with a
        baseline: ``loo_marg`` is the form under ``K + H Lambda H^T``."""
        return self._loo("psoap_chunk_loo", lwls, gp, mu_GP, epoch_index, n_epochs)

    def _loo(self, entry, lwls, gp, mu_GP, epoch_index, n_epochs, tau=None, qp=None):
        """the body of ``loo``, ``loo_marg``, ``loo_tv`` and ``loo_qp``: ``entry`` names the library's function, which with ``tau``
        takes it after ``gp`` and with ``qp = (gamma, period)`` those two behind ``tau``"""
        lwls = as_f64(np.atleast_2d(lwls))
        c = lwls.shape[0]
        lwls = as_f64(lwls, (c, self.N))
        gp = as_f64(gp, (2 * c,))
        hyper = [as_f64(np.atleast_1d(as_f64(v)), (c,)) for v in (() if tau is None else (tau,)) + (() if qp is None else tuple(qp))]
        after_gp = tuple(dptr(v) for v in hyper)
        N = self.N
        lnp, logp = np.empty(1), np.empty(1)
        mean, var, plogp = np.empty(N), np.empty(N), np.empty(N)
        if epoch_index is None:
            ep, ne, resid, chi2, elogp, npix = None, 0, None, None, None, None
        else:
            ep = np.ascontiguousarray(epoch_index, dtype=np.int32)
            if ep.shape != (N,):
                raise ValueError("epoch_index must have shape (N,)")
            ne = int(ep.max()) + 1 if n_epochs is None else int(n_epochs)
            resid, chi2, elogp, npix = np.empty(N), np.empty(max(ne, 0)), np.empty(max(ne, 0)), np.empty(max(ne, 0), dtype=np.int32)
        i32 = ctypes.POINTER(ctypes.c_int32)
        check(getattr(self._L, entry)(self._h, c, dptr(lwls), dptr(gp), *after_gp, float(mu_GP),
                                      None if ep is None else ep.ctypes.data_as(i32), ne, dptr(lnp), dptr(logp), dptr(mean),
                                      dptr(var), dptr(plogp), None if ep is None else dptr(resid),
                                      None if ep is None else dptr(chi2), None if ep is None else dptr(elogp),
                                      None if ep is None else npix.ctypes.data_as(i32)), entry)
        return LooResult(float(lnp[0]), float(logp[0]), mean, var, plogp, self.fl, resid, chi2, elogp, npix)

    def loo_marg(self, lwls, gp, mu_GP: float = 1.0, epoch_index=None, n_epochs: int | None = None) -> "LooResult":
        """``loo`` under the baseline of ``set_baseline`` (include/psoap_gp.h: psoap_chunk_loo_marg): the same arguments and
        the same ``LooResult`` with ``A = (K + H Lambda H^T)^-1`` -- every pixel and every epoch predicted from the others
        with the continuum of each epoch integrated out, so an epoch whose only fault is a continuum offset within the
        prior is not an outlier.  ``lnp`` has the bits of ``lnlike_marg``.  ``epoch_index`` is the index of the epoch
        outputs; it need not be the baseline's."""
        if getattr(self, "_baseline", None) is None:
            raise _lib.PsoapError("loo_marg: call set_baseline first")
        return self._loo("psoap_chunk_loo_marg", lwls, gp, mu_GP, epoch_index, n_epochs)

    def loo_tv(self, lwls, gp, tau, mu_GP: float = 1.0, epoch_index=None, n_epochs: int | None = None) -> "LooResult":
        """``loo`` under the time-variable kernel of ``lnlike_tv`` (include/psoap_gp.h: psoap_chunk_loo_tv; needs
        ``set_times``): the same arguments with ``tau`` (c,) and the same ``LooResult`` with ``A = K^-1`` of that kernel --
        every pixel and every epoch predicted from the others by the model ``optimize_GP_timevar`` fits, so an epoch whose
        lines drifted as the fitted time scale allows is not an outlier.  ``lnp`` has the bits of ``lnlike_tv``; with every
        ``tau = inf`` every field has the bits of ``loo``.  ``tau <= 0`` or NaN gives ``lnp = -inf`` and NaN like a negative
        hyper-parameter; a handle with a baseline is refused."""
        return self._loo("psoap_chunk_loo_tv", lwls, gp, mu_GP, epoch_index, n_epochs, tau)

    def loo_qp(self, lwls, gp, tau, gamma, period, mu_GP: float = 1.0, epoch_index=None, n_epochs: int | None = None) -> "LooResult":
        """``loo_tv`` under the quasi-periodic kernel of ``lnlike_qp`` (include/psoap_gp.h: psoap_chunk_loo_qp; needs
        ``set_times``): ``gamma`` and ``period`` (c,) behind ``tau``, the same ``LooResult`` with ``A = K^-1`` of that kernel --
        the outlier search under the model ``optimize_GP_quasiperiodic`` fits.  ``lnp`` has the bits of ``lnlike_qp``; with every
        ``gamma = 0`` every field has the bits of ``loo_tv``.  A value that is no proposal gives ``lnp = -inf`` and NaN like a
        negative hyper-parameter; a handle with a baseline is refused."""
        return self._loo("psoap_chunk_loo_qp", lwls, gp, mu_GP, epoch_index, n_epochs, tau, (gamma, period))

    def loo_release(self):
        """Free the leave-one-out workspace (the packed epoch blocks); the next ``loo`` allocates it again."""
        check(self._L.psoap_chunk_loo_release(self._h), "psoap_chunk_loo_release")

    def set_baseline(self, order: int, x, epoch_index, n_epochs: int, prior_sd, weight=None):
        """A Chebyshev polynomial of degree ``order`` per epoch, with a Gaussian prior of standard deviations ``prior_sd``
        (order + 1,), to be integrated out by ``lnlike_marg`` (include/psoap_gp.h: psoap_chunk_set_baseline).  ``x`` (N,): the
        observed-frame ln-wavelengths; ``epoch_index`` (N,): every epoch's pixels one contiguous run; ``weight`` (N,): what
        multiplies the polynomial at each pixel -- ``None`` for an additive offset, the flux for the first-order form of a
        multiplicative correction.  A ``set_data`` after a baseline WITH weights makes ``lnlike_marg`` refuse until the
        baseline is set again."""
        x = as_f64(x, (self.N,))
        ep = np.ascontiguousarray(epoch_index, dtype=np.int32)
        if ep.shape != (self.N,):
            raise ValueError("epoch_index must have shape (N,)")
        sd = as_f64(np.atleast_1d(prior_sd))
        if sd.shape != (int(order) + 1,):
            raise ValueError("prior_sd must hold order + 1 values")
        w = None if weight is None else as_f64(weight, (self.N,))
        check(self._L.psoap_chunk_set_baseline(self._h, int(order), dptr(x), ep.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                               int(n_epochs), None if w is None else dptr(w), dptr(sd)),
              "psoap_chunk_set_baseline")
        self._baseline = (int(n_epochs), int(order))

    def lnlike_marg(self, lwls, gps, mu_GP: float = 1.0, want_beta: bool = False, want_cov: bool = False,
                    want_flux: bool = False):
        """The likelihood with the baseline of ``set_baseline`` integrated out (include/psoap_gp.h:
        psoap_chunk_lnlike_marg).  ``lwls`` (c, N) with ``gps`` (2c,) -> the value, or a ``MargResult`` when any of
        ``want_beta`` / ``want_cov`` / ``want_flux`` is set; ``lwls`` (B, c, N) with ``gps`` (B, 2c), B <= max_batch -> the same
        with a leading axis of B.  A negative hyper-parameter or a matrix that is not positive definite gives ``-inf`` and
        NaN in every other field."""
        return self._lnlike_marg("psoap_chunk_lnlike_marg", "lnlike_marg", lwls, gps, mu_GP, want_beta, want_cov, want_flux)

    def _lnlike_marg(self, entry, who, lwls, gps, mu_GP, want_beta, want_cov, want_flux, tau=None):
        """the body of ``lnlike_marg`` and ``lnlike_marg_tv``: ``entry`` names the library's function, which with ``tau`` takes
        it after ``gp``"""
        if getattr(self, "_baseline", None) is None:
            raise _lib.PsoapError(f"{who}: call set_baseline first")
        ne, order = self._baseline
        q = ne * (order + 1)
        single, B, c, lwls, gps = self._proposals(lwls, gps)
        taus = None if tau is None else as_f64(np.atleast_2d(as_f64(tau)), (B, c))      # (kept alive over the call)
        after_gp = () if taus is None else (dptr(taus),)
        more = want_beta or want_cov or want_flux
        lnp = np.empty(B)
        parts = np.empty((B, 4)) if more else None
        beta = np.empty((B, q)) if want_beta else None
        cov = np.empty((B, q, q)) if want_cov else None
        flc = np.empty((B, self.N)) if want_flux else None
        opt = lambda a: None if a is None else dptr(a)      # noqa: E731
        check(getattr(self._L, entry)(self._h, B, c, dptr(lwls), dptr(gps), *after_gp, float(mu_GP), dptr(lnp), opt(parts),
                                      opt(beta), opt(cov), opt(flc)), entry)
        if not more:
            return float(lnp[0]) if single else lnp
        if beta is not None:
            beta = beta.reshape(B, ne, order + 1)
        if single:
            return MargResult(float(lnp[0]), parts[0], None if beta is None else beta[0], None if cov is None else cov[0],
                              None if flc is None else flc[0])
        return MargResult(lnp, parts, beta, cov, flc)

    def lnlike_marg_grad(self, lwls, gps, mu_GP: float = 1.0):
        """Value and analytic gradient of the likelihood with the baseline of ``set_baseline`` integrated out
        (include/psoap_gp.h: psoap_chunk_lnlike_marg_grad): ``(lnp, grad_gp, grad_lwl, grad_mu)`` with the shapes of
        ``lnlike_grad`` -- ``lwls`` (c, N) with ``gps`` (2c,), or (B, c, N) with (B, 2c), any B.  ``lnp`` has the bits of
        ``lnlike_marg``.  A negative hyper-parameter or a matrix that is not positive definite gives ``-inf`` and NaN
        gradients."""
        if getattr(self, "_baseline", None) is None:
            raise _lib.PsoapError("lnlike_marg_grad: call set_baseline first")
        return self._lnlike_grad("psoap_chunk_lnlike_marg_grad", lwls, gps, mu_GP, None)      # (``parts``: not asked for)

    def lnprob_marg_grad(self, model_id: int, p_orb, gps, mu_GP: float = 1.0, want_vel: bool = False):
        """``lnprob_grad`` under the baseline of ``set_baseline`` (include/psoap_gp.h: psoap_chunk_lnprob_marg_grad; needs
        ``set_grid`` and the dates): the same arguments, the same tuple."""
        if getattr(self, "_baseline", None) is None:
            raise _lib.PsoapError("lnprob_marg_grad: call set_baseline first")
        return self._lnprob_grad("psoap_chunk_lnprob_marg_grad", True, model_id, p_orb, gps, mu_GP, want_vel)

    # -- the time-variable kernel under the baseline (include/psoap_gp.h: psoap_chunk_lnlike_marg_tv) ----------------
    def lnlike_marg_tv(self, lwls, gps, tau, mu_GP: float = 1.0, want_beta: bool = False, want_cov: bool = False,
                       want_flux: bool = False):
        """``lnlike_marg`` under the time-variable kernel of ``lnlike_tv`` (include/psoap_gp.h: psoap_chunk_lnlike_marg_tv;
        needs ``set_baseline`` and ``set_times``): ``tau`` (c,) or (B, c) beside ``gps``, the other arguments and the return
        value as ``lnlike_marg``.  With every ``tau = inf`` every field has the bits of ``lnlike_marg``; ``tau <= 0`` or NaN
        gives ``-inf`` and NaN like a negative hyper-parameter."""
        return self._lnlike_marg("psoap_chunk_lnlike_marg_tv", "lnlike_marg_tv", lwls, gps, mu_GP, want_beta, want_cov, want_flux,
                                 tau)

    def lnlike_marg_tv_grad(self, lwls, gps, tau, mu_GP: float = 1.0):
        """Value and analytic gradient of ``lnlike_marg_tv`` (include/psoap_gp.h: psoap_chunk_lnlike_marg_tv_grad):
        ``(lnp, grad_gp, grad_tau, grad_lwl, grad_mu)`` with the shapes of ``lnlike_tv_grad``, any B.  ``lnp`` has the bits
        of ``lnlike_marg_tv``; with every ``tau = inf`` the other four outputs have the bits of ``lnlike_marg_grad`` and
        ``grad_tau`` is exactly 0.  ``tau <= 0`` or NaN, a negative hyper-parameter or a matrix that does not factor gives
        ``-inf`` and NaN gradients for that proposal."""
        if getattr(self, "_baseline", None) is None:
            raise _lib.PsoapError("lnlike_marg_tv_grad: call set_baseline first")
        single, B, c, lwls, gps = self._proposals(lwls, gps)
        taus = as_f64(np.atleast_2d(as_f64(tau)), (B, c))
        lnp, g_gp, g_tau, g_lwl, g_mu = np.empty(B), np.empty((B, 2 * c)), np.empty((B, c)), np.empty((B, c, self.N)), np.empty(B)
        check(self._L.psoap_chunk_lnlike_marg_tv_grad(self._h, B, c, dptr(lwls), dptr(gps), dptr(taus), float(mu_GP), dptr(lnp),
                                                      None, dptr(g_gp), dptr(g_tau), dptr(g_lwl), dptr(g_mu)),
              "psoap_chunk_lnlike_marg_tv_grad")      # (``parts``: not asked for)
        if single:
            return float(lnp[0]), g_gp[0], g_tau[0], g_lwl[0], float(g_mu[0])
        return lnp, g_gp, g_tau, g_lwl, g_mu

    def fisher_marg_tv(self, lwls, gp, tau, tan_gp, tan_tau=None, tan_lwl=None, want_mu: bool = False):
        """``fisher_tv`` under the baseline of ``set_baseline`` (include/psoap_gp.h: psoap_chunk_fisher_marg_tv): the same
        arguments, ``F_st = 1/2 tr(Kt^-1 K_s Kt^-1 K_t)`` with ``Kt = K_tv + H Lambda H^T`` -- the information of the
        likelihood ``lnlike_marg_tv`` returns.  With every ``tau = inf`` it has the bits of ``fisher_marg``, and a tangent
        with nothing but a time-scale part gives an exactly-zero row and column."""
        if getattr(self, "_baseline", None) is None:
            raise _lib.PsoapError("fisher_marg_tv: call set_baseline first")
        return self._fisher("psoap_chunk_fisher_marg_tv", lwls, gp, tan_gp, tan_lwl, want_mu, tau, tan_tau)

    def marg_release(self):
        """Free the device side of the baseline and the workspace of ``lnlike_marg`` and ``lnlike_marg_grad`` beyond the
        gradient's; the baseline stays set and the next call allocates everything again."""
        check(self._L.psoap_chunk_marg_release(self._h), "psoap_chunk_marg_release")

    def upload(self, lwls, gps, mu_GP: float = 1.0):
        lwls = as_f64(lwls)
        B, c, _ = lwls.shape
        lwls = as_f64(lwls, (B, c, self.N))
        gps = as_f64(gps, (B, 2 * c))
        check(self._L.psoap_batch_upload(self._h, B, c, dptr(lwls), dptr(gps), float(mu_GP)), "psoap_batch_upload")
        self._B = B

    def upload_velocities(self, velocities, gps, mu_GP: float = 1.0):
        vel = as_f64(velocities)
        if vel.ndim != 3 or vel.shape[2] != self.n_epochs:
            raise ValueError("velocities must have shape (B, c, n_epochs); call set_grid first")
        B, c, _ = vel.shape
        gps = as_f64(gps, (B, 2 * c))
        check(self._L.psoap_batch_upload_velocities(self._h, B, c, dptr(vel), dptr(gps), float(mu_GP)),
              "psoap_batch_upload_velocities")
        self._B = B

    def set_tau(self, tau):
        """Time scales ``tau`` (B, c) in days for the upload that is pending (``upload``, ``upload_velocities`` or a
        ``ChunkWorker.upload_*``; include/psoap_gp.h: psoap_batch_set_tau; needs ``set_times``): ``eval`` then evaluates the
        time-variable kernel of ``lnlike_tv`` on the staged path, whatever ``set_mode`` says.  ``inf`` is the static model
        (the bits of the same upload under ``set_mode("staged")``); ``tau <= 0`` or NaN gives ``-inf`` for that proposal
        alone.  The next upload clears the time scales.  Refused without a pending upload, for another shape, without
        times, with an open stream or on a handle with a baseline."""
        tau = as_f64(np.atleast_2d(as_f64(tau)))
        if tau.ndim != 2:
            raise ValueError("tau must have shape (B, c)")
        B, c = tau.shape
        check(self._L.psoap_batch_set_tau(self._h, B, c, dptr(tau)), "psoap_batch_set_tau")

    def lnprob_tv_grad(self, model_id: int, p_orb, gps, tau, mu_GP: float = 1.0, want_vel: bool = False):
        """``lnprob_grad`` under the time-variable kernel of ``lnlike_tv`` (include/psoap_gp.h: psoap_chunk_lnprob_tv_grad;
        needs ``set_grid``, the dates and ``set_times``): ``tau`` (B, c) beside ``gps`` ->
        ``(lnp (B,), grad_orb (B, n_orb), grad_gp (B, 2c), grad_tau (B, c), grad_mu (B,))``, with ``grad_vel`` appended when
        ``want_vel``.  With every ``tau = inf`` ``grad_tau`` is exactly 0.  A faster-than-light proposal, a negative
        hyper-parameter, ``tau <= 0`` or NaN, or a matrix that is not positive definite gives ``-inf`` and NaN gradients
        for that proposal."""
        return self._lnprob_grad("psoap_chunk_lnprob_tv_grad", False, model_id, p_orb, gps, mu_GP, want_vel, tau)

    def lnprob_marg_tv_grad(self, model_id: int, p_orb, gps, tau, mu_GP: float = 1.0, want_vel: bool = False):
        """``lnprob_tv_grad`` under the baseline of ``set_baseline`` (include/psoap_gp.h: psoap_chunk_lnprob_marg_tv_grad):
        the same arguments, the same tuple."""
        if getattr(self, "_baseline", None) is None:
            raise _lib.PsoapError("lnprob_marg_tv_grad: call set_baseline first")
        return self._lnprob_grad("psoap_chunk_lnprob_marg_tv_grad", True, model_id, p_orb, gps, mu_GP, want_vel, tau)

    def eval(self):
        check(self._L.psoap_batch_eval(self._h), "psoap_batch_eval")

    def fetch(self) -> np.ndarray:
        out = np.empty(self._B)
        check(self._L.psoap_batch_fetch(self._h, dptr(out)), "psoap_batch_fetch")
        return out

    def sync(self):
        check(self._L.psoap_chunk_sync(self._h), "psoap_chunk_sync")

    # -- streamed evaluation (include/psoap_gp.h: psoap_stream_*) ----------------------------------------
    def stream_open(self, c: int, lanes: int | None = None, scheme: int = -1):
        """Keep ONE launch of the persistent kernel resident: ``stream_submit`` hands proposals to free lanes,
        ``stream_fetch`` returns their lnprob while the other lanes keep the device busy (the back-to-back iterations
        of /root/reference/psoap/sample_parallel.py:434-438).  Batch calls are refused until ``stream_close``."""
        lanes = self.max_batch if lanes is None else int(lanes)
        check(self._L.psoap_stream_open(self._h, int(c), lanes, int(scheme)), "psoap_stream_open")
        self._stream_c = int(c)
        self.stream_lanes = lanes

    def stream_submit(self, lwls, gps, mu_GP: float = 1.0) -> np.ndarray:
        """``lwls`` (n, c, N), ``gps`` (n, 2c) -> tickets (n,) int64"""
        lwls = as_f64(lwls)
        if lwls.ndim != 3 or lwls.shape[1:] != (self._stream_c, self.N):
            raise ValueError(f"lwls must have shape (n, {self._stream_c}, {self.N})")
        n = lwls.shape[0]
        gps = as_f64(gps, (n, 2 * self._stream_c))
        tickets = np.empty(n, dtype=np.int64)
        check(self._L.psoap_stream_submit(self._h, n, dptr(lwls), dptr(gps), float(mu_GP),
                                          tickets.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))), "psoap_stream_submit")
        return tickets

    def stream_submit_velocities(self, velocities, gps, mu_GP: float = 1.0) -> np.ndarray:
        """``velocities`` (n, c, n_epochs): the resident launch shifts the chunk's grid itself (``set_grid`` before
        ``stream_open``)"""
        vel = as_f64(velocities)
        if vel.ndim != 3 or vel.shape[1:] != (self._stream_c, self.n_epochs):
            raise ValueError(f"velocities must have shape (n, {self._stream_c}, {self.n_epochs}); call set_grid first")
        n = vel.shape[0]
        gps = as_f64(gps, (n, 2 * self._stream_c))
        tickets = np.empty(n, dtype=np.int64)
        check(self._L.psoap_stream_submit_velocities(self._h, n, dptr(vel), dptr(gps), float(mu_GP),
                                                     tickets.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))),
              "psoap_stream_submit_velocities")
        return tickets

    def stream_submit_orbits(self, model_id: int, p_orb, gps, mu_GP: float = 1.0) -> np.ndarray:
        """orbital parameters (n, n_orb): Kepler solve, |v| >= c rule and Doppler shift inside the resident launch"""
        p_orb = as_f64(np.atleast_2d(p_orb))
        n = p_orb.shape[0]
        from .utils import MODEL_ID, n_params_orb
        width = {MODEL_ID[m]: n_params_orb[m] for m in MODEL_ID}.get(int(model_id))
        if width is None or p_orb.shape[1] != width:       # (the library copies exactly that many doubles per proposal)
            raise ValueError(f"p_orb must have shape (n, {width}) for orbit model {model_id}")
        gps = as_f64(gps, (n, 2 * self._stream_c))
        tickets = np.empty(n, dtype=np.int64)
        check(self._L.psoap_stream_submit_orbits(self._h, n, int(model_id), dptr(p_orb), dptr(gps), float(mu_GP),
                                                 tickets.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))),
              "psoap_stream_submit_orbits")
        return tickets

    def stream_fetch(self, tickets) -> np.ndarray:
        tickets = np.ascontiguousarray(tickets, dtype=np.int64)
        out = np.empty(tickets.shape[0])
        check(self._L.psoap_stream_fetch(self._h, tickets.shape[0],
                                         tickets.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), dptr(out)),
              "psoap_stream_fetch")
        return out

    def stream_wait_any(self, tickets) -> int:
        """index of a ticket whose result has arrived (blocks until one has)"""
        tickets = np.ascontiguousarray(tickets, dtype=np.int64)
        w = ctypes.c_int(-1)
        check(self._L.psoap_stream_wait_any(self._h, tickets.shape[0],
                                            tickets.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), ctypes.byref(w)),
              "psoap_stream_wait_any")
        return int(w.value)

    def stream_ready(self, ticket: int) -> bool:
        r = ctypes.c_int(0)
        check(self._L.psoap_stream_ready(self._h, int(ticket), ctypes.byref(r)), "psoap_stream_ready")
        return bool(r.value)

    def stream_stats(self) -> dict:
        a, b, c_, t = (ctypes.c_longlong(0) for _ in range(4))
        sch = ctypes.c_int(0)
        check(self._L.psoap_stream_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c_), ctypes.byref(sch),
                                         ctypes.byref(t)), "psoap_stream_stats")
        return {"launches": a.value, "submitted": b.value, "completed": c_.value, "scheme": sch.value,
                "tasks_per_matrix": t.value}

    def stream_pause(self):
        """The resident launch leaves now (after what is in flight) and the device is free; the next submit relaunches."""
        check(self._L.psoap_stream_pause(self._h), "psoap_stream_pause")

    def stream_last_launch(self) -> dict:
        """the resident launch ``stream_pause`` ended last: duration by HIP events on its stream, matrices completed"""
        ms, n = ctypes.c_double(0.0), ctypes.c_longlong(0)
        check(self._L.psoap_stream_last_launch(self._h, ctypes.byref(ms), ctypes.byref(n)), "psoap_stream_last_launch")
        return {"ms": ms.value, "matrices": n.value}

    def stream_close(self):
        check(self._L.psoap_stream_close(self._h), "psoap_stream_close")

    def predict(self, mode: int, lwls, lwls_predict, mu_c, gp, want_sigma=True):
        """``predict_*`` on this chunk's resident ``fl`` / ``sigma`` (include/psoap_gp.h: psoap_chunk_predict;
        mode 0 components, 1 sum, 2 predict_f).  The workspace stays with the handle.
        ``want_sigma``: True -> (mu, Sigma); "diag" -> (mu, diag(Sigma)) without ever forming Sigma
        (psoap_chunk_predict_var); False -> mu.  Always under the plain ``K``, also on a handle with a baseline:
        ``predict_marg`` is the form under ``K + H Lambda H^T``."""
        return self._predict("psoap_chunk_predict", mode, lwls, lwls_predict, mu_c, gp, want_sigma)

    def _predict(self, entry, mode, lwls, lwls_predict, mu_c, gp, want_sigma):
        """the body of ``predict`` and ``predict_marg``: ``entry`` names the library's function, ``entry + "_var"`` its
        mean-and-variances form"""
        lwls = as_f64(np.atleast_2d(lwls))
        pred = as_f64(np.atleast_2d(lwls_predict))
        c = lwls.shape[0]
        lwls = as_f64(lwls, (c, self.N))
        M = pred.shape[1]
        pred = as_f64(pred, (c, M))
        mu_c = as_f64(mu_c)
        gp = as_f64(gp, (2 * c,))
        R = c * M if mode == 0 else M
        mu = np.empty(R)
        status = ctypes.c_int(0)
        self._sigma_rows = 0           # (what predict_draw sizes its output by: the library keeps the record itself)
        if isinstance(want_sigma, str):
            if want_sigma != "diag":
                raise ValueError('want_sigma must be True, False or "diag"')
            var = np.empty(R)
            check(getattr(self._L, entry + "_var")(self._h, int(mode), c, M, dptr(lwls), dptr(pred), dptr(mu_c), dptr(gp),
                                                   dptr(mu), dptr(var), ctypes.byref(status)), entry + "_var")
            if status.value != 0:
                raise np.linalg.LinAlgError("data covariance matrix is not positive definite")
            return mu, var
        Sigma = np.empty((R, R)) if want_sigma else None
        check(getattr(self._L, entry)(self._h, int(mode), c, M, dptr(lwls), dptr(pred), dptr(mu_c), dptr(gp),
                                      dptr(mu), None if Sigma is None else dptr(Sigma), ctypes.byref(status)), entry)
        if status.value != 0:
            raise np.linalg.LinAlgError("data covariance matrix is not positive definite")
        if want_sigma:
            self._sigma_rows = R
        return (mu, Sigma) if want_sigma else mu

    def predict_marg(self, mode: int, lwls, lwls_predict, mu_c, gp, want_sigma=True):
        """``predict`` under the baseline of ``set_baseline`` (include/psoap_gp.h: psoap_chunk_predict_marg): the same
        arguments and return shapes, the conditional of the components under ``K + H Lambda H^T`` -- the continuum of
        every epoch integrated out, its uncertainty in ``Sigma`` / the variances, instead of a continuum frozen at its
        posterior mean.  Mode 0 with two or three components, mode 1 with two, mode 2 with one.  ``LinAlgError`` when ``K``
        is not positive definite (or the Gram matrix does not factor); ``PsoapError`` without a baseline."""
        return self._predict("psoap_chunk_predict_marg", mode, lwls, lwls_predict, mu_c, gp, want_sigma)

    def predict_tv(self, mode: int, lwls, lwls_predict, t_predict, mu_c, gp, tau, want_sigma=True):
        """``predict`` under the time-variable kernel of ``lnlike_tv`` (include/psoap_gp.h: psoap_chunk_predict_tv; needs
        ``set_times``): the component spectra at chosen dates.  A prediction point is ``(lwls_predict[k][m], t_predict[m])``:
        ``t_predict`` (M,) in days is shared by the components and has the constant removed that ``set_times``' times have;
        several dates are several runs of it (with the grid repeated), and ``Sigma`` then holds the covariance between the
        dates.  ``tau`` (c,); ``inf`` keeps a component static, and with every ``tau = inf`` the result has the bits of
        ``predict`` on the staged route.  Return forms as ``predict``; ``predict_draw`` works after a call that returned
        ``Sigma``.  Mode 0 with two or three components, mode 1 with two, mode 2 with one.  ``LinAlgError`` when ``K`` is not
        positive definite; ``PsoapError`` without times, with a baseline or an open stream, for a ``tau`` that is no time
        scale or a ``t_predict`` that is not finite."""
        lwls = as_f64(np.atleast_2d(lwls))
        pred = as_f64(np.atleast_2d(lwls_predict))
        c = lwls.shape[0]
        lwls = as_f64(lwls, (c, self.N))
        M = pred.shape[1]
        pred = as_f64(pred, (c, M))
        t_pred = as_f64(np.atleast_1d(as_f64(t_predict)), (M,))
        mu_c = as_f64(mu_c)
        gp = as_f64(gp, (2 * c,))
        tau = as_f64(np.atleast_1d(as_f64(tau)), (c,))
        R = c * M if mode == 0 else M
        mu = np.empty(R)
        status = ctypes.c_int(0)
        self._sigma_rows = 0
        if isinstance(want_sigma, str):
            if want_sigma != "diag":
                raise ValueError('want_sigma must be True, False or "diag"')
            second = np.empty(R)
            entry = "psoap_chunk_predict_tv_var"
        else:
            second = np.empty((R, R)) if want_sigma else None
            entry = "psoap_chunk_predict_tv"
        check(getattr(self._L, entry)(self._h, int(mode), c, M, dptr(lwls), dptr(pred), dptr(t_pred), dptr(mu_c), dptr(gp), dptr(tau),
                                      dptr(mu), None if second is None else dptr(second), ctypes.byref(status)), entry)
        if status.value != 0:
            raise np.linalg.LinAlgError("data covariance matrix is not positive definite")
        if second is not None and second.ndim == 2:
            self._sigma_rows = R
        return mu if second is None else (mu, second)

    def predict_draw(self, n_draws: int, seed=None, z=None, nugget: float = 1e-8) -> np.ndarray:
        """``n_draws`` spectra from the posterior of the last ``predict`` / ``predict_marg`` call of this handle that returned
        ``Sigma`` (include/psoap_gp.h: psoap_chunk_predict_draw) -> ``(n_draws, R)``, ``R`` that call's rows:
        ``mu + U^T z_d`` with ``U^T U = Sigma + nugget I``, i.e. draws from ``N(mu, Sigma + nugget I)`` -- not from
        ``N(mu, Sigma)``: ``Sigma`` on a fine grid is numerically rank deficient and the Cholesky factor needs the nugget
        (an absolute variance in flux^2).  ``seed``: the normals come from the device's counter-based generator (element
        ``i`` of draw ``d`` depends on ``(seed, d, i)`` alone).  ``z`` ``(n_draws, R)``: these normals instead.  One of the
        two.  ``mu`` and ``Sigma`` stay on the device: call again with another seed, number of draws or nugget without a
        new predict.  ``LinAlgError`` when ``Sigma + nugget I`` does not factor; ``PsoapError`` without such a predict call."""
        if (seed is None) == (z is None):
            raise ValueError("predict_draw takes a seed or z (n_draws, R), one of the two")
        D = int(n_draws)
        if z is not None:
            z = as_f64(np.atleast_2d(z))
            if z.shape[0] != D:
                raise ValueError(f"z must hold {D} rows, one per draw; got {z.shape}")
            R = z.shape[1]
        else:
            R = self._sigma_rows
            seed = int(seed)
            if not 0 <= seed < 2 ** 64:
                raise ValueError("seed must be an unsigned 64-bit integer")
        if z is not None and self._sigma_rows and R != self._sigma_rows:
            raise ValueError(f"z must have {self._sigma_rows} columns, the rows of the last predict call; got {R}")
        out = np.empty((max(D, 0), max(R, 0)))
        status = ctypes.c_int(0)
        check(self._L.psoap_chunk_predict_draw(self._h, D, ctypes.c_ulonglong(0 if seed is None else seed),
                                               None if z is None else dptr(z), float(nugget), dptr(out), ctypes.byref(status)),
              "psoap_chunk_predict_draw")
        if status.value != 0:
            raise np.linalg.LinAlgError("Sigma + nugget I is not positive definite")
        return out

    # -- mixture moments over chain samples (include/psoap_gp.h: psoap_chunk_mix_*) -------------------------------
    def mix_begin(self, mode: int, lwls_predict, mu_c, s_max: int, want_sigma: bool = True, marg: bool = False):
        """Start a mixture of up to ``s_max`` parameter samples on this handle: all of them are predicted on ``lwls_predict``
        (c, M) with prior means ``mu_c``, as ``predict`` (``marg``: as ``predict_marg``, under the current baseline) takes
        them.  ``want_sigma=False`` accumulates the variances only.  The accumulators start at zero."""
        pred = as_f64(np.atleast_2d(lwls_predict))
        c, M = pred.shape
        mu_c = as_f64(np.atleast_1d(mu_c))
        if mu_c.shape[0] < (c if mode == 0 else 1):
            raise ValueError("mu_c must hold one prior mean per component in mode 0, else one")
        check(self._L.psoap_chunk_mix_begin(self._h, int(bool(marg)), int(mode), c, M, dptr(pred), dptr(mu_c), int(s_max),
                                            int(bool(want_sigma))), "psoap_chunk_mix_begin")
        self._mix = (c, c * M if mode == 0 else M, bool(want_sigma))

    def mix_add(self, lwls, gp, weight: float = 1.0) -> bool:
        """Predict one sample -- rest-frame grids ``lwls`` (c, N), hyper-parameters ``gp`` (2c,) -- and fold its mean and
        ``Sigma`` (or variances) into the mixture with ``weight``; nothing of size R^2 leaves the device.  -> True, or False
        when the sample's data covariance is not positive definite: it is then not folded and the mixture is as before.
        After a folded sample of a full-``Sigma`` mixture ``predict_draw`` draws from that sample's posterior."""
        c, R, full = getattr(self, "_mix", None) or (np.atleast_2d(lwls).shape[0], 0, False)
        lwls = as_f64(np.atleast_2d(lwls), (c, self.N))
        gp = as_f64(gp, (2 * c,))
        status = ctypes.c_int(0)
        self._sigma_rows = 0
        check(self._L.psoap_chunk_mix_add(self._h, dptr(lwls), dptr(gp), float(weight), ctypes.byref(status)), "psoap_chunk_mix_add")
        if status.value == 0 and full:
            self._sigma_rows = R
        return status.value == 0

    def mix_finish(self, want_sigma=None) -> dict:
        """The moments of what has been folded so far (it only reads the accumulators: call it again, or go on adding):
        ``mu`` (R,), ``Sigma`` (R, R) or None, ``var_within`` and ``var_between`` (R,) with ``diag(Sigma) = var_within +
        var_between``, ``n_folded`` and the sum of the weights ``W``.  ``want_sigma=False`` on a full-``Sigma`` mixture spares
        the download."""
        c, R, full = getattr(self, "_mix", None) or (0, 1, False)
        want = full if want_sigma is None else bool(want_sigma)
        mu, vw, vb = np.empty(R), np.empty(R), np.empty(R)
        Sigma = np.empty((R, R)) if want else None
        n, W = ctypes.c_int(0), ctypes.c_double(0.0)
        check(self._L.psoap_chunk_mix_finish(self._h, dptr(mu), None if Sigma is None else dptr(Sigma), dptr(vw), dptr(vb),
                                             ctypes.byref(n), ctypes.byref(W)), "psoap_chunk_mix_finish")
        return {"mu": mu, "Sigma": Sigma, "var_within": vw, "var_between": vb, "n_folded": n.value, "W": W.value}

    def mix_release(self):
        """End the mixture and free its buffers (the predict workspace stays)."""
        self._mix = None
        check(self._L.psoap_chunk_mix_release(self._h), "psoap_chunk_mix_release")

    def predict_release(self):
        """Free the predict workspace (``predict``, ``predict_marg`` and ``predict_draw`` share it); the next call allocates
        it again."""
        self._sigma_rows = 0
        check(self._L.psoap_chunk_predict_release(self._h), "psoap_chunk_predict_release")

    def predict_timings(self) -> dict:
        t = _lib.PredictTimings()
        check(self._L.psoap_chunk_predict_timings(self._h, ctypes.byref(t)), "psoap_chunk_predict_timings")
        return t.as_dict()

    def timings(self) -> dict:
        t = Timings()
        check(self._L.psoap_chunk_get_timings(self._h, ctypes.byref(t)), "psoap_chunk_get_timings")
        out = {"total_ms": t.total_ms}
        for k, name in enumerate(K_NAMES):
            out[name] = {"ms": t.ms[k], "launches": int(t.launches[k]), "flops": t.flops[k], "bytes": t.bytes[k]}
        return out

    def sky_stats(self) -> dict:
        """The skyline of the last evaluation (include/psoap_gp.h: psoap_chunk_sky_stats): tiles and tile-GEMM units of the
        list that ran against the dense ones, plan builds and plan-cache hits so far, whether the slot's skyline was read, and
        the units executed once every matrix's updates are clipped to its own envelope (PSOAP_SKY_CLIP=0: the planned ones),
        and the 16-row stages of those units that run once every update starts at its matrix's own first row group (8 per unit
        under PSOAP_SKY_FINE=0)."""
        names = ("tiles_planned", "tiles_dense", "units_planned", "units_dense", "plan_builds", "cache_hits", "skyline_on",
                 "units_clipped", "stages_clipped")
        out = (ctypes.c_longlong * len(names))()
        n = self._L.psoap_chunk_sky_stats(self._h, out, len(names))
        if n != len(names):
            raise _lib.PsoapError(f"psoap_chunk_sky_stats reports {n} fields, psoap_amd.chunk names {len(names)}")
        return dict(zip(names, (int(v) for v in out)))


class StreamPipeline:
    """``groups`` sub-ensembles of one walker ensemble in flight through a stream (``ChunkHandle.stream_open``): step k of
    group g is fetched and its successor submitted while the other groups keep the device busy -- neither group's
    proposals depend on another group's accept / reject (red / black halves of an ensemble; independent chains), so
    the iteration order of /root/reference/psoap/sample_parallel.py:434-438 is kept per group.

        pipe = StreamPipeline(h, c, walkers=32, groups=2)
        pipe.start(lwls, gps)                    # all groups submitted (group g delayed by g / groups of a period)
        for k in range(steps):
            lnp = pipe.step(next_lwls, next_gps) # per group: fetch, then submit the same rows of the next proposals
        last = pipe.drain()

    ``step`` returns the lnprob of the proposals submitted one call earlier, in walker order."""

    def __init__(self, handle: ChunkHandle, c: int, walkers: int, groups: int = 2, scheme: int = -1, submit=None):
        """``submit``: what turns the rows of a group into tickets -- default ``handle.stream_submit(lwls, gps, mu_GP)``;
        e.g. ``handle.stream_submit_velocities`` or ``ChunkWorker.stream_submit`` (orbital parameters in): ``start`` /
        ``step`` then take that callable's array arguments, each sliced by the group's rows."""
        if walkers % groups:
            raise ValueError("walkers must be a multiple of groups")
        self.h, self.c, self.walkers, self.groups = handle, int(c), int(walkers), int(groups)
        self.rows = [slice(g * walkers // groups, (g + 1) * walkers // groups) for g in range(groups)]
        handle.stream_open(c, walkers, scheme)
        self._submit = submit if submit is not None else handle.stream_submit
        self.tickets = [None] * groups
        self.period = None             # seconds per ensemble step, measured by calibrate()

    def _go(self, g, arrays, mu_GP):
        r = self.rows[g]
        self.tickets[g] = self._submit(*[a[r] for a in arrays], mu_GP)

    def calibrate(self, *arrays, mu_GP: float = 1.0, steps: int = 2) -> float:
        """Seconds per ensemble step in the steady state (a few untimed steps): what the start-up stagger is set from."""
        import time
        self.start(*arrays, mu_GP=mu_GP, stagger=0.0)
        self.step(*arrays, mu_GP=mu_GP)
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step(*arrays, mu_GP=mu_GP)
        self.period = (time.perf_counter() - t0) / steps
        self.drain()
        return self.period

    def start(self, *arrays, mu_GP: float = 1.0, stagger: float | None = None):
        """Submit every group, group g a little later than group g - 1, so that the groups end up ``1 / groups`` of a
        period apart and their first block rows and tails never coincide.  While only k groups are in flight they have
        the whole device and advance ``groups / k`` times as fast as in the steady state: the k-th interval is
        ``k * period / groups**2`` long (two groups: the second a QUARTER of a period after the first, which is then
        half way through).  ``stagger``: that unit, ``period / groups**2``, in seconds (default from ``calibrate``)."""
        import time
        if stagger is None:
            stagger = (self.period or 0.0) / self.groups ** 2
        t0 = time.perf_counter()
        for g in range(self.groups):
            while time.perf_counter() - t0 < 0.5 * g * (g + 1) * stagger:
                pass
            self._go(g, arrays, mu_GP)

    def step(self, *arrays, mu_GP: float = 1.0, between=None) -> np.ndarray:
        """``between(g, rows, lnp_rows)``: called for every group after its results are in and BEFORE its successor is
        submitted -- where a sampler decides accept / reject, and where several ranks exchange the group's lnprobs
        (the gather of /root/reference/psoap/sample_parallel.py:378-387: the next proposals depend on the chunk sum)."""
        out = np.empty(self.walkers)
        for g, r in enumerate(self.rows):
            out[r] = self.h.stream_fetch(self.tickets[g])
            if between is not None:
                between(g, r, out[r])
            self._go(g, arrays, mu_GP)
        return out

    def step_any_order(self, *arrays, mu_GP: float = 1.0) -> np.ndarray:
        """The same step with the groups taken in the order in which they COMPLETE (``groups == walkers``: every chain
        resubmitted the moment its result is there -- independent chains): no lane waits for the slowest matrix of a
        group.  Every group is fetched and resubmitted exactly once per call."""
        out = np.empty(self.walkers)
        left = list(range(self.groups))
        while left:
            # (a group is complete when its last ticket is: wait on one ticket per group)
            k = self.h.stream_wait_any([self.tickets[g][-1] for g in left]) if len(left) > 1 else 0
            g = left.pop(k)
            r = self.rows[g]
            out[r] = self.h.stream_fetch(self.tickets[g])
            self._go(g, arrays, mu_GP)
        return out

    def drain(self, between=None) -> np.ndarray:
        out = np.empty(self.walkers)
        for g, r in enumerate(self.rows):
            out[r] = self.h.stream_fetch(self.tickets[g])
            if between is not None:
                between(g, r, out[r])
            self.tickets[g] = None
        return out

    def close(self):
        self.h.stream_close()


class ChunkGroup:
    """Several chunk handles (one device, one component count; sizes may differ) evaluated by ONE launch
    of the persistent kernel over the heterogeneous batch -- the one-GPU form of the reference's one
    worker process per chunk (sample_parallel.py:258-278).  ``upload*`` on every member, ``eval()``,
    ``fetch()`` on every member.  Small chunks cannot fill the device one at a time; together the
    matrices of all chunks hide each other's dependency chains."""

    def __init__(self, handles):
        self.handles = list(handles)
        if not self.handles:
            raise ValueError("a group needs at least one chunk handle")
        self._L = _lib.load()
        self._g = ctypes.c_void_p()
        arr = (ctypes.c_void_p * len(self.handles))(*[h._h for h in self.handles])
        check(self._L.psoap_group_create(ctypes.byref(self._g), arr, len(self.handles)), "psoap_group_create")

    def eval(self):
        check(self._L.psoap_group_eval(self._g), "psoap_group_eval")

    def stats(self) -> dict:
        """task-list builds (batch sizes changed) and record refreshes (a member changed its proposal slot) so far"""
        a, b = ctypes.c_longlong(0), ctypes.c_longlong(0)
        check(self._L.psoap_group_stats(self._g, ctypes.byref(a), ctypes.byref(b)), "psoap_group_stats")
        return {"plan_builds": a.value, "record_refreshes": b.value}

    def close(self):
        if getattr(self, "_g", None) is not None and self._g:
            self._L.psoap_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def microbench(device: int | None = None) -> dict:
    """Measured ceilings of the device (libpsoap_bench.so, include/psoap_bench.h): never part of the product path."""
    L = _lib.load_bench()
    check = _lib.check_bench
    dev = _lib.default_device() if device is None else device
    tf = ctypes.c_double()
    w = ctypes.c_double()
    c = ctypes.c_double()
    check(L.psoap_microbench_mfma_f64(dev, ctypes.byref(tf)), "psoap_microbench_mfma_f64")
    check(L.psoap_microbench_hbm(dev, ctypes.byref(w), ctypes.byref(c)), "psoap_microbench_hbm")
    t1 = ctypes.c_double()
    t0 = ctypes.c_double()
    # variants 9 / 8: the production engine (LDS-DMA staging) on L2-resident / HBM-streamed operands
    check(L.psoap_microbench_tile_engine(dev, 9, ctypes.byref(t1)), "psoap_microbench_tile_engine")
    check(L.psoap_microbench_tile_engine(dev, 8, ctypes.byref(t0)), "psoap_microbench_tile_engine")
    return {"mfma_f64_tflops": tf.value, "hbm_write_gbs": w.value, "hbm_copy_gbs": c.value,
            "tile_engine_l2_tflops": t1.value, "tile_engine_hbm_tflops": t0.value}
