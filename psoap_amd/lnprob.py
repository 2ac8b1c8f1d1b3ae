"""The per-chunk ``lnprob(p)`` of the parallel sampler with everything after the parameter
plumbing on the device.

``ChunkWorker.lnprob(p)`` reproduces ``Worker.lnprob`` (/root/reference/psoap/sample_parallel.py:168-198):
``convert_vector`` -> orbit velocities -> |v| >= c_kms -> -inf -> ``replicate_wls`` -> ``lnlike[model]``.
Orbit evaluation (batched Kepler solve), Doppler shift and likelihood run in the HIP library; per proposal
the host ships ``n_orb + 2c`` doubles and receives one.  ``lnprob_batch`` evaluates a whole ensemble.
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib
from ._lib import as_f64, check, dptr
from .chunk import ChunkHandle
from .utils import MODEL_ID, N_COMPONENTS, convert_vectors, convert_vectors_timevar, n_params_orb, registered_params, timevar_spec


class ChunkWorker:
    timevar = None      # (``{"fit", "tau"}`` on a worker made with ``timevar=...``)

    def __init__(self, model: str, lwl, fl, sigma, epoch_index, dates, fix_params=(), defaults=None,
                 max_batch: int = 1, device: int | None = None, soften: float = 1.0, baseline: dict | None = None,
                 timevar: dict | None = None):
        """lwl/fl/sigma: the chunk's masked, flattened arrays (N,); epoch_index (N,): epoch of each pixel;
        dates (n_epochs,): ``date1D``; ``soften`` scales sigma (sample_parallel.py:141).

        ``baseline = {"order": k, "sd": [s_0 .. s_k], "weight": "one" | "flux"}``: ``lnprob`` and ``lnprob_batch`` evaluate the
        likelihood with a Chebyshev polynomial of degree k per epoch integrated out (``ChunkHandle.lnlike_marg``) -- an
        additive offset ("one") or the polynomial times the flux ("flux") -- ``lnprob_grad*`` its gradient
        (``ChunkHandle.lnprob_marg_grad``), ``fisher*`` its Fisher information (``ChunkHandle.fisher_marg``) and ``loo*`` its
        leave-one-out cross-validation (``ChunkHandle.loo_marg``).  The split-phase and streamed entries
        (``upload_*``, ``stream_*``) evaluate the plain likelihood and refuse to run on such a worker.  ``None``: every
        path as it was.

        ``timevar = {"fit": [bool per component], "tau": [default per component, inf allowed], "times": None | (N,)}``: the
        time-variable kernel of ``ChunkHandle.lnlike_tv`` over the pixels' ``times`` in days (``None``:
        ``dates[epoch_index]`` minus its minimum).  A fitted vector is then the model's registered vector followed by one
        ``tau_c`` in days for every component with ``fit`` true, in component order (``utils.convert_vectors_timevar``); the
        other components stay at their default.  ``lnprob`` / ``lnprob_batch`` and the split-phase ``upload_*`` carry the
        time scales to the device (``ChunkHandle.set_tau``; with a baseline ``ChunkHandle.lnlike_marg_tv``),
        ``lnprob_grad*`` return the ``tau`` entries in vector order, ``fisher*`` / ``loo*`` dispatch to ``fisher_tv`` /
        ``loo_tv`` (``fisher_marg_tv`` under a baseline; ``loo`` under a baseline is refused: not built).  The streamed
        entries and ``PSOAP_GPU_SERVER`` are refused.  ``None``: every path as it was."""
        self.model = model
        self.fix_params = list(fix_params)
        self.defaults = dict(defaults or {})
        self.handle = ChunkHandle(fl, as_f64(sigma) * soften, max_batch=max_batch, device=device)
        dates = as_f64(dates)
        self.handle.set_grid(lwl, epoch_index, dates.shape[0])
        # the observed-frame grid, the epoch of every pixel and the dates, for the grid tangents of ``fisher``
        self.lwl, self.epoch_index, self.dates = as_f64(lwl), np.asarray(epoch_index, dtype=np.int64), dates
        check(self.handle._L.psoap_chunk_set_dates(self.handle._h, dptr(dates), dates.shape[0]), "psoap_chunk_set_dates")
        self.baseline = None
        if baseline is not None:
            unknown = set(baseline) - {"order", "sd", "weight"}
            if unknown or "order" not in baseline or "sd" not in baseline:
                raise ValueError(f"baseline needs 'order' and 'sd' (and optionally 'weight'); got {sorted(baseline)}")
            kind = baseline.get("weight", "one")
            if kind not in ("one", "flux"):
                raise ValueError("baseline['weight'] must be 'one' or 'flux'")
            self.baseline = {"order": int(baseline["order"]), "sd": [float(v) for v in baseline["sd"]], "weight": kind}
            self.handle.set_baseline(self.baseline["order"], self.lwl, self.epoch_index, dates.shape[0], self.baseline["sd"],
                                     self.handle.fl if kind == "flux" else None)
        self.timevar = None
        if timevar is not None:
            if os.environ.get("PSOAP_GPU_SERVER", "").strip().lower() not in ("", "0"):
                raise _lib.PsoapError("a timevar worker needs the device in this process (PSOAP_GPU_SERVER serves the static "
                                      "likelihood only)")
            fit, tau, times = timevar_spec(model, timevar)
            if times is None:
                times = dates[self.epoch_index]
                times = times - times.min()
            self.times = as_f64(times, (self.handle.N,))
            self.timevar = {"fit": fit, "tau": tau}
            self.handle.set_times(self.times)
            # an upload that will carry time scales is evaluated on the staged path whatever the mode: in staged mode the
            # upload does not queue the skyline's sort and envelope kernels, whose results only the persistent kernel reads
            self.handle.set_mode("staged")

    # -- time scales in the fitted vector (utils.convert_vectors_timevar) ------------------------------------------------
    def split_vectors(self, ps):
        """fitted vectors (B, n_fit) -> ``(p_orb, p_gp, taus)``; ``taus`` (B, c) on a ``timevar`` worker, else ``None``"""
        if self.timevar is None:
            return (*convert_vectors(np.atleast_2d(ps), self.model, self.fix_params, **self.defaults), None)
        return convert_vectors_timevar(np.atleast_2d(ps), self.model, self.fix_params, self.timevar["fit"], self.timevar["tau"],
                                       **self.defaults)

    def _taus(self, tau, B):
        """``tau`` (c,) or (B, c), ``None``: the defaults -> (B, c); ``None`` on a worker without ``timevar``"""
        if self.timevar is None:
            if tau is not None:
                raise _lib.PsoapError("this worker has no time scales (ChunkWorker(..., timevar=...))")
            return None
        c = N_COMPONENTS[self.model]
        tau = self.timevar["tau"] if tau is None else as_f64(tau)
        return as_f64(np.broadcast_to(np.atleast_2d(tau), (B, c)))

    def _no_timevar(self, what):
        if self.timevar is not None:
            raise _lib.PsoapError(f"{what} has no temporal factor; this worker has time scales (use lnprob / lnprob_batch or "
                                  "the upload_* entries)")

    def _fit_index(self):
        """columns of a full ``[orbit, GP, tau]`` array that a fitted vector holds, in vector order"""
        reg = registered_params[self.model]
        ind = [i for i, name in enumerate(reg) if name not in self.fix_params]
        if self.timevar is not None:
            first = n_params_orb[self.model] + 2 * N_COMPONENTS[self.model]
            ind += [first + int(k) for k in np.flatnonzero(self.timevar["fit"])]
        return ind

    def close(self):
        self.handle.close()

    def _no_baseline(self, what):
        if self.baseline is not None:
            raise _lib.PsoapError(f"{what} evaluates the plain likelihood; this worker has a baseline (use lnprob / lnprob_batch)")

    # -- likelihood with the per-epoch continuum integrated out (include/psoap_gp.h: psoap_chunk_lnlike_marg) ---------
    def shifted_grids(self, p_orb):
        """(B, n_orb) -> ``(lwls (B, c, N), too_fast (B,))``: the velocities from the device (``orbit.velocities``), the
        grids shifted on the host exactly as ``fisher_orbits`` and ``loo_orbits`` shift them"""
        from .data import c_kms
        from .orbit import velocities
        p_orb = as_f64(np.atleast_2d(p_orb))
        p_orb = as_f64(p_orb, (p_orb.shape[0], n_params_orb[self.model]))
        vel = velocities(self.model, p_orb, self.dates, device=self.handle.device)
        fast = np.any(np.abs(vel) >= c_kms, axis=(1, 2))
        return self.lwl[None, None, :] + (-vel[:, :, self.epoch_index]) / c_kms, fast

    def marg_orbits(self, p_orb, p_gp, mu_GP: float = 1.0, tau=None, **want):
        """The marginal likelihood with the vectors already split: (B, n_orb) and (B, 2c) -> (B,), or a ``chunk.MargResult``
        with ``want_beta`` / ``want_cov`` / ``want_flux``; walked in pieces of ``max_batch``.  A faster-than-light orbit gives
        ``-inf`` (and NaN), as a negative hyper-parameter or a matrix that is not positive definite does.  On a ``timevar``
        worker the kernel is the time-variable one (``ChunkHandle.lnlike_marg_tv``) at ``tau`` (B, c) or (c,) (``None``: the
        defaults)."""
        if self.baseline is None:
            raise _lib.PsoapError("this worker has no baseline (ChunkWorker(..., baseline=...))")
        if os.environ.get("PSOAP_GPU_SERVER", "").strip().lower() not in ("", "0"):
            raise _lib.PsoapError("the marginal likelihood needs the device in this process (PSOAP_GPU_SERVER serves values only)")
        from .chunk import MargResult
        lwls, fast = self.shifted_grids(p_orb)
        B, c = lwls.shape[0], N_COMPONENTS[self.model]
        p_gp = as_f64(np.atleast_2d(p_gp), (B, 2 * c))
        lwls[fast] = lwls[~fast][0] if np.any(~fast) else self.lwl          # (a stand-in: overwritten below)
        taus, mb = self._taus(tau, B), self.handle.max_batch
        if taus is None:
            pieces = [self.handle.lnlike_marg(lwls[s:s + mb], p_gp[s:s + mb], mu_GP, **want) for s in range(0, B, mb)]
        else:
            pieces = [self.handle.lnlike_marg_tv(lwls[s:s + mb], p_gp[s:s + mb], taus[s:s + mb], mu_GP, **want)
                      for s in range(0, B, mb)]
        if not isinstance(pieces[0], MargResult):
            out = np.concatenate(pieces)
            out[fast] = -np.inf
            return out
        cat = lambda k: None if getattr(pieces[0], k) is None else np.concatenate([getattr(r, k) for r in pieces])  # noqa: E731
        res = MargResult(cat("lnp"), cat("parts"), cat("beta"), cat("beta_cov"), cat("fl_cor"))
        res.lnp[fast] = -np.inf
        for k in ("parts", "beta", "beta_cov", "fl_cor"):
            if getattr(res, k) is not None:
                getattr(res, k)[fast] = np.nan
        return res

    def upload_proposals(self, ps, mu_GP: float = 1.0) -> None:
        """Ship fitted parameter vectors (B, n_fit); the orbit solve and the Doppler shift are queued on the
        chunk's stream.  Follow with ``handle.eval()`` (or a ``ChunkGroup.eval()``) and ``handle.fetch()``."""
        self._no_baseline("upload_proposals")
        p_orb, p_gp, taus = self.split_vectors(ps)
        self.upload_orbits(p_orb, p_gp, mu_GP, taus)

    def upload_orbits(self, p_orb, p_gp, mu_GP: float = 1.0, tau=None) -> None:
        """The same with the vectors already split: orbital parameters (B, n_orb) and GP parameters (B, 2c).  The library
        reads exactly 2c GP parameters per proposal, so a narrower array is refused here.  (ST2 registers two GP
        parameters, utils.py:7, for a likelihood of two components, covariance.py:379: its fitted vectors stop at
        ``upload_proposals`` as they stop with a TypeError in ``Worker.lnprob``; this entry takes all four.)  On a ``timevar``
        worker the upload carries ``tau`` (B, c) or (c,) (``None``: the defaults) and ``handle.eval()`` takes the staged path
        with the time-variable fill (``ChunkHandle.set_tau``); such a handle cannot join a ``ChunkGroup.eval()``."""
        self._no_baseline("upload_orbits")
        p_orb = as_f64(np.atleast_2d(p_orb))
        B = p_orb.shape[0]
        p_orb = as_f64(p_orb, (B, n_params_orb[self.model]))
        p_gp = as_f64(np.atleast_2d(p_gp), (B, 2 * N_COMPONENTS[self.model]))
        taus = self._taus(tau, B)          # (before anything is queued: a refusal leaves no upload pending)
        h = self.handle
        check(h._L.psoap_batch_upload_orbits(h._h, B, MODEL_ID[self.model], dptr(p_orb), dptr(p_gp), float(mu_GP)),
              "psoap_batch_upload_orbits")
        h._B = B
        if taus is not None:
            h.set_tau(taus)

    # -- streamed form: ONE resident launch across sampler iterations (include/psoap_gp.h: psoap_stream_*) ----------
    def stream_open(self, lanes: int | None = None, scheme: int = -1):
        self._no_baseline("the streamed path")
        self._no_timevar("the streamed path")
        self.handle.stream_open(N_COMPONENTS[self.model], lanes, scheme)

    def stream_submit(self, ps, mu_GP: float = 1.0) -> np.ndarray:
        """fitted parameter vectors (n, n_fit) -> tickets; Kepler solve, |v| >= c rule, Doppler shift and likelihood all
        inside the resident launch (``Worker.lnprob`` for n proposals, sample_parallel.py:168-198)"""
        self._no_baseline("the streamed path")
        self._no_timevar("the streamed path")
        p_orb, p_gp = convert_vectors(np.atleast_2d(ps), self.model, self.fix_params, **self.defaults)
        return self.handle.stream_submit_orbits(MODEL_ID[self.model], p_orb, p_gp, mu_GP)

    def stream_fetch(self, tickets) -> np.ndarray:
        return self.handle.stream_fetch(tickets)

    def stream_close(self):
        self.handle.stream_close()

    def lnprob_batch(self, ps, mu_GP: float = 1.0) -> np.ndarray:
        if self.baseline is not None:
            p_orb, p_gp, taus = self.split_vectors(ps)
            return self.marg_orbits(p_orb, p_gp, mu_GP, taus)
        self.upload_proposals(ps, mu_GP)
        self.handle.eval()
        return self.handle.fetch()

    def lnprob(self, p, mu_GP: float = 1.0) -> float:
        return float(self.lnprob_batch(np.atleast_2d(p), mu_GP)[0])

    # -- gradient of lnprob(p) (include/psoap_gp.h: psoap_chunk_lnprob_grad) ----------------------------------------
    def lnprob_grad_orbits(self, p_orb, p_gp, mu_GP: float = 1.0, want_vel: bool = False, tau=None):
        """The gradient with the vectors already split, as ``upload_orbits`` takes them: orbital parameters (B, n_orb) and
        GP parameters (B, 2c) -> ``(lnp (B,), grad_orb (B, n_orb), grad_gp (B, 2c), grad_mu (B,))`` (and ``grad_vel
        (B, c, n_epochs)`` with ``want_vel``).  Kepler solve, orbit Jacobian, Doppler shift, likelihood gradient and the
        chain rule run on the device.  The only way in for ST2, for the reason ``upload_orbits`` documents.  On a worker
        with a baseline the likelihood in the middle is the marginal one (``ChunkHandle.lnprob_marg_grad``).  On a ``timevar``
        worker the kernel is the time-variable one at ``tau`` (B, c) or (c,) (``None``: the defaults) and ``grad_tau (B, c)``
        follows ``grad_gp`` in the tuple (``ChunkHandle.lnprob_tv_grad`` / ``lnprob_marg_tv_grad``)."""
        if os.environ.get("PSOAP_GPU_SERVER", "").strip().lower() not in ("", "0"):
            raise _lib.PsoapError("lnprob_grad needs the device in this process (PSOAP_GPU_SERVER serves values only)")
        p_orb = as_f64(np.atleast_2d(p_orb))
        B = p_orb.shape[0]
        p_orb = as_f64(p_orb, (B, n_params_orb[self.model]))
        p_gp = as_f64(np.atleast_2d(p_gp), (B, 2 * N_COMPONENTS[self.model]))
        taus = self._taus(tau, B)
        if taus is not None:
            entry = self.handle.lnprob_marg_tv_grad if self.baseline is not None else self.handle.lnprob_tv_grad
            return entry(MODEL_ID[self.model], p_orb, p_gp, taus, mu_GP, want_vel=want_vel)
        if getattr(self, "baseline", None) is not None:      # (the gradient of what ``lnprob`` returns on this worker)
            return self.handle.lnprob_marg_grad(MODEL_ID[self.model], p_orb, p_gp, mu_GP, want_vel=want_vel)
        return self.handle.lnprob_grad(MODEL_ID[self.model], p_orb, p_gp, mu_GP, want_vel=want_vel)

    def lnprob_grad_batch(self, ps, mu_GP: float = 1.0):
        """Fitted parameter vectors (B, n_fit) -> ``(lnp (B,), grad (B, n_fit))``: the derivative with respect to every
        non-fixed parameter, in registered order; fixed parameters drop out.  A proposal whose ``lnp`` is ``-inf`` has a
        NaN gradient.  On a ``timevar`` worker the fitted time scales' derivatives follow, in vector order."""
        p_orb, p_gp, taus = self.split_vectors(ps)
        if taus is None:
            lnp, g_orb, g_gp, _g_mu = self.lnprob_grad_orbits(p_orb, p_gp, mu_GP)
            full = np.concatenate([g_orb, g_gp], axis=1)
        else:
            lnp, g_orb, g_gp, g_tau, _g_mu = self.lnprob_grad_orbits(p_orb, p_gp, mu_GP, tau=taus)
            full = np.concatenate([g_orb, g_gp, g_tau], axis=1)
        return lnp, np.ascontiguousarray(full[:, self._fit_index()])

    def lnprob_grad(self, p, mu_GP: float = 1.0):
        lnp, grad = self.lnprob_grad_batch(np.atleast_2d(p), mu_GP)
        return float(lnp[0]), grad[0]

    # -- Fisher information of lnprob(p) (include/psoap_gp.h: psoap_chunk_fisher) ------------------------------------
    def fisher_orbits(self, p_orb, p_gp, tau=None):
        """The Fisher information of this chunk with the vectors already split: orbital parameters (n_orb,) and GP
        parameters (2c,) -> ``(n_orb + 2c, n_orb + 2c)`` in registered order.  The tangent of orbital parameter i moves
        the grid of component c by ``dx[n] = -J[c, epoch(n), i] / c_kms`` with ``J`` the device's velocity Jacobian
        (``orbit.velocity_jacobian``, which also gives the velocities the grids are shifted by, as ``lnprob`` shifts
        them); the tangents of the GP parameters are unit vectors.  The (T, c, N) tangents are assembled on the host,
        everything of order N^3 runs on the device.  A faster-than-light orbit, a negative hyper-parameter or a matrix
        that is not positive definite gives NaN in every entry.  On a worker with a baseline the information is that of the
        marginal likelihood (``ChunkHandle.fisher_marg``): of what ``lnprob`` returns on this worker.  On a ``timevar`` worker
        the kernel is the time-variable one at ``tau`` (c,) (``None``: the defaults) and the matrix has one more row and
        column per component, the unit ``dtau`` tangents, after the GP parameters: ``(n_orb + 3c, n_orb + 3c)``
        (``ChunkHandle.fisher_tv``, under a baseline ``fisher_marg_tv``)."""
        if os.environ.get("PSOAP_GPU_SERVER", "").strip().lower() not in ("", "0"):
            raise _lib.PsoapError("fisher needs the device in this process (PSOAP_GPU_SERVER serves values only)")
        from .data import c_kms
        from .orbit import velocity_jacobian
        c, n_orb = N_COMPONENTS[self.model], n_params_orb[self.model]
        p_orb = as_f64(np.ravel(p_orb), (n_orb,))
        p_gp = as_f64(np.ravel(p_gp), (2 * c,))
        vel, jac = velocity_jacobian(self.model, p_orb[None], self.dates, device=self.handle.device)
        taus = self._taus(tau, 1)
        T = n_orb + 2 * c + (0 if taus is None else c)
        if np.any(np.abs(vel[0]) >= c_kms):
            return np.full((T, T), np.nan)
        ep = self.epoch_index
        lwls = self.lwl[None, :] + (-vel[0][:, ep]) / c_kms          # (as the device shifts: fill_kernels.hpp)
        tan_lwl = np.zeros((T, c, self.handle.N))
        tan_lwl[:n_orb] = -np.moveaxis(jac[0], 2, 0)[:, :, ep] / c_kms
        tan_gp = np.zeros((T, 2 * c))
        tan_gp[n_orb:n_orb + 2 * c] = np.eye(2 * c)
        if taus is not None:
            tan_tau = np.zeros((T, c))
            tan_tau[n_orb + 2 * c:] = np.eye(c)
            entry = self.handle.fisher_marg_tv if self.baseline is not None else self.handle.fisher_tv
            return entry(lwls, p_gp, taus[0], tan_gp, tan_tau, tan_lwl)
        if getattr(self, "baseline", None) is not None:      # (the information of what ``lnprob`` returns on this worker)
            return self.handle.fisher_marg(lwls, p_gp, tan_gp, tan_lwl)
        return self.handle.fisher(lwls, p_gp, tan_gp, tan_lwl)

    def fisher(self, p):
        """One fitted parameter vector (n_fit,) -> ``(n_fit, n_fit)`` over the non-fixed parameters in registered order,
        the ordering of ``lnprob_grad``; fixed parameters drop out."""
        p_orb, p_gp, taus = self.split_vectors(p)
        full = self.fisher_orbits(p_orb[0], p_gp[0], None if taus is None else taus[0])
        fit_ind = self._fit_index()
        return np.ascontiguousarray(full[np.ix_(fit_ind, fit_ind)])

    # -- leave-one-out cross-validation at lnprob(p) (include/psoap_gp.h: psoap_chunk_loo) ----------------------------
    def loo_orbits(self, p_orb, p_gp, mu_GP: float = 1.0, tau=None):
        """Leave-one-out cross-validation of this chunk with the vectors already split: orbital parameters (n_orb,) and GP
        parameters (2c,) -> a ``chunk.LooResult`` with the epoch fields over the worker's own ``epoch_index``.  The
        velocities come from the device (``orbit.velocities``) and the grids are shifted on the host exactly as
        ``fisher_orbits`` shifts them.  A faster-than-light orbit gives ``lnp = -inf`` and NaN, as a negative
        hyper-parameter or a matrix that is not positive definite does.  On a worker with a baseline every prediction is made
        under the marginal likelihood (``ChunkHandle.loo_marg``): an epoch whose only fault is a continuum offset within the
        prior is not an outlier, and ``lnp`` is what ``lnprob`` returns on this worker.  On a ``timevar`` worker every
        prediction is made under the time-variable kernel at ``tau`` (c,) (``None``: the defaults; ``ChunkHandle.loo_tv``);
        with a baseline as well it is refused: that combination is not built."""
        if self.timevar is not None and self.baseline is not None:
            raise _lib.PsoapError("loo: leave-one-out under a baseline and time scales together is not built")
        if os.environ.get("PSOAP_GPU_SERVER", "").strip().lower() not in ("", "0"):
            raise _lib.PsoapError("loo needs the device in this process (PSOAP_GPU_SERVER serves values only)")
        from .chunk import LooResult
        from .data import c_kms
        from .orbit import velocities
        c, n_orb = N_COMPONENTS[self.model], n_params_orb[self.model]
        p_orb = as_f64(np.ravel(p_orb), (n_orb,))
        p_gp = as_f64(np.ravel(p_gp), (2 * c,))
        ep, ne = self.epoch_index, self.dates.shape[0]
        vel = velocities(self.model, p_orb[None], self.dates, device=self.handle.device)[0]
        if np.any(np.abs(vel) >= c_kms):
            return LooResult.degenerate(self.handle.N, np.bincount(ep, minlength=ne))
        lwls = self.lwl[None, :] + (-vel[:, ep]) / c_kms          # (as the device shifts: fill_kernels.hpp)
        taus = self._taus(tau, 1)
        if taus is not None:
            return self.handle.loo_tv(lwls, p_gp, taus[0], mu_GP, ep, ne)
        if getattr(self, "baseline", None) is not None:
            return self.handle.loo_marg(lwls, p_gp, mu_GP, ep, ne)
        return self.handle.loo(lwls, p_gp, mu_GP, ep, ne)

    def loo(self, p, mu_GP: float = 1.0):
        """One fitted parameter vector (n_fit,) -> the ``chunk.LooResult`` of this chunk there"""
        p_orb, p_gp, taus = self.split_vectors(p)
        return self.loo_orbits(p_orb[0], p_gp[0], mu_GP, None if taus is None else taus[0])

    # -- per-epoch velocities free of any orbit (include/psoap_gp.h: psoap_chunk_fisher_vel) ---------------------------
    def _grids_at(self, vel, what, baseline_ok=False):
        """a free velocity table (c, E) -> ``(lwls (c, N), too_fast)``, the grids shifted as ``shifted_grids`` shifts them"""
        if not baseline_ok:
            self._no_baseline(what)
        self._no_timevar(what)
        if os.environ.get("PSOAP_GPU_SERVER", "").strip().lower() not in ("", "0"):
            raise _lib.PsoapError(f"{what} needs the device in this process (PSOAP_GPU_SERVER serves values only)")
        from .data import c_kms
        vel = as_f64(vel, (N_COMPONENTS[self.model], self.dates.shape[0]))
        fast = bool(np.any(np.abs(vel) >= c_kms))
        return self.lwl[None, :] + (-vel[:, self.epoch_index]) / c_kms, fast

    def fisher_vel_at(self, vel, p_gp):
        """The ``(c E, c E)`` information of the per-epoch velocities of this chunk at the free velocity table ``vel``
        (c, E) and GP parameters ``p_gp`` (2c,), row ``c * E + e`` (``ChunkHandle.fisher_vel``): AT FIXED hyper-parameters,
        with one null direction per component.  Any ``|v| >= c_kms``, a negative hyper-parameter or a matrix that is not
        positive definite gives NaN in every entry.  A worker with a baseline is refused here: ``info_vel_at`` is the path
        that accepts one, with ``(K + H Lambda H^T)^-1`` in place of ``K^-1``."""
        lwls, fast = self._grids_at(vel, "fisher_vel_at")
        c, E = N_COMPONENTS[self.model], self.dates.shape[0]
        if fast:
            return np.full((c * E, c * E), np.nan)
        return self.handle.fisher_vel(lwls, as_f64(np.ravel(p_gp), (2 * c,)), self.epoch_index, E)

    def lnlike_grad_vel(self, vel, p_gp, mu_GP: float = 1.0):
        """``(lnp, grad_vel (c, E))`` of this chunk at the free velocity table ``vel`` (c, E): ``ChunkHandle.lnlike_grad``
        folded by ``covariance.velocity_gradient``.  Any ``|v| >= c_kms``, a negative hyper-parameter or a matrix that is
        not positive definite gives ``-inf`` and NaN.  A worker with a baseline is refused, as for ``fisher_vel_at``;
        ``info_vel_at`` accepts one."""
        from .covariance import velocity_gradient
        lwls, fast = self._grids_at(vel, "lnlike_grad_vel")
        c, E = N_COMPONENTS[self.model], self.dates.shape[0]
        if fast:
            return -np.inf, np.full((c, E), np.nan)
        lnp, _g_gp, g_lwl, _g_mu = self.handle.lnlike_grad(lwls, as_f64(np.ravel(p_gp), (2 * c,)), mu_GP)
        return float(lnp), velocity_gradient(g_lwl, self.epoch_index, E)

    def info_vel_at(self, vel, p_gp, mu_GP: float = 1.0):
        """``(lnp, grad_vel (c, E), F (c E, c E), J (c E, c E))`` of this chunk at the free velocity table ``vel`` (c, E) from
        one factorisation (``ChunkHandle.info_vel``): value, gradient, expected and observed information, ``E[J] = F``.  On
        a worker with a baseline everything is taken under the marginal likelihood, the one ``lnprob`` returns on this
        worker -- this is the path that accepts a baseline.  Any ``|v| >= c_kms``, a negative hyper-parameter or a matrix
        that is not positive definite gives ``-inf`` and NaN."""
        lwls, fast = self._grids_at(vel, "info_vel_at", baseline_ok=True)
        c, E = N_COMPONENTS[self.model], self.dates.shape[0]
        if fast:
            return -np.inf, np.full((c, E), np.nan), np.full((c * E, c * E), np.nan), np.full((c * E, c * E), np.nan)
        return self.handle.info_vel(lwls, as_f64(np.ravel(p_gp), (2 * c,)), self.epoch_index, E, mu_GP,
                                    marg=self.baseline is not None)


def baseline_fit(workers, p, mu_GP=1.0):
    """The continuum of every epoch at the fitted vector ``p``, per chunk: a list, in the order of ``workers`` (each made
    with ``baseline=...``), of dicts with ``beta`` (n_epochs, order + 1), ``beta_cov`` (q, q), ``beta_sd`` (as ``beta``),
    ``fl_cor`` (N,) and ``lnp`` -- all epochs of a chunk jointly, in one evaluation, with error bars: the counterpart of the
    iterated, frozen ``cycle_calibration``."""
    workers = list(workers) if isinstance(workers, (list, tuple)) else [workers]
    out = []
    for w in workers:
        p_orb, p_gp = convert_vectors(np.atleast_2d(p), w.model, w.fix_params, **w.defaults)
        r = w.marg_orbits(p_orb[:1], p_gp[:1], mu_GP, want_beta=True, want_cov=True, want_flux=True)
        out.append({"beta": r.beta[0], "beta_cov": r.beta_cov[0], "beta_sd": r.beta_sd[0], "fl_cor": r.fl_cor[0],
                    "lnp": float(r.lnp[0])})
    return out


def write_corrected_chunks(chunk_rows, chunks, fits, prefix="", fmt="npz"):
    """Write the corrected fluxes of ``baseline_fit`` back into chunk files through ``data.Chunk.save`` (what
    scripts/psoap_apply_calibration.py does with the frozen polynomials): ``chunk_rows`` holds ``(order, wl0, wl1)`` per chunk
    as in ``chunks.dat``, ``chunks`` the UNMASKED 2-D ``data.Chunk`` objects in the same order (``Chunk.open``), ``fits`` the
    list ``baseline_fit`` returned for workers built from their masked copies.  Masked pixels keep their flux.  -> the file
    names."""
    from .data import Chunk
    names = []
    for (order, wl0, wl1), ch, fit in zip(chunk_rows, chunks, fits):
        if np.ndim(ch.wl) != 2:
            raise ValueError("write_corrected_chunks needs the 2-D chunks (before apply_mask)")
        if int(np.count_nonzero(ch.mask)) != np.shape(fit["fl_cor"])[0]:
            raise ValueError("a fit does not have one corrected flux per unmasked pixel of its chunk")
        fl = np.array(ch.fl, dtype=np.float64)
        fl[ch.mask] = fit["fl_cor"]
        names.append(Chunk(ch.wl, fl, ch.sigma, ch.date, ch.mask).save(order, wl0, wl1, prefix=prefix, fmt=fmt))
    return names


def loo_outliers(workers, p, pix_sigma=5.0, epoch_p=1e-4, mu_GP=1.0):
    """What disagrees with the fitted model at ``p``, per chunk: a list, in the order of ``workers``, of dicts with
    ``pixels`` (indices with ``|pix_z| > pix_sigma``), ``epochs`` (ids whose ``ep_chi2`` has an upper-tail chi-squared
    probability below ``epoch_p`` at ``ep_npix`` degrees of freedom, ``scipy.stats.chi2.sf``), the probabilities ``epoch_sf``
    of every epoch and the ``LooResult`` itself (``loo``).  Workers built with ``baseline=...`` predict under their marginal
    likelihood: a continuum offset the baseline absorbs flags nothing.  The two defaults are conventions, not measurements: 5 sigma per
    pixel (one in 1.7 million under the model), and one in 10,000 per epoch (a hundred epochs of ten chunks then flag one
    good epoch in ten runs)."""
    from scipy.stats import chi2
    workers = list(workers) if isinstance(workers, (list, tuple)) else [workers]
    out = []
    for w in workers:
        r = w.loo(p, mu_GP)
        with np.errstate(invalid="ignore"):
            pixels = np.flatnonzero(np.abs(r.pix_z) > pix_sigma)
            sf = np.where(r.ep_npix > 0, chi2.sf(r.ep_chi2, np.maximum(r.ep_npix, 1)), 1.0)
            epochs = np.flatnonzero(sf < epoch_p)
        out.append({"pixels": pixels, "epochs": epochs, "epoch_sf": sf, "loo": r})
    return out


def loo_mask_rows(chunks_meta, outliers, pad_days=0.1):
    """``masks.dat`` rows ``(wl0, wl1, t0, t1)`` for the epochs ``loo_outliers`` flagged: ``chunks_meta`` holds, per chunk
    and in the same order, ``(wl0, wl1, dates)`` -- the chunk's wavelength range as in ``chunks.dat`` and the date of every
    epoch.  A flagged epoch becomes the chunk's whole range over ``date -+ pad_days``, the tenth of a day of
    the reference's scripts/psoap_generate_masks.py:95-98 by default.  Flagged pixels make no row: a row removes a
    whole epoch of a chunk.  Write them with ``data.write_mask_table``."""
    rows = []
    for (wl0, wl1, dates), found in zip(chunks_meta, outliers):
        dates = np.asarray(dates, dtype=np.float64)
        for e in found["epochs"]:
            rows.append((float(wl0), float(wl1), float(dates[e] - pad_days), float(dates[e] + pad_days)))
    return rows


def fisher_information(workers, p):
    """The Fisher information of the SUM of the workers' ``lnprob`` at the fitted vector ``p``: the sum of
    ``ChunkWorker.fisher`` over the chunks, ``(n_fit, n_fit)``.  Workers built with ``baseline=...`` contribute the
    information of their marginal likelihood, so ``laplace_covariance`` and ``fisher_jumps`` carry the uncertainty of the
    continuum."""
    workers = list(workers) if isinstance(workers, (list, tuple)) else [workers]
    total = None
    for w in workers:
        F = w.fisher(p)
        total = F if total is None else total + F
    return total


def laplace_covariance(workers, p, prior_precision=None):
    """The Laplace covariance at ``p``: the inverse, by Cholesky, of the summed Fisher information plus
    ``prior_precision`` (``(n_fit, n_fit)``, or ``(n_fit,)`` for a diagonal one).  Raises ``np.linalg.LinAlgError`` when
    that sum is not positive definite -- a direction the data do not constrain needs a prior."""
    from scipy.linalg import cho_factor, cho_solve
    F = fisher_information(workers, p)
    if prior_precision is not None:
        pp = as_f64(prior_precision)
        F = F + (np.diag(pp) if pp.ndim == 1 else pp)
    if not np.all(np.isfinite(F)):
        raise np.linalg.LinAlgError("the Fisher information is not finite")
    try:
        factor = cho_factor(F, lower=True)
    except np.linalg.LinAlgError:
        raise np.linalg.LinAlgError("the summed Fisher information is not positive definite") from None
    C = cho_solve(factor, np.eye(F.shape[0]))
    return 0.5 * (C + C.T)


def fisher_jumps(workers, p, fname=None, prior_precision=None):
    """A proposal covariance before any chain exists: ``2.38**2 / d`` times the Laplace covariance at ``p`` (the scaling
    of ``utils.estimate_covariance``).  With ``fname`` the matrix is also saved with ``np.save``: what the ``opt_jump``
    key of config.yaml names (``sample_parallel.proposal_covariance``)."""
    C = laplace_covariance(workers, p, prior_precision)
    cov = 2.38 ** 2 / C.shape[0] * C
    if fname is not None:
        np.save(fname, cov)
    return cov


def optimize_orbit(workers, p0, bounds=None, mu_GP=1.0, ftol=1e-10, full_output=False):
    """L-BFGS-B fit of one fitted parameter vector to several chunks from ``p0``, with the analytic gradient
    (``ChunkWorker.lnprob_grad``, ``jac=True``): the objective is minus the SUM of the workers' ``lnprob``, the sum
    ``sample_parallel`` takes over its chunks.  No priors: the caller passes ``bounds`` (SciPy's form, one pair per fitted
    parameter).  Returns the fitted vector, or SciPy's whole result with ``full_output`` (``-result.fun`` is the summed
    ``lnprob`` reached, ``result.jac`` the gradient of minus that sum there).  Modelled on ``covariance.optimize_GP``.
    Workers built with ``baseline=...`` are fitted under their marginal likelihood: ``baseline_fit`` at the result then gives
    the continuum that belongs to the fit."""
    from scipy.optimize import minimize
    workers = list(workers) if isinstance(workers, (list, tuple)) else [workers]
    x0 = as_f64(np.atleast_1d(p0))

    def func(x):
        total, grad = 0.0, np.zeros_like(x)
        for w in workers:
            lnp, g = w.lnprob_grad(x, mu_GP)
            if not np.isfinite(lnp):
                return np.inf, np.zeros_like(x)
            total += lnp
            grad += g
        return -total, -grad

    res = minimize(func, x0, jac=True, method="L-BFGS-B", bounds=bounds, options={"ftol": ftol})
    return res if full_output else res["x"]


# ---- per-epoch radial velocities with error bars, free of any orbit model --------------------------------------------------
def _velocity_contrasts(c, n_epochs, idx):
    """``Q^T`` (c (len(idx) - 1), c E) of ``velocity_pinv``: per component the Helmert contrasts of the seen epochs ``idx``"""
    n = c * n_epochs
    rows = []
    for k in range(c):
        for j in range(1, idx.size):
            v = np.zeros(n)
            v[k * n_epochs + idx[:j]] = 1.0
            v[k * n_epochs + idx[j]] = -float(j)
            rows.append(v / np.sqrt(j * (j + 1.0)))
    return np.array(rows)


def velocity_pinv(F, c, n_epochs, seen):
    """``F^+`` on the complement of the ``c`` per-component constant vectors and of the epochs nobody sees (``seen`` (E,)
    bool): with ``Q`` an orthonormal basis of that complement (per component the Helmert contrasts of the seen epochs),
    ``Q (Q^T F Q)^-1 Q^T``.  Rows and columns of unseen epochs are zero."""
    n = c * n_epochs
    idx = np.flatnonzero(np.asarray(seen, dtype=bool))
    if idx.size < 2:
        return np.zeros((n, n))
    Q = _velocity_contrasts(c, n_epochs, idx).T
    M = Q.T @ as_f64(F) @ Q
    return Q @ np.linalg.solve(0.5 * (M + M.T), Q.T)


def velocity_scoring(value, grad_info, vel0, seen, max_iter=20, tol=1e-10):
    """Fisher scoring on a velocity table from ``vel0`` (c, E): ``value(vel) -> lnp`` and ``grad_info(vel) -> (g (c, E),
    F (c E, c E))`` are the summed likelihood, its gradient and its information.  Per iteration ``delta = F^+ g``
    (``velocity_pinv``), the step halved until the value does not decrease; stops when the Newton decrement
    ``g^T F^+ g <= tol``.  -> dict with ``vel``, ``cov`` (F^+ at ``vel``), ``n_iter``, ``decrement``, ``lnp_start``, ``lnp``,
    ``converged``.  The loop of ``epoch_velocities``; the tests run it on a float64 CPU twin as well."""
    vel = as_f64(vel0).copy()
    c, E = vel.shape
    lnp = lnp0 = float(value(vel))
    it = 0
    while True:
        g, F = grad_info(vel)
        if not (np.isfinite(lnp) and np.all(np.isfinite(g)) and np.all(np.isfinite(F))):
            raise np.linalg.LinAlgError("the likelihood, its gradient or its information is not finite at the velocity table")
        cov = velocity_pinv(F, c, E, seen)
        gv = as_f64(g).reshape(-1)
        delta = cov @ gv
        dec = float(gv @ delta)
        if dec <= tol or it >= max_iter:
            return {"vel": vel, "cov": cov, "n_iter": it, "decrement": dec, "lnp_start": lnp0, "lnp": lnp, "converged": dec <= tol}
        step, moved = 1.0, False
        for _ in range(60):
            trial = vel + step * delta.reshape(c, E)
            v = float(value(trial))
            if v >= lnp:
                vel, lnp, moved = trial, v, True
                break
            step *= 0.5
        it += 1
        if not moved:
            return {"vel": vel, "cov": cov, "n_iter": it, "decrement": dec, "lnp_start": lnp0, "lnp": lnp, "converged": False}


def velocity_newton(value, info, vel0, seen, max_iter=20, tol=1e-10):
    """Newton's method on a velocity table from ``vel0`` (c, E): ``info(vel) -> (lnp, g (c, E), F, J)`` is one call for the
    summed likelihood, its gradient, its expected and its observed information; ``value(vel) -> lnp`` serves the line
    search.  Per iteration the step is ``J^+ g`` when ``Q^T J Q`` (the ``Q`` of ``velocity_pinv``) has a Cholesky factor --
    the data's own curvature: quadratic convergence near the optimum -- and ``F^+ g`` otherwise (``n_fallback`` counts
    those); the step is halved until ``value`` does not decrease (one more ``value`` call at the start gives the line search
    its first level), so ``lnp`` is never lowered.  Stops when the decrement
    ``g^T cov g <= tol``.  -> the dict of ``velocity_scoring`` plus ``cov_kind`` (``"observed"``: ``cov = J^+`` at ``vel``,
    or ``"expected"``) and ``n_fallback``."""
    vel = as_f64(vel0).copy()
    c, E = vel.shape
    idx = np.flatnonzero(np.asarray(seen, dtype=bool))
    it, n_fallback, lnp0 = 0, 0, None
    ref = float(value(vel))      # the line search compares values of ONE evaluation path: info's lnp may differ from it by rounding
    while True:
        lnp, g, F, J = info(vel)
        lnp = float(lnp)
        if lnp0 is None:
            lnp0 = lnp
        if not (np.isfinite(lnp) and np.all(np.isfinite(g)) and np.all(np.isfinite(F)) and np.all(np.isfinite(J))):
            raise np.linalg.LinAlgError("the likelihood, its gradient or its information is not finite at the velocity table")
        kind = "observed"
        if idx.size >= 2:
            Qt = _velocity_contrasts(c, E, idx)
            M = Qt @ as_f64(J) @ Qt.T
            try:
                np.linalg.cholesky(0.5 * (M + M.T))
            except np.linalg.LinAlgError:
                kind = "expected"
        cov = velocity_pinv(J if kind == "observed" else F, c, E, seen)
        gv = as_f64(g).reshape(-1)
        delta = cov @ gv
        dec = float(gv @ delta)
        out = {"vel": vel, "cov": cov, "n_iter": it, "decrement": dec, "lnp_start": lnp0, "lnp": lnp, "converged": dec <= tol,
               "cov_kind": kind, "n_fallback": n_fallback}
        if dec <= tol or it >= max_iter:
            return out
        n_fallback += kind == "expected"
        step, moved = 1.0, False
        for _ in range(60):
            trial = vel + step * delta.reshape(c, E)
            v = float(value(trial))
            if v >= ref:
                vel, ref, moved = trial, v, True
                break
            step *= 0.5
        it += 1
        if not moved:
            out.update(n_iter=it, converged=False, n_fallback=n_fallback)
            return out


class EpochVelocities:
    """What ``epoch_velocities`` returns: ``dates`` (E,), ``vel`` (c, E), ``cov`` (c E, c E) ``= F^+`` (``cov_kind``
    ``"expected"``; with ``method="newton"`` ``J^+``, ``"observed"``, unless the last iteration fell back), ``sigma`` (c, E) (NaN
    for an epoch no chunk sees), ``n_iter``, ``decrement``, ``lnp_start``, ``lnp``, ``converged``.  The errors are those of
    RELATIVE velocities at FIXED hyper-parameters: the constant shift of each component is a null direction of the
    likelihood and is never moved -- each component's mean over the seen epochs stays the orbit's."""

    def __init__(self, dates, fit, seen):
        self.dates = as_f64(dates)
        self.vel, self.cov = fit["vel"], fit["cov"]
        c, E = self.vel.shape
        self.seen = np.asarray(seen, dtype=bool)
        self.sigma = np.where(self.seen[None, :], np.sqrt(np.maximum(np.diag(self.cov), 0.0)).reshape(c, E), np.nan)
        self.n_iter, self.decrement, self.converged = fit["n_iter"], fit["decrement"], fit["converged"]
        self.lnp_start, self.lnp = fit["lnp_start"], fit["lnp"]
        self.cov_kind, self.n_fallback = fit.get("cov_kind", "expected"), fit.get("n_fallback", 0)

    def write_table(self, fname):
        """``date, v_0, sigma_0, v_1, sigma_1, ...`` per epoch, one row each, with ``np.savetxt``"""
        cols = [self.dates]
        for k in range(self.vel.shape[0]):
            cols += [self.vel[k], self.sigma[k]]
        head = "date " + " ".join(f"v_{k} sigma_{k}" for k in range(self.vel.shape[0]))
        np.savetxt(fname, np.column_stack(cols), header=head)
        return fname


def epoch_velocities(workers, p, max_iter=20, tol=1e-10, mu_GP=1.0, vel0=None, method="scoring"):
    """The radial velocity of every component at every epoch with its error bar, free of any orbit model: Fisher scoring
    on the velocity table of the SUM of the workers' likelihoods, from the orbit's velocities at the fitted vector ``p``
    with the GP parameters of ``p`` held fixed.  The workers must share ``dates``.  Per iteration the summed
    ``g = sum_k grad_vel_k`` (``ChunkWorker.lnlike_grad_vel``) and ``F = sum_k F_k`` (``ChunkWorker.fisher_vel_at``), the
    step ``F^+ g`` with the pseudo-inverse taken on the complement of the ``c`` per-component constant vectors and of the
    epochs no chunk sees (a chunk in which an epoch is fully masked contributes zeros for it), halved until the summed
    likelihood (``ChunkHandle.upload_velocities``) does not decrease; it stops when the Newton decrement
    ``g^T F^+ g <= tol`` -- dimensionless, half of it the expected gain in ``lnp``: every velocity is then within
    ``sqrt(tol)`` of its error bar from the stationary point.  -> ``EpochVelocities``.

    The errors are those of RELATIVE velocities AT FIXED hyper-parameters: each component's constant shift is a null
    direction (the kernel is stationary) and its plain mean over the seen epochs stays the orbit's (the plain mean, not a
    weighted one, on purpose: the null vector of ``F`` is the constant vector, and a step in its complement keeps that mean); the cross information with
    ``(amp, l)`` stays with ``fisher_information``.  Workers with a baseline are refused by the default method;
    ``method="newton"`` is the path that accepts them.  ``vel0`` (c, E): a table to start from instead of the orbit's (an earlier fit; its
    per-component means are then the ones that stay).  Fisher scoring converges linearly -- the information is the expected
    curvature, not the data's own -- so ``converged`` can be False after ``max_iter``; the result then still never lowered
    ``lnp``, and ``decrement`` says how far it is.

    ``method="newton"``: Newton's method on the OBSERVED information (``velocity_newton``), one ``ChunkWorker.info_vel_at``
    per worker and iteration -- value, gradient, ``F`` and ``J`` from one factorisation -- with quadratic convergence near
    the optimum, ``cov = J^+`` there (``cov_kind``), and a fall-back to the scoring step wherever ``J`` is not positive
    definite on the complement.  Workers with a baseline are fitted under their marginal likelihood: a per-epoch continuum
    offset within the prior does not bias the velocities."""
    from .orbit import velocities
    if method not in ("scoring", "newton"):
        raise ValueError("epoch_velocities: method must be 'scoring' or 'newton'")
    workers = list(workers) if isinstance(workers, (list, tuple)) else [workers]
    w0 = workers[0]
    if os.environ.get("PSOAP_GPU_SERVER", "").strip().lower() not in ("", "0"):
        raise _lib.PsoapError("epoch_velocities needs the device in this process (PSOAP_GPU_SERVER serves values only)")
    for w in workers:
        if method == "scoring":
            w._no_baseline("epoch_velocities")
        if w.model != w0.model or w.dates.shape != w0.dates.shape or not np.array_equal(w.dates, w0.dates):
            raise ValueError("epoch_velocities: the workers must share the model and the dates")
    c, E = N_COMPONENTS[w0.model], w0.dates.shape[0]
    p_orb, p_gp = convert_vectors(np.atleast_2d(p), w0.model, w0.fix_params, **w0.defaults)
    gp = as_f64(p_gp[0], (2 * c,))
    if vel0 is None:
        vel0 = velocities(w0.model, as_f64(p_orb[:1]), w0.dates, device=w0.handle.device)[0]
    vel0 = as_f64(vel0, (c, E))
    seen = np.zeros(E, dtype=bool)
    for w in workers:
        seen |= np.bincount(w.epoch_index, minlength=E) > 0

    if method == "newton":
        def info(vel):
            lnp, g, F, J = 0.0, np.zeros((c, E)), np.zeros((c * E, c * E)), np.zeros((c * E, c * E))
            for w in workers:
                lnp_w, g_w, F_w, J_w = w.info_vel_at(vel, gp, mu_GP)
                lnp, g, F, J = lnp + lnp_w, g + g_w, F + F_w, J + J_w
            return lnp, g, F, J

        def value_newton(vel):
            from .data import c_kms
            if np.any(np.abs(vel) >= c_kms):
                return -np.inf
            total = 0.0
            for w in workers:
                lwls = w._grids_at(vel, "epoch_velocities", baseline_ok=True)[0]
                if w.baseline is not None:
                    total += float(w.handle.lnlike_marg(lwls, gp, mu_GP))
                else:
                    total += float(w.handle.lnlike_batch(lwls[None], gp[None], mu_GP)[0])
            return total

        return EpochVelocities(w0.dates, velocity_newton(value_newton, info, vel0, seen, max_iter, tol), seen)

    def value(vel):
        from .data import c_kms
        if np.any(np.abs(vel) >= c_kms):
            return -np.inf
        for w in workers:
            w.handle.upload_velocities(vel[None], gp[None], mu_GP)
        for w in workers:
            w.handle.eval()
        return float(sum(float(w.handle.fetch()[0]) for w in workers))

    def grad_info(vel):
        g, F = np.zeros((c, E)), np.zeros((c * E, c * E))
        for w in workers:
            g += w.lnlike_grad_vel(vel, gp, mu_GP)[1]
            F += w.fisher_vel_at(vel, gp)
        return g, F

    return EpochVelocities(w0.dates, velocity_scoring(value, grad_info, vel0, seen, max_iter, tol), seen)
