"""GPU tests of the observed information of the epoch velocities (psoap_chunk_info_vel, psoap_amd/csrc/vel_newton_kernels.hpp)
and of the Newton fit on top of it (psoap_amd.lnprob.epoch_velocities(method="newton")).

Shapes (tests/vel_newton_reference.py: SHAPES): the cases of fisher_reference.CASES -- one tile, exactly 128, 129, three ragged
tiles, c = 1, 2, 3 -- c E = 33 and 36, an empty epoch among unequal ones, pixels permuted at random at N = 300, and whole
epochs in shuffled order there; each plain and under a baseline of order 0 and 2.  A baseline takes the pixels of an epoch
contiguous only, so the permuted shape under a baseline is that refusal, and the shuffled whole epochs are the shape on which
the pair pass sorts a tile's column slots under Kt^-1 and alpha_m.  lnp, grad, F and J against the long-double generic reference (info_ext), F and J
relative to sqrt(F_ss F_tt), grad to sqrt(F_ss).

The tolerances are derived, not fitted: the float64 twin of the structured form (info_f64) measured against the long-double
reference on these very shapes (python tests/vel_newton_reference.py, last row), times the project's margin of 8:

                          lnp       grad          F          J
    max              6.54e-14   5.22e-12   2.37e-12   6.31e-13        (the order-2 baselines set all four)

Against the device's own lnlike / lnlike_grad (lnlike_marg / lnlike_marg_grad) the two sides' tolerances add: twice the bound.
"""
import numpy as np
import pytest

import vel_fisher_reference as vr
import vel_newton_reference as nr
from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu

TOL = nr.TOL


def _handle(pr, order=None, **kw):
    from psoap_amd.chunk import ChunkHandle
    h = ChunkHandle(pr.fl, pr.sigma, **kw)
    if order is not None:
        x, ep, E, order, sd, weight = nr.baseline_args(pr, order)
        h.set_baseline(order, x, ep, E, sd, weight)
    return h


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).copy()


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("order", nr.BASELINES, ids=lambda o: "plain" if o is None else f"b{o}")
@pytest.mark.parametrize("shape", nr.SHAPES, ids=lambda s: s.name)
def test_against_long_double(shape, order):
    pr = nr.problem(shape)
    if shape.perm_seed is not None and order is not None:
        # psoap_chunk_set_baseline takes the pixels of an epoch contiguous only: on permuted pixels there is no baseline to
        # evaluate under, and the case is that refusal
        from psoap_amd._lib import PsoapError
        with pytest.raises(PsoapError, match="not contiguous"):
            _handle(pr, order)
        return
    ref = nr.shape_ext(shape, order)
    T = pr.c * pr.E
    with _handle(pr, order) as h:
        got = h.info_vel(pr.lwls, pr.gp, pr.ep, pr.E, nr.MU_GP, marg=order is not None)
        again = h.info_vel(pr.lwls, pr.gp, pr.ep, pr.E, nr.MU_GP, marg=order is not None)
        if order is None:
            F_old = h.fisher_vel(pr.lwls, pr.gp, pr.ep, pr.E)
            lnp_dev = float(h.lnlike_batch(pr.lwls[None], pr.gp[None], nr.MU_GP)[0])
            g_lwl = h.lnlike_grad(pr.lwls, pr.gp, nr.MU_GP)[2]
        else:
            lnp_dev = float(h.lnlike_marg(pr.lwls, pr.gp, nr.MU_GP))
            g_lwl = h.lnlike_marg_grad(pr.lwls, pr.gp, nr.MU_GP)[2]
    from psoap_amd.covariance import velocity_gradient
    lnp, g, F, J = got
    err = nr.errors((lnp, g.reshape(-1), F, J), ref)
    d = np.sqrt(np.abs(np.diag(F)))
    scale = d * np.sum(d)
    scale[scale == 0.0] = 1.0
    null = float(max(np.max(np.abs(J @ u) / scale) for u in vr.null_vectors(pr.c, pr.E)))
    g_dev = velocity_gradient(g_lwl, pr.ep, pr.E)
    err_lnp_dev = abs(lnp - lnp_dev) / max(1.0, abs(lnp_dev))
    err_g_dev = nr.rel_to_scale(g, g_dev, ref[2])
    print(f"{shape.name} order {order}: " + ", ".join(f"{k} {err[k]:.2e} (bound {TOL[k]:.2e})" for k in nr.OUTPUTS)
          + f"; |J u_c| {null:.2e}; against the device's own lnp {err_lnp_dev:.2e}, grad {err_g_dev:.2e}")
    assert g.shape == (pr.c, pr.E) and F.shape == J.shape == (T, T)
    assert np.isfinite(lnp) and np.all(np.isfinite(g)) and np.all(np.isfinite(F)) and np.all(np.isfinite(J))
    assert _same_bits(J, J.T) and _same_bits(F, F.T)
    for a, b in zip(got, again):
        assert _same_bits(a, b)
    if order is None:
        assert _same_bits(F, F_old)
    for k in nr.OUTPUTS:
        assert err[k] <= TOL[k], k
    assert null <= TOL["J"]
    assert err_lnp_dev <= 2 * TOL["lnp"] and err_g_dev <= 2 * TOL["grad"]
    empty = np.flatnonzero(np.bincount(pr.ep, minlength=pr.E) == 0)
    for e in empty:
        rows = [k * pr.E + e for k in range(pr.c)]
        assert np.all(J[rows] == 0.0) and np.all(J[:, rows] == 0.0) and np.all(F[rows] == 0.0) and np.all(g[:, e] == 0.0)
    if shape.name == "N300-empty":
        assert empty.tolist() == [1]


def test_conventions_refusals_and_release():
    import ctypes
    from psoap_amd._lib import PsoapError, as_f64, dptr
    from psoap_amd.chunk import ChunkHandle
    shape = nr.SHAPES[4]
    pr = nr.problem(shape)
    c, E, ep = pr.c, pr.E, pr.ep
    gps = syn.make_walkers(c, 4, seed=8500)
    lw = np.repeat(pr.lwls[None], 4, axis=0)
    with _handle(pr, max_batch=4) as h:
        before = h.lnlike_batch(lw, gps, 0.9)
        good = h.info_vel(pr.lwls, pr.gp, ep, E, nr.MU_GP)
        assert _same_bits(h.lnlike_batch(lw, gps, 0.9), before)      # the likelihood's workspaces are left as they were
        assert _same_bits(h.info_vel(pr.lwls, pr.gp, ep, mu_GP=nr.MU_GP)[3], good[3])      # n_epochs defaults to max + 1
        neg = pr.gp.copy()
        neg[0] = -neg[0]
        lnp, g, F, J = h.info_vel(pr.lwls, neg, ep, E)              # status 0: no exception
        assert lnp == -np.inf and np.all(np.isnan(g)) and np.all(np.isnan(F)) and np.all(np.isnan(J))
        assert g.shape == (c, E) and J.shape == (c * E, c * E)
        with pytest.raises(PsoapError, match="set_baseline"):
            h.info_vel(pr.lwls, pr.gp, ep, E, marg=True)
        # ... and past ChunkHandle's own check, the library's
        T = c * E
        out = [np.empty(1), np.empty(T), np.empty((T, T)), np.empty((T, T))]
        ep32 = np.ascontiguousarray(ep, dtype=np.int32)
        rc = h._L.psoap_chunk_info_vel(h._h, 1, c, dptr(as_f64(pr.lwls)), dptr(as_f64(pr.gp)), nr.MU_GP, E,
                                       ep32.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), *[dptr(a) for a in out])
        assert rc == 2 and h._L.psoap_last_error() == b"psoap_chunk_info_vel: call psoap_chunk_set_baseline first"
        bad = ep.copy()
        bad[17] = E
        with pytest.raises(PsoapError, match="epoch index out of range"):
            h.info_vel(pr.lwls, pr.gp, bad, E)
        bad[17] = -1
        with pytest.raises(PsoapError, match="epoch index out of range"):
            h.info_vel(pr.lwls, pr.gp, bad, E)
        with pytest.raises(PsoapError, match="n_epochs must be at least 1"):
            h.info_vel(pr.lwls, pr.gp, ep, 0)
        with pytest.raises(PsoapError, match="at most 2048"):
            h.info_vel(pr.lwls, pr.gp, ep, 2049)
        h.stream_open(c, 1)
        try:
            with pytest.raises(PsoapError, match="open stream"):
                h.info_vel(pr.lwls, pr.gp, ep, E)
        finally:
            h.stream_close()
        # release, twice, then another call: the workspace comes back, and so do the bits
        h.fisher_vel_release()
        h.fisher_vel_release()
        h.fisher_release()
        for a, b in zip(h.info_vel(pr.lwls, pr.gp, ep, E, nr.MU_GP), good):
            assert _same_bits(a, b)
    # not positive definite: zero noise and two identical pixels
    lw1 = pr.lwls.copy()
    lw1[:, 1] = lw1[:, 0]
    with ChunkHandle(pr.fl, np.zeros_like(pr.sigma)) as h:
        lnp, g, F, J = h.info_vel(lw1, pr.gp, ep, E)
        assert lnp == -np.inf and np.all(np.isnan(g)) and np.all(np.isnan(F)) and np.all(np.isnan(J))


def test_covariance_velocity_information_observed():
    from psoap_amd import covariance
    shape = nr.SHAPES[0]
    pr = nr.problem(shape)
    x, ep, E, order, sd, weight = nr.baseline_args(pr, 0)
    try:
        plain = covariance.velocity_information_observed(pr.lwls, pr.fl, pr.sigma, pr.gp, pr.ep, nr.MU_GP)
        marg = covariance.velocity_information_observed(pr.lwls, pr.fl, pr.sigma, pr.gp, pr.ep, nr.MU_GP,
                                                        baseline={"x": x, "epoch_index": ep, "order": 0, "prior_sd": sd})
        bad = covariance.velocity_information_observed(pr.lwls, pr.fl, pr.sigma, [-0.2, 5.0, 0.1, 7.0], pr.ep)
    finally:
        covariance.release_handles()
    assert bad[0] == -np.inf and np.all(np.isnan(bad[3])) and bad[3].shape == plain[3].shape
    for got, o in ((plain, None), (marg, 0)):
        err = nr.errors((got[0], got[1].reshape(-1), got[2], got[3]), nr.shape_ext(shape, o))
        assert all(err[k] <= TOL[k] for k in nr.OUTPUTS), err


# ---- the fit: lnprob.epoch_velocities(method="newton") --------------------------------------------------------------------
def _fit_worker(ch, fl=None, **kw):
    from psoap_amd.lnprob import ChunkWorker
    from psoap_amd.utils import registered_params
    full = dict(zip(registered_params["SB2"], list(syn.ORBIT_BASE["SB2"]) + list(vr.fit_gp())))
    w = ChunkWorker("SB2", ch.lwl, ch.fl if fl is None else fl, ch.sigma, ch.epoch_index, ch.dates, defaults=full, **kw)
    return np.array([full[n] for n in registered_params["SB2"]]), w


def _check_fit(res, twin, start):
    sig = np.sqrt(np.diag(twin["cov"])).reshape(twin["vel"].shape)
    off = np.max(np.abs(res.vel - twin["vel"]) / sig)
    mean_shift = np.max(np.abs(res.vel.mean(axis=1) - start.mean(axis=1)))
    print(f"device newton: {res.n_iter} iterations (twin {twin['n_iter']}), decrement {res.decrement:.2e}, lnp {res.lnp_start:.6f} -> "
          f"{res.lnp:.6f}; max |v - twin| / sigma {off:.2e}; mean shift {mean_shift:.2e} km/s; {res.cov_kind}, "
          f"{res.n_fallback} fall-backs")
    assert res.converged and res.decrement <= 1e-10 and abs(res.n_iter - twin["n_iter"]) <= 1
    assert res.lnp >= res.lnp_start
    assert mean_shift <= 1e-12 * 60.0
    assert off <= 1e-4                      # the rule of tests/test_gpu_vel_fisher.py::test_fit_against_the_cpu_twin
    assert res.cov_kind == twin["cov_kind"] == "observed"
    assert np.max(np.abs(res.sigma - sig)) <= 1e-4 * np.max(sig)


def test_newton_fit_against_the_cpu_twin_and_scoring():
    """vel_fisher_reference.fit_chunk() from 1 km/s off the scoring twin's optimum, as the scoring fit test starts"""
    from psoap_amd import lnprob
    ch = vr.fit_chunk()
    _, start = vr.cpu_fit_optimum()
    twin = nr.cpu_newton(ch, vr.fit_gp(), start)
    p, w = _fit_worker(ch)
    try:
        res = lnprob.epoch_velocities([w], p, mu_GP=vr.FIT_MU, vel0=start, method="newton")
        scoring = lnprob.epoch_velocities([w], p, mu_GP=vr.FIT_MU, vel0=start)
    finally:
        w.close()
    _check_fit(res, twin, start)
    print(f"scoring: {scoring.n_iter} iterations, {scoring.cov_kind}")
    assert res.n_iter <= scoring.n_iter and scoring.cov_kind == "expected"


def test_newton_converges_where_scoring_does_not():
    """seed HARD_SEED of 7903 .. 7924 from the chunk's true velocities: the scoring twin misses the decrement in 20 iterations,
    the Newton twin reaches it (vel_newton_reference.seed_table, profiles/vel_newton.md)"""
    from psoap_amd import lnprob
    ch = nr.fit_chunk(nr.HARD_SEED)
    start = ch.velocities
    twin = nr.cpu_newton(ch, vr.fit_gp(), start)
    assert twin["converged"] and not vr.cpu_fit(ch, vr.fit_gp(), start)["converged"]
    p, w = _fit_worker(ch)
    try:
        res = lnprob.epoch_velocities([w], p, mu_GP=vr.FIT_MU, vel0=start, method="newton")
    finally:
        w.close()
    _check_fit(res, twin, start)


def test_baseline_worker_is_not_biased_by_continuum_offsets():
    """a per-epoch continuum offset drawn from the baseline's prior: the velocities fitted under the baseline stay within their
    own error bars of those from the unoffset flux (the plain fit moves by more: tests/test_vel_newton_reference.py)"""
    from psoap_amd import lnprob
    from psoap_amd._lib import PsoapError
    ch = vr.fit_chunk()
    fl_off, _ = nr.offset_flux(ch)
    start = ch.velocities
    p, w0 = _fit_worker(ch, baseline=dict(nr.FIT_BASELINE))
    _, w1 = _fit_worker(ch, fl_off, baseline=dict(nr.FIT_BASELINE))
    try:
        with pytest.raises(PsoapError, match="this worker has a baseline"):
            lnprob.epoch_velocities([w0], p, mu_GP=vr.FIT_MU, vel0=start)
        clean = lnprob.epoch_velocities([w0], p, mu_GP=vr.FIT_MU, vel0=start, method="newton")
        offset = lnprob.epoch_velocities([w1], p, mu_GP=vr.FIT_MU, vel0=start, method="newton")
        lnp, g, F, J = w1.info_vel_at(offset.vel, vr.fit_gp(), vr.FIT_MU)
        want = w1.handle.lnlike_marg(ch.lwl[None, :] + (-offset.vel[:, ch.epoch_index]) / vr.C_KMS, vr.fit_gp(), vr.FIT_MU)
        fast = start.copy()
        fast[1, 2] = 3.0e5
        assert w1.info_vel_at(fast, vr.fit_gp())[0] == -np.inf and np.all(np.isnan(w1.info_vel_at(fast, vr.fit_gp())[3]))
    finally:
        w0.close()
        w1.close()
    twin = nr.cpu_newton(ch, vr.fit_gp(), start, fl=fl_off, order=0, sd=nr.FIT_BASELINE["sd"])
    shift = np.max(np.abs(offset.vel - clean.vel) / offset.sigma)
    sig = np.sqrt(np.diag(twin["cov"])).reshape(twin["vel"].shape)
    off = np.max(np.abs(offset.vel - twin["vel"]) / sig)
    print(f"baseline fits: {clean.n_iter} and {offset.n_iter} iterations; max |v_offset - v_clean| / sigma {shift:.3f}; "
          f"against the twin {off:.2e}")
    assert clean.converged and offset.converged and offset.cov_kind == "observed"
    assert shift <= 1.0
    assert off <= 1e-4 and abs(offset.n_iter - twin["n_iter"]) <= 1
    assert abs(lnp - float(want)) <= 2 * TOL["lnp"] * max(1.0, abs(float(want))) and J.shape == (12, 12)
