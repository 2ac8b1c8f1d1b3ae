"""GPU tests of the time scales at the ``lnprob(p)`` boundary: ``upload_*`` + ``set_tau`` + ``eval`` (psoap_batch_set_tau),
``lnprob_tv_grad`` (psoap_chunk_lnprob_tv_grad) and a ``ChunkWorker(timevar=...)`` under the lock-step sampler.

Values: relative 1e-10 on lnp against the long-double chain of tests/timevar_sampling_reference.py, as the sibling tests.

Gradients: each output within 8 times the float64 twin's error against long double on these cases, measured on the CPU
(``python tests/timevar_sampling_reference.py``), 8 being the margin of tests/test_gpu_grad.py:

    case              b   grad_orb    grad_gp   grad_tau    grad_mu
    SB2-N100          0   2.27e-17   1.88e-17   2.55e-17   5.74e-18
    SB2-N100          4   1.51e-17   5.57e-17   1.09e-17   1.57e-17
    SB2-N129          0   6.95e-18   1.33e-17   1.14e-17   6.88e-18
    SB2-N129          4   3.08e-17   4.12e-17   7.13e-17   9.60e-18
    ST3-N300          0   6.04e-18   1.25e-17   5.00e-18   2.75e-18
    ST3-N300          4   3.46e-17   1.85e-16   3.42e-17   8.01e-18
    SB1-N128          0   7.03e-18   3.32e-17   8.37e-19   2.01e-17
    SB1-N128          4   3.67e-17   2.92e-17   0.00e+00   1.54e-17
    SB2-N129-perm     0   1.71e-17   6.77e-17   8.66e-18   1.74e-17
    SB2-N129-perm     4   8.22e-18   1.17e-17   9.09e-17   3.78e-17
    max                   3.67e-17   1.85e-16   9.09e-17   3.78e-17

The three seeded defects of the reference module (tau read as (c, B), times not permuted with the pixels, the previous
upload's tau kept) move lnp by 1e-1 .. 1e+2 relative on these cases (tests/test_timevar_vectors.py checks it on the CPU).
"""
import numpy as np
import pytest

import timevar_sampling_reference as tsr
from psoap_amd import utils

pytestmark = pytest.mark.gpu

MARGIN = 8
TOL = {"orb": MARGIN * 3.67e-17, "gp": MARGIN * 1.85e-16, "tau": MARGIN * 9.09e-17, "mu": MARGIN * 3.78e-17}
LNP_RTOL = 1e-10
MU = tsr.MU_GP
INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).copy()


def _worker(case, timevar=True, **kw):
    from psoap_amd.lnprob import ChunkWorker
    d = tsr.case_data(case)
    if timevar:
        kw["timevar"] = {"fit": [True] * case.c, "tau": [INF] * case.c}
    kw.setdefault("max_batch", tsr.B_MAX)
    return ChunkWorker(case.model, d.lwl, d.fl, d.sigma, d.epoch_index, d.dates, **kw)


def _vectors(case, B=tsr.B_MAX):
    """fitted vectors (B, n_orb + 2c + c): nothing fixed, every tau fitted"""
    d = tsr.case_data(case)
    return utils.join_vectors_timevar(np.hstack([d.p_orb[:B], d.gp[:B]]), d.tau[:B], [True] * case.c)


def _eval(w, p_orb, gp, tau):
    w.upload_orbits(p_orb, gp, MU, tau)
    w.handle.eval()
    return w.handle.fetch()


# ---- 1. values against long double, B across the gradient's group of 8 and the stream-group split ---------------------------
@pytest.mark.parametrize("B", (1, 8, 9))
@pytest.mark.parametrize("case", tsr.CASES, ids=lambda c: c.id)
def test_lnprob_batch_against_long_double(case, B):
    w = _worker(case)
    try:
        assert np.array_equal(w.times, tsr.case_data(case).times)
        got = w.lnprob_batch(_vectors(case, B), MU)
    finally:
        w.close()
    want = np.array([tsr.chain_ext(case, b).lnp for b in range(B)])
    rel = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{case.id} B={B}: largest relative error of lnp {rel.max():.2e} (bound {LNP_RTOL:.0e})")
    assert got.shape == (B,) and np.all(rel <= LNP_RTOL), (got, want)


# ---- 2. gradients against long double ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tsr.CASES, ids=lambda c: c.id)
def test_lnprob_tv_grad_against_long_double(case):
    d = tsr.case_data(case)
    w = _worker(case)
    try:
        lnp, g_orb, g_gp, g_tau, g_mu = w.lnprob_grad_orbits(d.p_orb, d.gp, MU, tau=d.tau)          # B = 9: two groups
        lnp_v, grad_v = w.lnprob_grad_batch(_vectors(case), MU)
        one = w.lnprob_grad_orbits(d.p_orb[4:5], d.gp[4:5], MU, tau=d.tau[4:5])
        val = _eval(w, d.p_orb, d.gp, d.tau)
    finally:
        w.close()
    # the vector form is the same call: every column, the tau entries last, in component order
    assert np.array_equal(_bits(lnp_v), _bits(lnp)) and np.array_equal(_bits(grad_v), _bits(np.hstack([g_orb, g_gp, g_tau])))
    # a proposal's bits depend neither on B nor on its position
    for a, b in zip(one, (lnp[4:5], g_orb[4:5], g_gp[4:5], g_tau[4:5], g_mu[4:5])):
        assert np.array_equal(_bits(a), _bits(b))
    # grad_tau is exactly +0 where tau = inf
    assert d.tau[4, case.c - 1] == INF and _bits(g_tau[4, case.c - 1]) == 0
    for b in tsr.GRAD_PROPOSALS:
        ref = tsr.chain_ext(case, b)
        err = tsr.errors(g_orb[b], g_gp[b], g_tau[b], g_mu[b], ref)
        print(f"{case.id} b={b}: lnp {lnp[b]!r} ext {ref.lnp!r}; error / S: " +
              ", ".join(f"{k} {v:.2e} (bound {TOL[k]:.2e})" for k, v in err.items()))
        assert abs(lnp[b] - ref.lnp) <= LNP_RTOL * max(1.0, abs(ref.lnp))
        for k in err:
            assert err[k] <= TOL[k], (k, b, err[k], TOL[k])
    # the batch route and the gradient entry compute the same likelihood
    assert np.all(np.abs(val - lnp) <= LNP_RTOL * np.maximum(1.0, np.abs(lnp)))


# ---- 3. bit contracts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (tsr.CASES[2], tsr.CASES[4]), ids=lambda c: c.id)
def test_tau_inf_has_the_bits_of_the_plain_staged_evaluation(case):
    d = tsr.case_data(case)
    plain, w = _worker(case, timevar=False), _worker(case)
    try:
        plain.handle.set_mode("staged")
        plain.upload_orbits(d.p_orb, d.gp, MU)
        plain.handle.eval()
        want = plain.handle.fetch()
        got = _eval(w, d.p_orb, d.gp, None)          # the defaults: every tau = inf
        g = w.lnprob_grad_orbits(d.p_orb[:2], d.gp[:2], MU)
        g0 = plain.lnprob_grad_orbits(d.p_orb[:2], d.gp[:2], MU)
    finally:
        plain.close()
        w.close()
    assert np.all(np.isfinite(want)) and np.array_equal(_bits(got), _bits(want))
    # the gradient entries: grad_tau exactly +0, everything else the bits of lnprob_grad
    assert np.all(_bits(g[3]) == 0)
    for a, b in zip((g[0], g[1], g[2], g[4]), g0):
        assert np.array_equal(_bits(a), _bits(b))


def test_bits_do_not_depend_on_batch_position_stream_groups_or_mode():
    from psoap_amd import _lib
    case = tsr.CASES[1]
    d = tsr.case_data(case)
    w = _worker(case)
    try:
        full = _eval(w, d.p_orb, d.gp, d.tau)
        for k in (0, 3, 8):
            alone = _eval(w, d.p_orb[k:k + 1], d.gp[k:k + 1], d.tau[k:k + 1])
            assert np.array_equal(_bits(alone), _bits(full[k:k + 1])), k
        # the same proposal at another position
        order = np.array([8, 3, 0, 1, 2, 4, 5, 6, 7])
        assert np.array_equal(_bits(_eval(w, d.p_orb[order], d.gp[order], d.tau[order])), _bits(full[order]))
        for groups in (1, 3, 4):
            w.handle.set_stream_groups(groups)
            assert np.array_equal(_bits(_eval(w, d.p_orb, d.gp, d.tau)), _bits(full)), groups
        # set_mode("dag") with time scales: still the staged bits, no persistent launch, not a policy event
        w.handle.set_stream_groups(2)
        w.handle.set_mode("dag")
        forms, share = _lib.dag_form_launches(), _lib.share_stats()
        assert np.array_equal(_bits(_eval(w, d.p_orb, d.gp, d.tau)), _bits(full))
        assert _lib.dag_form_launches() == forms
        after = _lib.share_stats()
        assert after["staged_policy"] == share["staged_policy"] and after["dag_launches"] == share["dag_launches"]
        w.handle.set_mode("staged")
        assert np.array_equal(_bits(_eval(w, d.p_orb, d.gp, d.tau)), _bits(full))
    finally:
        w.close()


# ---- 4. conventions ------------------------------------------------------------------------------------------------------------
def test_a_tau_that_is_no_time_scale_and_a_fast_orbit_give_minus_inf_there_alone():
    case = tsr.CASES[0]
    d = tsr.case_data(case)
    w = _worker(case)
    try:
        full = _eval(w, d.p_orb, d.gp, d.tau)
        g_full = w.lnprob_grad_orbits(d.p_orb, d.gp, MU, tau=d.tau)
        assert np.all(np.isfinite(full))
        for k, bad in ((2, 0.0), (8, -3.0), (0, float("nan"))):
            tau = d.tau.copy()
            tau[k, 1] = bad
            got = _eval(w, d.p_orb, d.gp, tau)
            keep = np.arange(tsr.B_MAX) != k
            assert got[k] == -np.inf and np.array_equal(_bits(got[keep]), _bits(full[keep])), (k, bad)
            g = w.lnprob_grad_orbits(d.p_orb, d.gp, MU, tau=tau)
            assert g[0][k] == -np.inf and all(np.all(np.isnan(a[k])) for a in g[1:])
            assert all(np.array_equal(_bits(a[keep]), _bits(b[keep])) for a, b in zip(g, g_full))
            # the next upload starts from clean flags
            assert np.array_equal(_bits(_eval(w, d.p_orb, d.gp, d.tau)), _bits(full))
        # a faster-than-light orbit in one proposal
        fast = d.p_orb.copy()
        fast[5, 1] = 4.0e5          # K of SB2, km/s
        got = _eval(w, fast, d.gp, d.tau)
        keep = np.arange(tsr.B_MAX) != 5
        assert got[5] == -np.inf and np.array_equal(_bits(got[keep]), _bits(full[keep]))
        g = w.lnprob_grad_orbits(fast, d.gp, MU, tau=d.tau)
        assert g[0][5] == -np.inf and all(np.all(np.isnan(a[5])) for a in g[1:])
        assert all(np.array_equal(_bits(a[keep]), _bits(b[keep])) for a, b in zip(g, g_full))
        assert np.array_equal(_bits(_eval(w, d.p_orb, d.gp, d.tau)), _bits(full))
    finally:
        w.close()


def test_set_tau_is_cleared_by_the_next_upload():
    case = tsr.CASES[0]
    d = tsr.case_data(case)
    B = 3
    lwls = np.stack([tsr.shifted_f64(case, d.p_orb[b]) for b in range(B)])
    w = _worker(case)
    h = w.handle
    try:
        h.set_mode("staged")

        def run(tau):
            h.upload(lwls, d.gp[:B], MU)
            if tau is not None:
                h.set_tau(tau)
            h.eval()
            return h.fetch()

        static = run(np.full((B, case.c), INF))
        a, b = run(d.tau[:B]), run(d.tau[:B])          # both slots have carried finite time scales
        assert np.array_equal(_bits(a), _bits(b)) and not np.array_equal(_bits(a), _bits(static))
        assert np.array_equal(_bits(run(None)), _bits(static)) and np.array_equal(_bits(run(None)), _bits(static))
        # ... and a second set_tau for the same upload replaces the first
        h.upload(lwls, d.gp[:B], MU)
        h.set_tau(d.tau[:B] * 2.0)
        h.set_tau(d.tau[:B])
        h.eval()
        assert np.array_equal(_bits(h.fetch()), _bits(a))
    finally:
        w.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    from psoap_amd import _lib
    from psoap_amd.chunk import ChunkGroup, ChunkHandle
    case = tsr.CASES[0]
    d = tsr.case_data(case)
    B = 2
    lwls = np.stack([tsr.shifted_f64(case, d.p_orb[b]) for b in range(B)])
    tau = d.tau[:B]
    # missing times
    with ChunkHandle(d.fl, d.sigma, max_batch=B) as h:
        h.upload(lwls, d.gp[:B], MU)
        with pytest.raises(_lib.PsoapError, match="psoap_batch_set_tau: call psoap_chunk_set_times first"):
            h.set_tau(tau)
        h.set_times(d.times)
        with pytest.raises(_lib.PsoapError, match="B and c must be those of the pending upload"):
            h.set_tau(d.tau[:3])
        h.set_tau(tau)
        # a pending upload with time scales: no group launch, no stream
        with ChunkHandle(d.fl, d.sigma, max_batch=B) as h2:
            h2.upload(lwls, d.gp[:B], MU)
            with ChunkGroup([h, h2]) as g:
                with pytest.raises(_lib.PsoapError, match="psoap_group_eval: a member's upload carries time scales"):
                    g.eval()
        with pytest.raises(_lib.PsoapError, match="psoap_stream_open: the handle's last upload carries time scales"):
            h.stream_open(case.c)
        h.eval()
        first = h.fetch()
        with pytest.raises(_lib.PsoapError, match="no upload is pending"):
            h.set_tau(tau)
        # the active slot still carries them
        with pytest.raises(_lib.PsoapError, match="psoap_stream_open"):
            h.stream_open(case.c)
        # an upload without time scales is what the next evaluation reads: the group launch takes it
        with ChunkHandle(d.fl, d.sigma, max_batch=B) as h2:
            h2.set_mode("staged")
            h2.upload(lwls, d.gp[:B], MU)
            h2.eval()
            static = h2.fetch()
            h.upload(lwls, d.gp[:B], MU)
            h2.upload(lwls, d.gp[:B], MU)
            with ChunkGroup([h, h2]) as g:
                g.eval()
                got, got2 = h.fetch(), h2.fetch()
            for v in (got, got2):
                assert np.all(np.abs(v - static) <= LNP_RTOL * np.abs(static))
        # an open stream
        h.stream_open(case.c)
        try:
            with pytest.raises(_lib.PsoapError, match=r"psoap_batch_set_tau: the handle has an open stream \(psoap_stream_close first\)"):
                h.set_tau(tau)
        finally:
            h.stream_close()
        h.upload(lwls, d.gp[:B], MU)
        h.set_tau(tau)
        h.eval()
        assert np.array_equal(_bits(h.fetch()), _bits(first))
    # a baseline
    w = _worker(case, timevar=False, max_batch=B, baseline={"order": 1, "sd": [0.05, 0.02]})
    try:
        w.handle.set_times(d.times)
        w.handle.upload(lwls, d.gp[:B], MU)
        with pytest.raises(_lib.PsoapError, match="psoap_batch_set_tau: the handle has a baseline .*psoap_chunk_lnlike_marg_tv"):
            w.handle.set_tau(tau)
        with pytest.raises(_lib.PsoapError, match="psoap_chunk_lnprob_tv_grad: the handle has a baseline"):
            w.handle.lnprob_tv_grad(utils.MODEL_ID[case.model], d.p_orb[:B], d.gp[:B], tau, MU)
    finally:
        w.close()
    # the worker's own refusals
    w = _worker(case)
    try:
        with pytest.raises(_lib.PsoapError, match="no temporal factor"):
            w.stream_open()
    finally:
        w.close()


def test_baseline_and_time_scales_together():
    """lnprob_batch through lnlike_marg_tv on host-shifted grids; the gradient through psoap_chunk_lnprob_marg_tv_grad; loo is
    refused"""
    from psoap_amd import _lib
    case = tsr.CASES[0]
    d = tsr.case_data(case)
    B = 3
    w = _worker(case, baseline={"order": 1, "sd": [0.05, 0.02]})
    try:
        ps = _vectors(case, B)
        got = w.lnprob_batch(ps, MU)
        lwls, fast = w.shifted_grids(d.p_orb[:B])
        want = w.handle.lnlike_marg_tv(lwls, d.gp[:B], d.tau[:B], MU)
        assert not fast.any() and np.all(np.isfinite(got)) and np.array_equal(_bits(got), _bits(want))
        lnp, grad = w.lnprob_grad_batch(ps, MU)
        assert grad.shape == ps.shape and np.all(np.isfinite(grad))
        assert np.all(np.abs(lnp - got) <= LNP_RTOL * np.maximum(1.0, np.abs(got)))
        # the tau columns against a central difference of the value (step 1e-4 relative: truncation ~1e-8, rounding ~1e-8)
        for k in range(case.c):
            col = ps.shape[1] - case.c + k
            hi, lo = ps[:1].copy(), ps[:1].copy()
            step = 1e-4 * ps[0, col]
            hi[0, col] += step
            lo[0, col] -= step
            fd = (w.lnprob_batch(hi, MU)[0] - w.lnprob_batch(lo, MU)[0]) / (2 * step)
            assert abs(fd - grad[0, col]) <= 1e-5 * max(abs(fd), abs(grad[0, col]), 1e-3), (k, fd, grad[0, col])
        F = w.fisher(ps[0])
        assert F.shape == (ps.shape[1],) * 2 and np.all(np.isfinite(F)) and np.array_equal(_bits(F), _bits(F.T))
        with pytest.raises(_lib.PsoapError, match="not built"):
            w.loo(ps[0], MU)
    finally:
        w.close()


def test_fisher_and_loo_dispatch_to_the_time_variable_forms():
    case = tsr.CASES[0]
    d = tsr.case_data(case)
    w = _worker(case)
    try:
        p = _vectors(case, 1)[0]
        F = w.fisher(p)
        lwls = w.shifted_grids(d.p_orb[:1])[0][0]
        n = p.shape[0]
        assert F.shape == (n, n) and np.all(np.isfinite(F)) and np.all(np.diag(F)[-case.c:] > 0)
        # the dtau block is fisher_tv's with unit time-scale tangents
        T = case.c
        want = w.handle.fisher_tv(lwls, d.gp[0], d.tau[0], np.zeros((T, 2 * case.c)), np.eye(T))
        assert np.allclose(F[-T:, -T:], want, rtol=1e-10, atol=0.0)
        r = w.loo(p, MU)
        want = w.handle.loo_tv(lwls, d.gp[0], d.tau[0], MU, d.epoch_index, len(d.dates))
        assert np.array_equal(_bits(r.pix_mean), _bits(want.pix_mean)) and r.lnp == want.lnp
    finally:
        w.close()


def test_value_only_call_of_the_gradient_entry():
    """grad_gp == NULL: the value alone, with the bits of the full call; a faster-than-light orbit still gives -inf"""
    from psoap_amd._lib import check, dptr
    case = tsr.CASES[0]
    d = tsr.case_data(case)
    B = tsr.B_MAX
    p_orb = d.p_orb.copy()
    p_orb[5, 1] = 4.0e5          # K of SB2, km/s
    w = _worker(case)
    try:
        full = w.lnprob_grad_orbits(p_orb, d.gp, MU, tau=d.tau)[0]
        lnp = np.full(B, np.nan)
        h = w.handle
        check(h._L.psoap_chunk_lnprob_tv_grad(h._h, B, utils.MODEL_ID[case.model], dptr(p_orb), dptr(d.gp), dptr(d.tau), MU,
                                              dptr(lnp), None, None, None, None, None), "psoap_chunk_lnprob_tv_grad")
        g_orb = np.empty((B, p_orb.shape[1]))
        rc = h._L.psoap_chunk_lnprob_tv_grad(h._h, B, utils.MODEL_ID[case.model], dptr(p_orb), dptr(d.gp), dptr(d.tau), MU,
                                             dptr(lnp.copy()), dptr(g_orb), None, None, None, None)
    finally:
        w.close()
    assert rc != 0          # a gradient without grad_gp is refused
    assert lnp[5] == -np.inf and np.isfinite(np.delete(lnp, 5)).all() and np.array_equal(_bits(lnp), _bits(full))


def test_fit_fisher_and_posterior_take_the_longer_vector():
    """lnprob.optimize_orbit, fisher_information, laplace_covariance and fisher_jumps on a timevar worker, and a
    sample_parallel.Posterior built with time scales"""
    from types import SimpleNamespace
    from psoap_amd import lnprob as plnprob
    from psoap_amd import sample_parallel as sp
    case = tsr.CASES[0]
    d = tsr.case_data(case)
    fit = [True, False]
    reg = utils.registered_params[case.model]
    pars = dict(zip(reg, np.concatenate([d.p_orb[0], d.gp[0]])))
    from psoap_amd.lnprob import ChunkWorker
    w = ChunkWorker(case.model, d.lwl, d.fl, d.sigma, d.epoch_index, d.dates, max_batch=4,
                    timevar={"fit": fit, "tau": [0.5 * d.span, INF]})
    try:
        p0 = utils.join_vectors_timevar(np.concatenate([d.p_orb[0], d.gp[0]]), [0.5 * d.span, INF], fit)[0]
        n = p0.shape[0]
        assert n == len(reg) + 1
        F = plnprob.fisher_information([w], p0)
        assert F.shape == (n, n) and np.array_equal(_bits(F), _bits(w.fisher(p0))) and F[-1, -1] > 0
        prec = 1e-6 * np.maximum(np.diag(F), 1e-12)          # a weak prior: a single small chunk does not constrain every orbit direction
        C = plnprob.laplace_covariance([w], p0, prior_precision=prec)
        J = plnprob.fisher_jumps([w], p0, prior_precision=prec)
        assert C.shape == (n, n) and np.all(np.diag(C) > 0) and np.allclose(J, 2.38 ** 2 / n * C, rtol=1e-14, atol=0.0)
        # a short fit inside a box of one per cent around the start: the summed lnprob does not go down, tau stays a time scale
        width = 0.01 * np.maximum(np.abs(p0), 1e-3)
        start = w.lnprob_grad(p0, MU)[0]
        res = plnprob.optimize_orbit([w], p0, bounds=list(zip(p0 - width, p0 + width)), mu_GP=MU, ftol=1e-7, full_output=True)
        assert res.x.shape == (n,) and np.isfinite(res.fun) and -res.fun >= start and res.x[-1] > 0
        lnp, g = w.lnprob_grad(res.x, MU)
        assert g.shape == (n,) and abs(lnp + res.fun) <= LNP_RTOL * abs(lnp)
    finally:
        w.close()
    chunk = SimpleNamespace(lwl=d.lwl, fl=d.fl, sigma=d.sigma, epoch_index=d.epoch_index, date1D=d.dates)
    tv = {"fit": np.array(fit), "tau": np.array([0.5 * d.span, INF])}
    post = sp.Posterior(case.model, [chunk], [], pars, max_batch=4, timevar=tv)
    try:
        assert post.group is None and not post.can_stream()
        P = utils.join_vectors_timevar(np.hstack([d.p_orb[:4], d.gp[:4]]), d.tau[:4], fit)
        P[2, -1] = -1.0          # no time scale: the prior decides, without a device call for that row's own value
        got = post.lnprob_batch(P)
        with pytest.raises(RuntimeError, match="no temporal factor"):
            post.stream_open()
    finally:
        post.close()
    for b in (0, 1, 3):
        want = tsr.chain_from(case.model, d.p_orb[b], d.gp[b], [d.tau[b, 0], INF], d.lwl, d.times, d.fl, d.sigma, d.epoch_index,
                              d.dates, 1.0).lnp
        assert abs(got[b] - want) <= LNP_RTOL * max(1.0, abs(want)), (b, got[b], want)
    assert got[2] == -np.inf


# ---- 6. the lock-step sampler on a timevar worker -----------------------------------------------------------------------------
def test_lockstep_sampler_stores_what_a_fresh_evaluation_returns():
    from psoap_amd.lnprob import ChunkWorker
    from psoap_amd.samplers import MultiChainMHSampler
    import grad_reference as gr
    from psoap_amd import synthetic as syn
    ch = gr.case_chunk((240, 2, 6, 50))
    dates = np.asarray(ch.dates, dtype=np.float64)
    span = float(dates.max() - dates.min())
    walkers, steps = 16, 10
    w = ChunkWorker("SB2", ch.lwl, ch.fl, ch.sigma, ch.epoch_index, dates, max_batch=walkers,
                    timevar={"fit": [True, False], "tau": [0.5 * span, INF]})
    calls = []

    def lnprob_batch(P):
        out = w.lnprob_batch(P, MU)
        calls.append((P.copy(), out.copy()))
        return out

    try:
        p0 = np.concatenate([syn.ORBIT_BASE["SB2"], syn.GP_BASE[2], [0.5 * span]])
        jumps = np.concatenate([[0.005, 0.05, 0.005, 0.3, 0.02, 0.02, 0.02], [0.002, 0.05, 0.002, 0.05], [0.05 * span]])
        s = MultiChainMHSampler(np.diag(jumps ** 2), p0.shape[0], lnprob_batch, walkers, seeds=list(range(40, 40 + walkers)))
        s.run_mcmc(p0, steps)
        assert s.chain.shape == (walkers, steps, 12) and np.all(np.isfinite(s.lnprobability))
        assert len(calls) == steps + 1 and s.naccepted.sum() > 0
        for i in range(steps):
            fresh = w.lnprob_batch(s.chain[:, i, :], MU)
            assert np.array_equal(_bits(fresh), _bits(s.lnprobability[:, i])), i
    finally:
        w.close()
    # the first step's proposals against the long-double chain
    P, got = calls[1]
    times = dates[ch.epoch_index] - dates[ch.epoch_index].min()
    for b in range(0, walkers, 3):
        tau = np.array([P[b, 11], INF])
        if not (tau[0] > 0 and np.isfinite(got[b])):
            continue
        want = tsr.chain_from("SB2", P[b, :7], P[b, 7:11], tau, ch.lwl, times, ch.fl, ch.sigma, ch.epoch_index, dates).lnp
        assert abs(got[b] - want) <= LNP_RTOL * max(1.0, abs(want)), (b, got[b], want)
    assert np.isfinite(got).sum() >= walkers // 2
