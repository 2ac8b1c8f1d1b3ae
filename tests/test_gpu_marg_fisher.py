"""GPU tests of the Fisher information and the leave-one-out cross-validation under the marginalised continuum
(psoap_chunk_fisher_marg, psoap_chunk_loo_marg, psoap_amd/csrc/marg_fisher_kernels.hpp).

The cases of tests/marg_reference.py (one tile and Q = 1; an exact tile; one pixel into the second tile with q = 9; epoch
edges on tile edges; an empty epoch with runs not in id order; Q = 2, so the second K loop spans two slots and M crosses a
block row) with both weights, the tangents of tests/marg_fisher_reference.py.  The device against the long-double reference
on the dense K + H Lambda H^T: F relative to sqrt(F_ss F_tt), F_mu relative to itself, the leave-one-out outputs in the
measures of tests/test_gpu_loo.py, lnp relative to max(1, |lnp|).

The tolerance is derived, not fitted: the float64 SciPy evaluation of the device's route (Wi, Wh, M, Vt, Kt^-1 = Wi^T Wi -
Vt^T Vt) measured against the long-double one on these very cases (python tests/marg_fisher_reference.py):

    case                           F      F_mu  pix_mean   pix_var  pix_logp  loo_logp  ep_resid   ep_chi2   ep_logp       lnp
    a-N100-c2-o1-one        2.70e-13  4.26e-14  1.75e-13  3.57e-12  2.98e-12  4.74e-14  1.36e-12  9.30e-13  1.72e-13  3.13e-14
    a-N100-c2-o1-flux       3.15e-13  7.68e-14  1.51e-13  3.46e-12  2.93e-12  9.92e-14  1.26e-12  1.30e-12  2.25e-13  4.60e-14
    b-N128-c1-o0-one        3.42e-14  1.89e-14  1.98e-15  6.78e-14  8.40e-14  2.42e-16  7.92e-15  1.31e-14  4.03e-16  8.46e-18
    b-N128-c1-o0-flux       3.28e-14  5.52e-15  1.88e-15  6.77e-14  6.78e-14  6.83e-16  8.01e-15  1.44e-14  2.36e-16  2.31e-16
    c-N129-c2-o2-one        1.09e-14  1.13e-15  1.60e-14  1.75e-13  4.07e-13  2.64e-15  9.82e-14  4.23e-14  9.35e-15  1.46e-15
    c-N129-c2-o2-flux       9.12e-15  9.44e-15  3.16e-14  2.28e-13  4.02e-13  6.14e-15  1.07e-13  1.84e-14  5.97e-15  2.17e-16
    d-N384-c1-o3-one        9.07e-14  8.55e-14  3.23e-14  7.64e-13  2.61e-12  6.88e-15  2.26e-13  5.42e-14  9.96e-15  2.57e-15
    d-N384-c1-o3-flux       9.26e-14  1.14e-13  3.41e-14  7.72e-13  1.86e-12  1.75e-15  2.04e-13  1.67e-13  2.29e-14  6.97e-16
    e-N300-c3-o1-one        2.04e-14  2.36e-14  5.66e-14  2.53e-13  1.37e-12  1.43e-15  1.94e-13  4.84e-14  5.64e-15  2.65e-16
    e-N300-c3-o1-flux       2.27e-14  1.87e-14  5.19e-14  3.41e-13  9.52e-13  3.91e-15  1.50e-13  4.18e-14  1.02e-14  1.22e-15
    f-N312-c2-o4-one        1.09e-11  1.20e-14  1.87e-12  7.01e-11  3.57e-11  1.20e-13  1.91e-12  2.17e-11  2.01e-12  7.30e-14
    f-N312-c2-o4-flux       1.10e-11  2.30e-14  1.67e-12  6.87e-11  3.02e-11  2.72e-14  1.64e-12  1.90e-11  1.97e-12  3.03e-14
    max                     1.10e-11  1.14e-13  1.87e-12  7.01e-11  3.57e-11  1.20e-13  1.91e-12  2.17e-11  2.01e-12  7.30e-14

(Case f sets most of the last row: a polynomial of degree 4 on 12 pixels per epoch makes M the worst conditioned.)  The
device sums in another order and fuses multiply-adds but is fp64 throughout: it gets the largest measured value of each
output times the project's margin of 8 (marg_fisher_reference.F64_MAX, MARGIN, TOL):

    F 8.80e-11  F_mu 9.12e-13  pix_mean 1.50e-11  pix_var 5.61e-10  pix_logp 2.86e-10  loo_logp 9.60e-13  ep_resid 1.53e-11
    ep_chi2 1.74e-10  ep_logp 1.61e-11  lnp 5.84e-13

On every case the long-double marginal F and pix_mean lie more than 4e9 of these tolerances from their plain-K twins
(tests/test_marg_fisher_reference.py checks more than 100): an implementation that drops the Vt loop cannot pass.
"""
import numpy as np
import pytest

import fisher_reference as fr
import loo_reference as lr
import marg_fisher_reference as mf
import marg_reference as mr

pytestmark = pytest.mark.gpu

TOL = mf.TOL
_LD = np.longdouble
KINDS = [(case, kind) for case in mr.CASES for kind in mr.WEIGHTS]
KIND_IDS = [f"{mr.case_id(case)}-{kind}" for case, kind in KINDS]


def _handle(ch, **kw):
    from psoap_amd.chunk import ChunkHandle
    return ChunkHandle(ch.fl, ch.sigma, **kw)


def _baseline(h, case, kind):
    ch = mr.case_chunk(case)
    h.set_baseline(ch.order, ch.x, ch.epoch_index, ch.n_epochs, mr.prior_sd(ch.order), mr.case_weight(case, kind))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).copy()


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _loo_fields(r):
    return (r.lnp, r.loo_logp, r.pix_mean, r.pix_var, r.pix_logp, r.ep_resid, r.ep_chi2, r.ep_logp)


def _same_loo(a, b):
    return all(_same_bits(x, y) for x, y in zip(_loo_fields(a), _loo_fields(b))) and np.array_equal(a.ep_npix, b.ep_npix)


@pytest.mark.parametrize("case,kind", KINDS, ids=KIND_IDS)
def test_fisher_marg_and_loo_marg_against_long_double(case, kind):
    ch, gp = mr.case_chunk(case), mr.case_gp(case)
    tan_lwl, tan_gp = mf.case_tangents(case)
    ref = mf.case_ext(case, kind)
    with _handle(ch) as h:
        _baseline(h, case, kind)
        F, F_mu = h.fisher_marg(ch.lwls, gp, tan_gp, tan_lwl, want_mu=True)
        loo = h.loo_marg(ch.lwls, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs)
        value = h.lnlike_marg(ch.lwls, gp, mr.MU_GP)
    err = mf.errors((F, F_mu, loo), ref)
    print(f"{mr.case_id(case)}-{kind}: " + ", ".join(f"{k} {v:.2e} ({v / TOL[k]:.2f} of the bound)" for k, v in err.items()))
    assert F.shape == (tan_gp.shape[0],) * 2 and np.all(np.isfinite(F))
    assert _same_bits(F, F.T)
    assert _same_bits(loo.lnp, value)
    assert np.array_equal(loo.ep_npix, ref[2].ep_npix)
    for k, v in err.items():
        assert v <= TOL[k], (k, v, TOL[k])


def test_bits_repeat_and_a_subsequence_of_the_tangents_shares_them():
    case, kind = mr.case_named("f"), "flux"            # Q = 2, three tile rows, T = 7
    ch, gp = mr.case_chunk(case), mr.case_gp(case)
    tan_lwl, tan_gp = mf.case_tangents(case)
    pick = [1, 4, 6]
    with _handle(ch) as h:
        _baseline(h, case, kind)
        seven, mu = h.fisher_marg(ch.lwls, gp, tan_gp, tan_lwl, want_mu=True)
        loo = h.loo_marg(ch.lwls, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs)
        again, mu2 = h.fisher_marg(ch.lwls, gp, tan_gp, tan_lwl, want_mu=True)
        three = h.fisher_marg(ch.lwls, gp, tan_gp[pick], tan_lwl[pick])
        loo2 = h.loo_marg(ch.lwls, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs)
        pixels_only = h.loo_marg(ch.lwls, gp, mr.MU_GP)
    assert _same_bits(seven, again) and _same_bits(mu, mu2) and _same_loo(loo, loo2)
    assert _same_bits(seven, seven.T) and _same_bits(three, three.T)
    assert _same_bits(three, seven[np.ix_(pick, pick)])
    assert len({float(v) for v in seven[np.triu_indices(7)]}) == 28
    # the pixel outputs do not depend on the epoch index of the outputs, which need not be the baseline's
    assert pixels_only.ep_chi2 is None
    assert all(_same_bits(getattr(pixels_only, k), getattr(loo, k)) for k in ("lnp", "loo_logp", "pix_mean", "pix_var", "pix_logp"))


def test_the_plain_and_the_marginal_entries_leave_each_other_as_they_were():
    """h.fisher, h.loo, h.lnlike_marg and h.lnlike_marg_grad before and after the new calls on the same handle: identical
    bits -- the shared workspaces are not left dirty -- and the plain entries differ from the marginal ones"""
    case, kind = mr.case_named("f"), "one"
    ch, gp = mr.case_chunk(case), mr.case_gp(case)
    tan_lwl, tan_gp = mf.case_tangents(case)
    with _handle(ch) as h:
        _baseline(h, case, kind)

        def old():
            return (h.fisher(ch.lwls, gp, tan_gp, tan_lwl, want_mu=True), h.loo(ch.lwls, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs),
                    h.lnlike_marg(ch.lwls, gp, mr.MU_GP), h.lnlike_marg_grad(ch.lwls, gp, mr.MU_GP), h.lnlike(ch.lwls, gp, mr.MU_GP))

        before = old()
        F, F_mu = h.fisher_marg(ch.lwls, gp, tan_gp, tan_lwl, want_mu=True)
        mid = old()
        loo = h.loo_marg(ch.lwls, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs)
        after = old()
        h.fisher_release(), h.loo_release(), h.marg_release(), h.grad_release()
        F2, F_mu2 = h.fisher_marg(ch.lwls, gp, tan_gp, tan_lwl, want_mu=True)       # every workspace comes back, and the bits
        loo2 = h.loo_marg(ch.lwls, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs)
    for got in (mid, after):
        assert _same_bits(got[0][0], before[0][0]) and _same_bits(got[0][1], before[0][1])
        assert _same_loo(got[1], before[1])
        assert _same_bits(got[2], before[2]) and _same_bits(got[4], before[4])
        assert all(_same_bits(a, b) for a, b in zip(got[3], before[3]))
    assert _same_bits(F, F2) and _same_bits(F_mu, F_mu2) and _same_loo(loo, loo2)
    assert fr.rel_to_scale(before[0][0], F) > 100 * TOL["F"]
    assert np.max(np.abs(before[1].pix_mean - loo.pix_mean)) > 100 * TOL["pix_mean"]


def test_conventions_and_refusals():
    from psoap_amd._lib import PsoapError
    from psoap_amd.chunk import ChunkHandle
    case, kind = mr.case_named("a"), "one"
    ch, gp, c = mr.case_chunk(case), mr.case_gp(case), case[2]
    tan_lwl, tan_gp = mf.case_tangents(case)
    T = tan_gp.shape[0]
    with _handle(ch) as h:
        # no baseline: the wrapper and the library both refuse
        with pytest.raises(PsoapError, match="set_baseline"):
            h.fisher_marg(ch.lwls, gp, tan_gp, tan_lwl)
        with pytest.raises(PsoapError, match="set_baseline"):
            h.loo_marg(ch.lwls, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs)
        with pytest.raises(PsoapError, match="psoap_chunk_fisher_marg: call psoap_chunk_set_baseline first"):
            h._fisher("psoap_chunk_fisher_marg", ch.lwls, gp, tan_gp, tan_lwl, False)
        with pytest.raises(PsoapError, match="psoap_chunk_loo_marg: call psoap_chunk_set_baseline first"):
            h._loo("psoap_chunk_loo_marg", ch.lwls, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs)
        _baseline(h, case, kind)
        # a negative hyper-parameter: status 0, NaN and -inf
        neg = gp.copy()
        neg[0] = -neg[0]
        F, mu = h.fisher_marg(ch.lwls, neg, tan_gp, tan_lwl, want_mu=True)
        assert F.shape == (T, T) and np.all(np.isnan(F)) and np.isnan(mu)
        r = h.loo_marg(ch.lwls, neg, mr.MU_GP, ch.epoch_index, ch.n_epochs)
        assert r.lnp == -np.inf and np.isnan(r.loo_logp)
        assert all(np.all(np.isnan(v)) for v in (r.pix_mean, r.pix_var, r.pix_logp, r.ep_resid, r.ep_chi2, r.ep_logp))
        # the number of tangents
        with pytest.raises(PsoapError, match="tangents"):
            h.fisher_marg(ch.lwls, gp, np.zeros((0, 2 * c)))
        with pytest.raises(PsoapError, match="tangents"):
            h.fisher_marg(ch.lwls, gp, np.zeros((33, 2 * c)))
        assert h.fisher_marg(ch.lwls, gp, np.tile(tan_gp[:1], (32, 1))).shape == (32, 32)
        # an epoch whose pixels are not one contiguous run; an index outside [0, n_epochs)
        bad = ch.epoch_index.copy()
        bad[0], bad[-1] = bad[-1], bad[0]
        with pytest.raises(PsoapError, match="psoap_chunk_loo_marg"):
            h.loo_marg(ch.lwls, gp, mr.MU_GP, bad, ch.n_epochs)
        with pytest.raises(PsoapError, match="psoap_chunk_loo_marg"):
            h.loo_marg(ch.lwls, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs - 1)
        # an open stream
        h.stream_open(c, 1)
        try:
            with pytest.raises(PsoapError, match="open stream"):
                h.fisher_marg(ch.lwls, gp, tan_gp, tan_lwl)
            with pytest.raises(PsoapError, match="open stream"):
                h.loo_marg(ch.lwls, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs)
        finally:
            h.stream_close()
        # an epoch index of the outputs that is not the baseline's: two runs instead of four
        two = (ch.epoch_index >= 2).astype(np.int64)
        r2 = h.loo_marg(ch.lwls, gp, mr.MU_GP, two, 2)
        r4 = h.loo_marg(ch.lwls, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs)
        assert np.array_equal(r2.ep_npix, [50, 50]) and _same_bits(r2.pix_mean, r4.pix_mean) and _same_bits(r2.lnp, r4.lnp)
    # not positive definite: zero noise and two identical pixels
    lw = ch.lwls.copy()
    lw[:, 1] = lw[:, 0]
    with ChunkHandle(ch.fl, np.zeros_like(ch.sigma)) as h:
        _baseline(h, case, kind)
        F, mu = h.fisher_marg(lw, gp, tan_gp, tan_lwl, want_mu=True)
        r = h.loo_marg(lw, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs)
    assert np.all(np.isnan(F)) and np.isnan(mu) and r.lnp == -np.inf and np.all(np.isnan(r.pix_mean))


def test_covariance_functions_go_through_the_cached_handle():
    from psoap_amd import covariance
    case, kind = mr.case_named("c"), "flux"
    ch, gp, c = mr.case_chunk(case), mr.case_gp(case), case[2]
    sd = mr.prior_sd(ch.order)
    F_ref, _, loo_ref = mf.case_ext(case, kind)
    try:
        F = covariance.fisher_information_marginal(ch.lwls, ch.fl, ch.sigma, gp, ch.x, ch.epoch_index, ch.order, sd, ch.fl)
        loo = covariance.loo_marginal(ch.lwls, ch.fl, ch.sigma, gp, ch.x, ch.epoch_index, ch.order, sd, ch.fl, mr.MU_GP)
        value = covariance.lnlike_marginal(ch.lwls, ch.fl, ch.sigma, gp, ch.x, ch.epoch_index, ch.order, sd, ch.fl, mr.MU_GP)
        assert len(covariance._handles) == 1
        bad_gp = [-0.2, 5.0, 0.1, 7.0]
        bad = covariance.fisher_information_marginal(ch.lwls, ch.fl, ch.sigma, bad_gp, ch.x, ch.epoch_index, ch.order, sd, ch.fl)
        bad_loo = covariance.loo_marginal(ch.lwls, ch.fl, ch.sigma, bad_gp, ch.x, ch.epoch_index, ch.order, sd, ch.fl)
    finally:
        covariance.release_handles()
    assert F.shape == (2 * c, 2 * c) and np.all(np.isnan(bad)) and bad_loo.lnp == -np.inf
    assert fr.rel_to_scale(F, F_ref[:2 * c, :2 * c]) <= TOL["F"]
    assert _same_bits(loo.lnp, value)
    err = lr.errors(loo, loo_ref)
    assert all(v <= TOL[k] for k, v in err.items()), err


# ---- worker level: the SB2 N = 129 chunk of orbit_grad_reference.CHAIN_CASES[0] -------------------------------------------
def _worker(ch, p_orb, gp, baseline, fix=("gamma",)):
    from psoap_amd.lnprob import ChunkWorker
    from psoap_amd.utils import registered_params
    full = dict(zip(registered_params["SB2"], list(p_orb) + list(gp)))
    w = ChunkWorker("SB2", ch.lwl, ch.fl, ch.sigma, ch.epoch_index, ch.dates, fix_params=list(fix), defaults=full, baseline=baseline)
    return w, np.array([full[n] for n in registered_params["SB2"] if n not in fix])


def test_worker_fisher_is_the_marginal_one_and_differs_from_the_plain_one():
    """ChunkWorker(baseline=...).fisher against the long-double reference on the grids the worker uses (the device's
    velocities, shifted as the device shifts them) with the tangents of the LONG-DOUBLE Jacobian, as tests/test_gpu_fisher.py
    does for the plain case, at the tolerance above; the same worker's plain Fisher information is far from it"""
    import orbit_grad_reference as ogr
    from psoap_amd import lnprob, orbit
    from psoap_amd.utils import registered_params
    case = ogr.CHAIN_CASES[0]
    assert (case.model, case.N) == ("SB2", 129)
    ch, p_orb, gp = case.chunk, case.p_orb, case.gp
    w, p = _worker(ch, p_orb, gp, mf.WORKER_BASELINE)
    try:
        F = w.fisher(p)
        lnp, grad = w.lnprob_grad(p)
        vel = orbit.velocities("SB2", p_orb[None], ch.dates)[0]
        lwls = ch.lwl[None, :] + (-vel[:, ch.epoch_index]) / fr.C_KMS
        n_orb = p_orb.shape[0]
        T = n_orb + 4
        tan_lwl, tan_gp = np.zeros((T, 2, ch.N)), np.zeros((T, 4))
        tan_gp[n_orb:] = np.eye(4)
        from psoap_amd.orbit import velocity_jacobian
        tan_lwl[:n_orb] = -np.moveaxis(velocity_jacobian("SB2", p_orb[None], ch.dates)[1][0], 2, 0)[:, :, ch.epoch_index] / fr.C_KMS
        keep_all = [i for i in range(T) if i >= n_orb or registered_params["SB2"][i] != "gamma"]
        plain = w.handle.fisher(lwls, gp, tan_gp, tan_lwl)[np.ix_(keep_all, keep_all)]
        total = lnprob.fisher_information([w], p)
    finally:
        w.close()
    assert F.shape == (p.shape[0],) * 2 == (grad.shape[0],) * 2 and _same_bits(F, F.T) and _same_bits(total, F)
    keep = [i for i in range(p_orb.shape[0]) if registered_params["SB2"][i] != "gamma"]
    F_ref = mf.worker_fisher_ext(ch, lwls, p_orb, gp, keep)
    err, sep = fr.rel_to_scale(F, F_ref), fr.rel_to_scale(plain, F_ref)
    print(f"SB2-N129 worker Fisher under the baseline: error {err:.2e} (bound {TOL['F']:.2e}); the plain one lies {sep:.2e} away")
    assert err <= TOL["F"]
    assert sep > 100 * TOL["F"]
    # the continuum costs information: Kt^-1 <= K^-1, so no direction is better constrained than under the plain K
    assert np.all(np.diag(F) <= np.diag(plain) * (1 + 1e-9))


def test_loo_outliers_does_not_flag_a_continuum_offset_the_baseline_absorbs():
    from psoap_amd import lnprob
    ch, p_orb, gp, _ = mf.offset_case()
    found = {}
    for name, base in (("marginal", mf.WORKER_BASELINE), ("plain", None)):
        w, p = _worker(ch, p_orb, gp, base)
        try:
            found[name] = lnprob.loo_outliers([w], p, mu_GP=mr.MU_GP)[0]
            if base is not None:
                assert _same_bits(found[name]["loo"].lnp, w.lnprob(p, mr.MU_GP))
        finally:
            w.close()
    print("epoch_sf under the baseline", found["marginal"]["epoch_sf"], "under the plain K", found["plain"]["epoch_sf"])
    assert mf.OFFSET_EPOCH in found["plain"]["epochs"]
    assert found["marginal"]["epochs"].size == 0
    assert lnprob.loo_mask_rows([(5000.0, 5010.0, ch.dates)], [found["marginal"]]) == []
    assert len(lnprob.loo_mask_rows([(5000.0, 5010.0, ch.dates)], [found["plain"]])) >= 1
