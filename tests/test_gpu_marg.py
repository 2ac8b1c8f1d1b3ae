"""GPU tests of the likelihood with a per-epoch continuum polynomial integrated out (psoap_chunk_set_baseline,
psoap_chunk_lnlike_marg; psoap_amd/csrc/marg_kernels.hpp, marg_plan.hpp).

The cases of tests/marg_reference.py -- the smallest shapes at which the appended-column skipping, the Gram tiles or the batch
of M can go wrong -- each with weight = None and weight = fl, against the long-double reference on the dense
K + H Lambda H^T, output by output: lnp and the four parts relative to max(1, |value|); beta and fl_cor absolute; beta_cov
absolute in units of the largest prior variance.

The tolerance is derived, not fitted: the float64 SciPy evaluation of the device's own formulae (marg_reference.marg_f64)
measured against the long-double one on these very cases (python tests/marg_reference.py):

    case                          lnp       quad   logdet_K       gain   logdet_M       beta   beta_cov     fl_cor
    a-N100-c2-o1-one         3.13e-14   1.56e-14   2.52e-16   2.27e-12   9.66e-14   8.60e-13   5.76e-13   1.06e-12
    a-N100-c2-o1-flux        4.60e-14   1.56e-14   2.52e-16   2.70e-12   7.67e-15   8.34e-13   6.88e-13   1.02e-12
    b-N128-c1-o0-one         1.55e-16   1.99e-15   2.14e-16   3.97e-14   7.16e-15   8.94e-16   7.72e-15   8.73e-16
    b-N128-c1-o0-flux        3.93e-16   1.99e-15   2.14e-16   1.87e-14   6.64e-15   1.58e-15   6.23e-15   1.67e-15
    c-N129-c2-o2-one         1.46e-15   3.24e-16   1.06e-16   4.49e-13   1.02e-14   3.78e-14   1.20e-12   1.25e-13
    c-N129-c2-o2-flux        2.17e-16   3.24e-16   1.06e-16   2.82e-14   3.38e-14   1.04e-13   1.21e-12   1.36e-13
    d-N384-c1-o3-one         2.57e-15   9.26e-15   1.61e-15   1.10e-12   1.89e-14   1.93e-13   1.05e-13   2.08e-13
    d-N384-c1-o3-flux        6.97e-16   9.26e-15   1.61e-15   5.23e-14   2.80e-14   1.34e-13   9.07e-14   2.00e-13
    e-N300-c3-o1-one         2.65e-16   1.45e-14   1.45e-15   4.93e-13   7.44e-15   1.13e-13   2.90e-13   1.17e-13
    e-N300-c3-o1-flux        1.22e-15   1.45e-14   1.45e-15   8.46e-14   1.12e-14   6.27e-14   2.65e-13   6.63e-14
    f-N312-c2-o4-one         7.30e-14   3.37e-15   5.85e-16   3.16e-12   2.22e-13   1.24e-12   4.07e-12   3.25e-12
    f-N312-c2-o4-flux        3.03e-14   3.37e-15   5.85e-16   1.51e-12   1.82e-13   1.18e-12   4.07e-12   3.24e-12
    max                      7.30e-14   1.56e-14   1.61e-15   3.16e-12   2.22e-13   1.24e-12   4.07e-12   3.25e-12

(The abscissa map u = off + scl x cancels five digits -- off and scl x are ~ 7e4 for a 25-pixel epoch -- which is what the
columns of 1e-12 are made of: numpy.polynomial.Chebyshev's own semantics.)  The device sums in another order and fuses
multiply-adds but is fp64 throughout: it gets the largest measured value of each output times the project's margin of 8
(tests/test_gpu_grad.py).  Nothing is fitted to the device's own results.

ChunkWorker(baseline=...) is compared with the reference on the grids of the LONG-DOUBLE orbit, while the worker shifts its
grid in float64; the margin there is measured the same way (tests/test_gpu_loo.py explains why it is another one): marg_f64
on the float64 grids against marg_ext on the long-double grids, on the SB2 chunk of that test:

    SB2-N240 orbit grids     3.47e-12   5.15e-12   3.50e-13   4.17e-12   3.89e-13   2.47e-12   2.78e-12   2.87e-12

again times 8.
"""
import ctypes

import numpy as np
import pytest

import marg_reference as mr
from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu

MARGIN = 8
F64 = {"lnp": 7.30e-14, "quad": 1.56e-14, "logdet_K": 1.61e-15, "gain": 3.16e-12, "logdet_M": 2.22e-13, "beta": 1.24e-12,
       "beta_cov": 4.07e-12, "fl_cor": 3.25e-12}          # the table above, last row
TOL = {k: MARGIN * v for k, v in F64.items()}
F64_ORBIT = {"lnp": 3.47e-12, "quad": 5.15e-12, "logdet_K": 3.50e-13, "gain": 4.17e-12, "logdet_M": 3.89e-13, "beta": 2.47e-12,
             "beta_cov": 2.78e-12, "fl_cor": 2.87e-12}    # the SB2 row above
TOL_ORBIT = {k: MARGIN * v for k, v in F64_ORBIT.items()}
FIELDS = ("lnp", "parts", "beta", "beta_cov", "fl_cor")
ALL = dict(want_beta=True, want_cov=True, want_flux=True)


def _handle(ch, **kw):
    from psoap_amd.chunk import ChunkHandle
    return ChunkHandle(ch.fl, ch.sigma, **kw)


def _baseline(h, case, kind, sd=None):
    ch = mr.case_chunk(case)
    h.set_baseline(ch.order, ch.x, ch.epoch_index, ch.n_epochs, mr.prior_sd(ch.order) if sd is None else sd,
                   mr.case_weight(case, kind))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_result(a, b, fields=FIELDS):
    return all(_same_bits(getattr(a, f), getattr(b, f)) for f in fields)


def _check(name, got, ref, sd, tol=TOL):
    err = mr.errors(got, ref, np.asarray(sd))
    print(f"{name}: " + ", ".join(f"{k} {v:.2e} ({tol[k]:.2e})" for k, v in err.items()))
    for k, v in err.items():
        assert v <= tol[k], (name, k, v, tol[k])


@pytest.mark.parametrize("kind", mr.WEIGHTS)
@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_id)
def test_marg_against_long_double(case, kind):
    ch, gp = mr.case_chunk(case), mr.case_gp(case)
    with _handle(ch) as h:
        _baseline(h, case, kind)
        got = h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL)
        value = h.lnlike_marg(ch.lwls, gp, mr.MU_GP)
    assert got.beta.shape == (ch.n_epochs, ch.order + 1) and got.fl_cor.shape == ch.fl.shape
    assert _same_bits(np.float64(value), np.float64(got.lnp))
    assert _same_bits(got.beta_cov, got.beta_cov.T)
    _check(f"{mr.case_id(case)}-{kind}", got, mr.case_ext(case, kind), mr.prior_sd(ch.order))


def test_empty_epoch_has_the_prior_and_adds_nothing():
    """case e, epoch 1: mean 0 and covariance Lambda exactly.  Against the same chunk without that epoch's columns the other
    columns sit elsewhere in M's tile (another elimination and summation order): the same numbers within twice the derived
    tolerances, not the same bits."""
    case = mr.case_named("e")
    ch, gp, sd = mr.case_chunk(case), mr.case_gp(case), mr.prior_sd(1)
    ep = np.asarray(ch.epoch_index).copy()
    ep[ep > 1] -= 1
    with _handle(ch) as h:
        _baseline(h, case, "one")
        full = h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL)
        h.set_baseline(ch.order, ch.x, ep, ch.n_epochs - 1, sd)
        less = h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL)
    assert np.all(full.beta[1] == 0.0)
    assert np.array_equal(full.beta_cov[2:4, 2:4], np.diag(sd * sd))
    assert not np.any(full.beta_cov[2:4, :2]) and not np.any(full.beta_cov[2:4, 4:])
    assert abs(full.lnp - less.lnp) <= 2 * TOL["lnp"] * max(1.0, abs(full.lnp))
    assert np.max(np.abs(full.fl_cor - less.fl_cor)) <= 2 * TOL["fl_cor"]
    assert np.max(np.abs(np.delete(full.beta, 1, axis=0) - less.beta)) <= 2 * TOL["beta"]


def test_bit_identity_across_calls_batches_and_optional_outputs():
    case = mr.case_named("f")
    ch, c = mr.case_chunk(case), case[2]
    gps = syn.make_walkers(c, 3, seed=9701)
    gps[0] = mr.case_gp(case)
    lw = np.stack([ch.lwls, ch.lwls + 1e-6, ch.lwls - 2e-6])
    with _handle(ch, max_batch=3) as h:
        _baseline(h, case, "flux")
        a = h.lnlike_marg(lw, gps, mr.MU_GP, **ALL)
        b = h.lnlike_marg(lw, gps, mr.MU_GP, **ALL)
        assert _same_result(a, b)
        for k in range(3):
            one = h.lnlike_marg(lw[k], gps[k], mr.MU_GP, **ALL)
            assert all(_same_bits(getattr(one, f), getattr(a, f)[k]) for f in FIELDS), k
        assert _same_bits(h.lnlike_marg(lw, gps, mr.MU_GP), a.lnp)
        only_beta = h.lnlike_marg(lw, gps, mr.MU_GP, want_beta=True)
        assert _same_result(only_beta, a, ("lnp", "parts", "beta")) and only_beta.beta_cov is None and only_beta.fl_cor is None
        only_cov = h.lnlike_marg(lw, gps, mr.MU_GP, want_cov=True)
        assert _same_result(only_cov, a, ("lnp", "parts", "beta_cov"))
        only_flux = h.lnlike_marg(lw, gps, mr.MU_GP, want_flux=True)
        assert _same_result(only_flux, a, ("lnp", "parts", "fl_cor"))


@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_id)
def test_vanishing_prior_is_the_plain_likelihood(case):
    ch, gp = mr.case_chunk(case), mr.case_gp(case)
    with _handle(ch) as h:
        plain = h.lnlike(ch.lwls, gp, mr.MU_GP)
        for kind in mr.WEIGHTS:
            _baseline(h, case, kind, np.full(ch.order + 1, 1e-12))
            got = h.lnlike_marg(ch.lwls, gp, mr.MU_GP)
            print(mr.case_id(case), kind, got - plain)
            assert abs(got - plain) <= 1e-10 * max(1.0, abs(plain)), kind


def test_raw_abi_null_outputs():
    from psoap_amd import _lib
    case = mr.case_named("c")
    ch, gp, c = mr.case_chunk(case), mr.case_gp(case), case[2]
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))      # noqa: E731
    with _handle(ch) as h:
        _baseline(h, case, "one")
        want = h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL)
        lw, lnp, parts = np.ascontiguousarray(ch.lwls), np.empty(1), np.empty(4)
        assert h._L.psoap_chunk_lnlike_marg(h._h, 1, c, dp(lw), dp(gp), mr.MU_GP, dp(lnp), None, None, None, None) == 0
        assert lnp[0] == want.lnp
        assert h._L.psoap_chunk_lnlike_marg(h._h, 1, c, dp(lw), dp(gp), mr.MU_GP, dp(lnp), dp(parts), None, None, None) == 0
        assert _same_bits(parts, want.parts)
        assert h._L.psoap_chunk_lnlike_marg(h._h, 1, c, dp(lw), dp(gp), mr.MU_GP, None, None, None, None, None) != 0
        assert _lib.load().psoap_last_error()


def test_conventions_and_refusals():
    from psoap_amd._lib import PsoapError, load
    from psoap_amd.chunk import ChunkHandle
    case = mr.case_named("a")
    ch, gp, c = mr.case_chunk(case), mr.case_gp(case), case[2]
    sd = mr.prior_sd(ch.order)
    last = lambda: load().psoap_last_error()      # noqa: E731

    def refused(match, fn, *a, **kw):
        with pytest.raises(PsoapError, match=match):
            fn(*a, **kw)
        assert last()

    with _handle(ch, max_batch=2) as h:
        # before a baseline (the Python layer refuses first; the library itself through the raw entry)
        with pytest.raises(PsoapError, match="set_baseline"):
            h.lnlike_marg(ch.lwls, gp, mr.MU_GP)
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))      # noqa: E731
        lw, lnp = np.ascontiguousarray(ch.lwls), np.empty(1)
        assert h._L.psoap_chunk_lnlike_marg(h._h, 1, c, dp(lw), dp(gp), mr.MU_GP, dp(lnp), None, None, None, None) != 0
        assert b"set_baseline" in last()
        x, ep, ne = ch.x, ch.epoch_index, ch.n_epochs
        refused("order", h.set_baseline, -1, x, ep, ne, [])
        i32 = ctypes.POINTER(ctypes.c_int32)
        ep32 = np.ascontiguousarray(ep, dtype=np.int32)
        assert h._L.psoap_chunk_set_baseline(h._h, -1, dp(x), ep32.ctypes.data_as(i32), ne, None, dp(sd)) != 0 and b"order" in last()
        refused("order", h.set_baseline, 16, x, ep, ne, np.ones(17))
        refused("1024", h.set_baseline, 15, x, ep, 65, np.ones(16))
        for bad in ([0.05, 0.0], [0.05, -1.0], [np.nan, 0.1], [0.05, np.inf]):
            refused("prior_sd", h.set_baseline, 1, x, ep, ne, bad)
        split = np.asarray(ep).copy()
        split[-1] = split[0]
        refused("not contiguous", h.set_baseline, 1, x, split, ne, sd)
        refused("out of range", h.set_baseline, 1, x, ep, 2, sd)
        # (a refused baseline leaves none behind)
        with pytest.raises(PsoapError, match="set_baseline"):
            h.lnlike_marg(ch.lwls, gp, mr.MU_GP)
        _baseline(h, case, "one")
        good = h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL)
        refused("max_batch", h.lnlike_marg, np.stack([ch.lwls] * 3), np.stack([gp] * 3), mr.MU_GP)
        h.stream_open(c, 1)
        try:
            refused("open stream", h.lnlike_marg, ch.lwls, gp, mr.MU_GP)
            refused("open stream", h.set_baseline, 1, x, ep, ne, sd)
        finally:
            h.stream_close()
        # negative hyper-parameters: status 0, -inf and NaN
        for k in (0, 1):
            neg = gp.copy()
            neg[k] = -neg[k]
            bad = h.lnlike_marg(np.stack([ch.lwls, ch.lwls]), np.stack([gp, neg]), mr.MU_GP, **ALL)
            assert bad.lnp[1] == -np.inf and all(np.all(np.isnan(getattr(bad, f)[1])) for f in FIELDS[1:])
            assert all(_same_bits(getattr(bad, f)[0], getattr(good, f)) for f in FIELDS)
    # not positive definite: zero noise and two identical pixels (the degenerate input of tests/test_gpu_loo.py)
    lw = ch.lwls.copy()
    lw[:, 1] = lw[:, 0]
    with ChunkHandle(ch.fl, np.zeros_like(ch.sigma)) as h:
        _baseline(h, case, "one")
        bad = h.lnlike_marg(lw, gp, mr.MU_GP, **ALL)
    assert bad.lnp == -np.inf and all(np.all(np.isnan(getattr(bad, f))) for f in FIELDS[1:])
    assert bad.beta_cov.shape == (8, 8) and bad.fl_cor.shape == ch.fl.shape


def test_lifecycle_release_set_data_and_the_handle_is_left_as_it_was():
    from psoap_amd._lib import PsoapError
    case = mr.case_named("f")
    ch, gp, c = mr.case_chunk(case), mr.case_gp(case), case[2]
    wc = syn.make_chunk(2, 3, 104, seed=9710)
    gps = syn.make_walkers(2, 4, seed=9711)
    lw = syn.walker_lwls(wc, syn.make_walker_velocities(wc, 4, seed=9712))
    with _handle(ch, max_batch=4) as h:
        _baseline(h, case, "one")
        good = h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL)
        before = h.lnlike_batch(lw, gps, 0.9)
        grad = h.lnlike_grad(ch.lwls, gp, mr.MU_GP)
        loo = h.loo(ch.lwls, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs)
        # an uploaded batch, a marginal call in between: the pending batch and everything else keep their bits
        h.upload(lw[::-1].copy(), gps[::-1].copy(), 0.9)
        assert _same_result(h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL), good)
        h.eval()
        assert _same_bits(h.fetch(), before[::-1]) and _same_bits(h.lnlike_batch(lw, gps, 0.9), before)
        again = h.lnlike_grad(ch.lwls, gp, mr.MU_GP)
        assert all(_same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(grad, again))
        loo2 = h.loo(ch.lwls, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs)
        assert _same_bits(loo.pix_mean, loo2.pix_mean) and _same_bits(loo.ep_chi2, loo2.ep_chi2) and loo.lnp == loo2.lnp
        # releases: the marginal workspace (twice), the shared gradient workspace, both
        h.marg_release()
        h.marg_release()
        assert _same_result(h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL), good)
        h.grad_release()
        assert _same_result(h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL), good)
        h.marg_release()
        h.grad_release()
        assert _same_result(h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL), good)
        # set_data: an unweighted baseline stays, and sees the new data
        h.set_data(ch.fl + 0.01, ch.sigma)
        moved = h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL)
        assert _same_bits(moved.beta_cov, good.beta_cov) and not _same_bits(moved.beta, good.beta)
        assert np.max(np.abs(moved.fl_cor - 0.01 - good.fl_cor)) < 0.01
        h.set_data(ch.fl, ch.sigma)
        assert _same_result(h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL), good)
        # a weighted one described the old data: refused until it is set again
        _baseline(h, case, "flux")
        flux = h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL)
        assert not _same_bits(flux.beta, good.beta)
        h.set_data(ch.fl, ch.sigma)
        with pytest.raises(PsoapError, match="set_baseline again"):
            h.lnlike_marg(ch.lwls, gp, mr.MU_GP)
        _baseline(h, case, "flux")
        assert _same_result(h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL), flux)
        # another baseline on the same handle (Q = 2 -> Q = 1) and back
        h.set_baseline(0, ch.x, ch.epoch_index, ch.n_epochs, [0.05])
        assert h.lnlike_marg(ch.lwls, gp, mr.MU_GP, want_beta=True).beta.shape == (26, 1)
        _baseline(h, case, "one")
        assert _same_result(h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL), good)


def test_covariance_functions_go_through_the_cached_handle():
    from psoap_amd import covariance
    case = mr.case_named("c")
    ch, gp = mr.case_chunk(case), mr.case_gp(case)
    sd = mr.prior_sd(ch.order)
    try:
        lnp = covariance.lnlike_marginal(ch.lwls, ch.fl, ch.sigma, gp, ch.x, ch.epoch_index, ch.order, sd, ch.fl, mr.MU_GP)
        beta, cov, flc, lnp2 = covariance.baseline_posterior(ch.lwls, ch.fl, ch.sigma, gp, ch.x, ch.epoch_index, ch.order, sd,
                                                             ch.fl, mr.MU_GP)
        assert len(covariance._handles) == 1
        neg = covariance.lnlike_marginal(ch.lwls, ch.fl, ch.sigma, -gp, ch.x, ch.epoch_index, ch.order, sd)
        nb, nc, nf, nl = covariance.baseline_posterior(ch.lwls, ch.fl, ch.sigma, -gp, ch.x, ch.epoch_index, ch.order, sd)
    finally:
        covariance.release_handles()
    assert isinstance(lnp, float) and lnp == lnp2 and neg == -np.inf and nl == -np.inf
    assert np.all(np.isnan(nb)) and nb.shape == beta.shape and np.all(np.isnan(nc)) and np.all(np.isnan(nf))
    ref = mr.case_ext(case, "flux")
    got = mr.Marg(lnp2, np.asarray(ref.parts, dtype=np.float64), beta, cov, flc)          # (the parts are not returned here)
    _check("covariance c-flux", got, ref, sd)


# ---- lnprob(p): grids from the orbit -------------------------------------------------------------------------------------
def _orbit_worker(baseline, fix=(), max_batch=1):
    from psoap_amd.lnprob import ChunkWorker
    from psoap_amd.utils import registered_params
    ch, p_orb, gp, lwls_ext, _ = mr.orbit_case()
    full = dict(zip(registered_params["SB2"], list(p_orb) + list(gp)))
    w = ChunkWorker("SB2", ch.lwl, ch.fl, ch.sigma, ch.epoch_index, ch.dates, fix_params=list(fix), defaults=full,
                    max_batch=max_batch, baseline=baseline)
    p = np.array([full[n] for n in registered_params["SB2"] if n not in fix])
    return ch, w, p, p_orb, gp, lwls_ext


def test_worker_with_a_baseline():
    from psoap_amd import covariance, lnprob
    from psoap_amd._lib import PsoapError
    base = {"order": 1, "sd": list(mr.PLANT_SD), "weight": "one"}
    ch, w, p, p_orb, gp, lwls_ext = _orbit_worker(base, fix=("gamma",), max_batch=2)
    try:
        P = np.stack([p, p * (1 + 1e-3), p * (1 - 1e-3)])
        got = w.lnprob_batch(P, mr.MU_GP)          # (three proposals through max_batch = 2: two pieces)
        assert w.lnprob(p, mr.MU_GP) == got[0]
        grids, fast = w.shifted_grids(np.stack([p_orb]))
        fit = lnprob.baseline_fit([w], p, mr.MU_GP)[0]
        for what in (w.upload_proposals, w.stream_submit):
            with pytest.raises(PsoapError, match="baseline"):
                what(P)
        with pytest.raises(PsoapError, match="baseline"):
            w.stream_open()
    finally:
        w.close()
    assert not fast[0]
    try:
        direct = covariance.lnlike_marginal(grids[0], ch.fl, ch.sigma, gp, ch.lwl, ch.epoch_index, 1, mr.PLANT_SD, None, mr.MU_GP)
    finally:
        covariance.release_handles()
    assert _same_bits(np.float64(direct), np.float64(got[0])) and fit["lnp"] == got[0]
    ref = mr.marg_ext(lwls_ext, ch.fl, ch.sigma, gp, ch.lwl, ch.epoch_index, mr.PLANT_EPOCHS, 1, mr.PLANT_SD, None, mr.MU_GP)
    res = mr.Marg(fit["lnp"], np.asarray(ref.parts, dtype=np.float64), fit["beta"], fit["beta_cov"], fit["fl_cor"])
    _check("SB2 worker", res, ref, mr.PLANT_SD, TOL_ORBIT)
    assert np.allclose(fit["beta_sd"], np.sqrt(np.diag(fit["beta_cov"])).reshape(6, 2))


def test_worker_without_a_baseline_is_as_before_and_says_so():
    from psoap_amd._lib import PsoapError
    ch, w, p, p_orb, gp, _ = _orbit_worker(None)
    try:
        assert w.baseline is None and np.isfinite(w.lnprob(p, mr.MU_GP))
        with pytest.raises(PsoapError, match="no baseline"):
            w.marg_orbits(p_orb, gp)
    finally:
        w.close()


def test_planted_tilt_is_recovered_on_the_device(tmp_path):
    from psoap_amd import data, lnprob
    ch, gp, beta = mr.planted()
    with _handle(ch) as h:
        h.set_baseline(1, ch.x, ch.epoch_index, ch.n_epochs, mr.PLANT_SD)
        got = h.lnlike_marg(ch.lwls, gp, mr.MU_GP, **ALL)
        plain = h.lnlike(ch.lwls, gp, mr.MU_GP)
    print(np.abs(got.beta - beta) / got.beta_sd)
    assert np.all(np.abs(got.beta - beta) < 4.0 * got.beta_sd)
    assert got.lnp > plain
    # the corrected fluxes back into a chunk file, through data.Chunk.save
    shape = (mr.PLANT_EPOCHS, mr.PLANT_PIX)
    two_d = data.Chunk(np.exp(ch.x).reshape(shape), ch.fl.reshape(shape), ch.sigma.reshape(shape),
                       np.repeat(np.arange(6.0), mr.PLANT_PIX).reshape(shape))
    fit = {"fl_cor": got.fl_cor}
    name, = lnprob.write_corrected_chunks([(22, 5000, 5010)], [two_d], [fit], prefix=str(tmp_path) + "/")
    back = data.Chunk.open(22, 5000, 5010, prefix=str(tmp_path) + "/")
    assert name.endswith(".npz") and _same_bits(back.fl.reshape(-1), got.fl_cor)
