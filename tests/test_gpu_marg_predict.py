"""GPU tests of the component spectra under the marginalised continuum (psoap_chunk_predict_marg, _predict_marg_var;
psoap_amd/csrc/marg_predict_kernels.hpp, marg_predict_plan.hpp).

The cases of tests/marg_predict_reference.py -- the smallest shapes at which a tile edge of each of the three column blocks
of [K | Cx^T | Ht] can go wrong -- each with weight = None and weight = fl, against the long-double reference on the dense
K + H Lambda H^T, output by output: mu absolute; Sigma and the variances absolute in units of the largest prior variance.

The tolerance is derived, not fitted: the float64 SciPy evaluation of the device's own formulae
(marg_predict_reference.marg_predict_f64) measured against the long-double one on these very cases
(python tests/marg_predict_reference.py):

    case                                     mu      Sigma        var
    a-N100-c2-o1-mode0-M50-one         6.05e-13   1.06e-13   1.06e-13
    a-N100-c2-o1-mode0-M50-flux        5.73e-13   9.34e-14   9.36e-14
    a-N100-c2-o1-mode1-M130-one        1.18e-12   2.25e-13   2.25e-13
    a-N100-c2-o1-mode1-M130-flux       1.10e-12   1.95e-13   1.95e-13
    b-N128-c1-o0-mode2-M128-one        4.23e-15   2.31e-15   1.31e-15
    b-N128-c1-o0-mode2-M128-flux       4.60e-15   2.21e-15   1.15e-15
    c-N129-c2-o2-mode0-M65-one         5.95e-14   2.93e-13   2.93e-13
    c-N129-c2-o2-mode0-M65-flux        1.11e-13   2.80e-13   2.79e-13
    d-N384-c1-o3-mode2-M129-one        2.03e-13   6.17e-14   6.14e-14
    d-N384-c1-o3-mode2-M129-flux       1.99e-13   6.34e-14   6.32e-14
    e-N300-c3-o1-mode0-M43-one         1.32e-13   3.45e-14   3.49e-14
    e-N300-c3-o1-mode0-M43-flux        1.22e-13   2.78e-14   2.81e-14
    f-N312-c2-o4-mode0-M100-one        2.92e-12   1.89e-12   1.89e-12
    f-N312-c2-o4-mode0-M100-flux       2.98e-12   1.60e-12   1.60e-12
    max                                2.98e-12   1.89e-12   1.89e-12

The device sums in another order and fuses multiply-adds but is fp64 throughout: it gets the largest measured value of each
output times the project's margin of 8 (tests/test_gpu_grad.py).  Nothing is fitted to the device's own results.
"""
import ctypes
import functools

import numpy as np
import pytest

import marg_predict_reference as mp
import marg_reference as mr
from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu

MARGIN = 8
F64 = {"mu": 2.98e-12, "Sigma": 1.89e-12, "var": 1.89e-12}          # the table above, last row
TOL = {k: MARGIN * v for k, v in F64.items()}


def _handle(ch, **kw):
    from psoap_amd.chunk import ChunkHandle
    return ChunkHandle(ch.fl, ch.sigma, **kw)


def _baseline(h, case, kind):
    ch = mr.case_chunk(case)
    h.set_baseline(ch.order, ch.x, ch.epoch_index, ch.n_epochs, mr.prior_sd(ch.order), mr.case_weight(case, kind))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _call(pc):
    """-> (mode, lwls, pred, mus, gp) of a case: what ``predict`` and ``predict_marg`` take"""
    case = mr.case_named(pc[0])
    return pc[1], mr.case_chunk(case).lwls, mp.pcase_pred(pc), mp.pcase_mus(pc), mr.case_gp(case)


@functools.lru_cache(maxsize=None)
def device(pc, kind):
    """every form of one case, once per session: -> dict(full=(mu, Sigma), mean=mu, diag=(mu, var), plain_diag=(mu, var))"""
    case = mr.case_named(pc[0])
    args = _call(pc)
    with _handle(mr.case_chunk(case)) as h:
        _baseline(h, case, kind)
        return {"full": h.predict_marg(*args), "mean": h.predict_marg(*args, want_sigma=False),
                "diag": h.predict_marg(*args, want_sigma="diag"), "plain_diag": h.predict(*args, want_sigma="diag")}


def _check(name, err, factor=1):
    print(f"{name}: " + ", ".join(f"{k} {v:.2e} ({factor * TOL[k]:.2e})" for k, v in err.items()))
    for k, v in err.items():
        assert v <= factor * TOL[k], (name, k, v, factor * TOL[k])


# ---- parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", mp.WEIGHTS)
@pytest.mark.parametrize("pc", mp.PCASES, ids=mp.pcase_id)
def test_predict_marg_against_long_double(pc, kind):
    got, ref = device(pc, kind), mp.pcase_ext(pc, kind)
    mu, Sigma = got["full"]
    R = ref.mu.shape[0]
    assert mu.shape == (R,) and Sigma.shape == (R, R) and got["diag"][1].shape == (R,)
    _check(f"{mp.pcase_id(pc)}-{kind}", mp.errors(mu, Sigma, got["diag"][1], ref))


# ---- forms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", mp.WEIGHTS)
@pytest.mark.parametrize("pc", mp.PCASES, ids=mp.pcase_id)
def test_the_three_forms_agree_and_the_covariance_only_grows(pc, kind):
    got, ref = device(pc, kind), mp.pcase_ext(pc, kind)
    (mu, Sigma), (mu_d, var) = got["full"], got["diag"]
    assert _same_bits(mu, got["mean"]) and _same_bits(mu, mu_d)
    assert _same_bits(Sigma, Sigma.T)
    unit = float(ref.prior_max)
    assert np.max(np.abs(var - np.diag(Sigma))) <= TOL["var"] * unit
    assert np.all(var >= got["plain_diag"][1] - TOL["var"] * unit)


# ---- determinism and non-interference ---------------------------------------------------------------------------------------
def test_bit_identity_across_calls_and_the_plain_entries_keep_their_bits():
    pc = mp.PCASES[6]               # f: Q = 2, R = 200
    case, args = mr.case_named(pc[0]), _call(pc)
    ch, gp = mr.case_chunk(case), mr.case_gp(case)
    with _handle(ch) as h:
        plain0 = h.predict(*args)
        _baseline(h, case, "flux")
        plain1 = h.predict(*args)
        lnp0 = h.lnlike_marg(ch.lwls, gp, mr.MU_GP, want_beta=True, want_flux=True)
        a = h.predict_marg(*args)
        b = h.predict_marg(*args)
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
        assert _same_bits(a[0], device(pc, "flux")["full"][0]) and _same_bits(a[1], device(pc, "flux")["full"][1])
        plain2 = h.predict(*args)
        for p in (plain1, plain2):
            assert _same_bits(p[0], plain0[0]) and _same_bits(p[1], plain0[1])
        lnp1 = h.lnlike_marg(ch.lwls, gp, mr.MU_GP, want_beta=True, want_flux=True)
        assert lnp0.lnp == lnp1.lnp and _same_bits(lnp0.parts, lnp1.parts) and _same_bits(lnp0.beta, lnp1.beta)
        assert _same_bits(lnp0.fl_cor, lnp1.fl_cor)
        d0 = h.predict_marg(*args, want_sigma="diag")
        h.marg_release()
        c1 = h.predict_marg(*args)
        h.predict_release()
        c2 = h.predict_marg(*args)
        h.marg_release()
        h.predict_release()
        d1 = h.predict_marg(*args, want_sigma="diag")
        for c in (c1, c2):
            assert _same_bits(c[0], a[0]) and _same_bits(c[1], a[1])
        assert _same_bits(d0[0], d1[0]) and _same_bits(d0[1], d1[1])
        t = h.predict_timings()
        assert t["flops"] > 0 and t["device_ms"] > 0


# ---- empty epoch ------------------------------------------------------------------------------------------------------------
def test_an_empty_epoch_changes_nothing():
    """case e, epoch 1 has no pixel: its columns of H are zero.  Against the same chunk without that epoch's columns the other
    columns sit elsewhere in M's tile (another elimination and summation order): the same numbers within twice the derived
    tolerances, not the same bits -- the convention of test_gpu_marg.test_empty_epoch_has_the_prior_and_adds_nothing."""
    pc = mp.PCASES[5]
    assert pc[0] == "e"
    case, args = mr.case_named("e"), _call(pc)
    ch = mr.case_chunk(case)
    ep = np.asarray(ch.epoch_index).copy()
    ep[ep > 1] -= 1
    full, full_d = device(pc, "one")["full"], device(pc, "one")["diag"]
    with _handle(ch) as h:
        h.set_baseline(ch.order, ch.x, ep, ch.n_epochs - 1, mr.prior_sd(ch.order))
        less = h.predict_marg(*args)
        less_d = h.predict_marg(*args, want_sigma="diag")
    unit = float(mp.pcase_ext(pc, "one").prior_max)
    assert np.max(np.abs(full[0] - less[0])) <= 2 * TOL["mu"]
    assert np.max(np.abs(full[1] - less[1])) <= 2 * TOL["Sigma"] * unit
    assert np.max(np.abs(full_d[1] - less_d[1])) <= 2 * TOL["var"] * unit
    _check("e without the empty epoch", mp.errors(less[0], less[1], less_d[1], mp.pcase_ext(pc, "one")))


# ---- conventions --------------------------------------------------------------------------------------------------------------
def test_refusals():
    from psoap_amd._lib import PsoapError
    pc = mp.PCASES[0]
    case, args = mr.case_named("a"), _call(pc)
    ch = mr.case_chunk(case)
    with _handle(ch) as h:
        with pytest.raises(PsoapError, match="call psoap_chunk_set_baseline first"):
            h.predict_marg(*args)
        with pytest.raises(PsoapError, match="call psoap_chunk_set_baseline first"):
            h.predict_marg(*args, want_sigma="diag")
        _baseline(h, case, "flux")
        good = h.predict_marg(*args)
        h.set_data(ch.fl, ch.sigma)
        with pytest.raises(PsoapError, match="psoap_chunk_set_data changed the data the baseline's weights were given for"):
            h.predict_marg(*args)
        _baseline(h, case, "flux")
        again = h.predict_marg(*args)
        assert _same_bits(good[0], again[0]) and _same_bits(good[1], again[1])
        with pytest.raises(PsoapError, match="mode 2"):
            h.predict_marg(2, *args[1:])
        with pytest.raises(PsoapError, match="mode 1"):
            h.predict_marg(1, ch.lwls[:1], args[2][:1], args[3][:1], args[4][:2])
        h.stream_open(2, 1)
        try:
            with pytest.raises(PsoapError, match="open stream"):
                h.predict_marg(*args)
        finally:
            h.stream_close()
    case3 = mr.case_named("e")
    ch3 = mr.case_chunk(case3)
    with _handle(ch3) as h:
        _baseline(h, case3, "one")
        with pytest.raises(PsoapError, match="three components"):
            h.predict_marg(1, ch3.lwls, np.tile(ch3.lwls[0], (3, 1)), [mr.MU_GP], mr.case_gp(case3))


def test_a_data_covariance_that_is_not_positive_definite_raises_and_the_handle_stays_usable():
    """zero noise and two identical pixels (the degenerate input of the plain predict and of tests/test_gpu_marg.py): status 1
    and NaN through the raw ABI, LinAlgError from every form of the wrapper; with the noise back the handle gives the bits
    of a fresh one."""
    from psoap_amd import _lib
    pc = mp.PCASES[0]
    case, (mode, lwls, pred, mus, gp) = mr.case_named("a"), _call(pc)
    ch = mr.case_chunk(case)
    lw = lwls.copy()
    lw[:, 1] = lw[:, 0]
    R = 2 * pc[2]
    with _handle(ch) as h:
        h.set_data(ch.fl, np.zeros_like(ch.sigma))
        _baseline(h, case, "one")
        for want in (True, False, "diag"):
            with pytest.raises(np.linalg.LinAlgError):
                h.predict_marg(mode, lw, pred, mus, gp, want_sigma=want)
        mu, Sigma, var, status = np.zeros(R), np.zeros((R, R)), np.zeros(R), ctypes.c_int(-1)
        a = [_lib.as_f64(v) for v in (lw, pred, mus, gp)]
        rc = _lib.load().psoap_chunk_predict_marg(h._h, mode, 2, pc[2], *[_lib.dptr(v) for v in a], _lib.dptr(mu), _lib.dptr(Sigma),
                                                  ctypes.byref(status))
        assert (rc, status.value) == (0, 1) and np.all(np.isnan(mu)) and np.all(np.isnan(Sigma))
        status = ctypes.c_int(-1)
        rc = _lib.load().psoap_chunk_predict_marg_var(h._h, mode, 2, pc[2], *[_lib.dptr(v) for v in a], _lib.dptr(mu),
                                                      _lib.dptr(var), ctypes.byref(status))
        assert (rc, status.value) == (0, 1) and np.all(np.isnan(mu)) and np.all(np.isnan(var))
        h.set_data(ch.fl, ch.sigma)
        after = h.predict_marg(mode, lwls, pred, mus, gp)
    fresh = device(pc, "one")["full"]
    assert _same_bits(after[0], fresh[0]) and _same_bits(after[1], fresh[1])


# ---- plumbing -----------------------------------------------------------------------------------------------------------------
def test_predict_marginal_is_the_handle_call():
    from psoap_amd import covariance as cov
    pc = mp.PCASES[3]
    case = mr.case_named(pc[0])
    ch = mr.case_chunk(case)
    mode, lwls, pred, mus, gp = _call(pc)
    try:
        for kind in mp.WEIGHTS:
            for want, key in ((True, "full"), ("diag", "diag")):
                got = cov.predict_marginal(lwls, ch.fl, ch.sigma, pred, mus, gp, ch.x, ch.epoch_index, ch.order, mr.prior_sd(ch.order),
                                           mr.case_weight(case, kind), mode=mode, want_sigma=want)
                ref = device(pc, kind)[key]
                assert _same_bits(got[0], ref[0]) and _same_bits(got[1], ref[1])
        mean = cov.predict_marginal(lwls, ch.fl, ch.sigma, pred, mus, gp, ch.x, ch.epoch_index, ch.order, mr.prior_sd(ch.order),
                                    mode=mode, want_sigma=False)
        assert _same_bits(mean, device(pc, "one")["mean"])
    finally:
        cov.release_handles()


def _chunk2d(s):
    from psoap_amd import data as pdata

    def full(v, fill):
        out = np.full(s.mask.shape, fill)
        out[s.mask] = v
        return out
    date = np.broadcast_to(s.dates[:, None], s.mask.shape).copy()
    return pdata.Chunk(np.exp(full(s.lwl, 8.5)), full(s.fl, 1.0), full(s.sigma, 1.0), date, s.mask.copy())


def test_retrieve_components_under_a_baseline():
    """an SB2 chunk of 6 epochs x 40 pixels (N about 240, as the worker tests of loo and marg): with ``baseline`` the helper
    returns ``predict_marginal`` on the grids it reports, bit for bit, in every form of get_Sigma; without it, what it
    returned before the keyword existed"""
    from psoap_amd import covariance as cov, retrieve
    from psoap_amd.data import epoch_index_of
    from psoap_amd.utils import registered_params
    s = syn.make_chunk(2, 6, 40, seed=9810, masked_fraction=0.1)
    ch = _chunk2d(s)
    p_orb = syn.make_orbit_proposals("SB2", 1, seed=9811)[0]
    gp = syn.GP_BASE[2]
    pars = dict(zip(registered_params["SB2"], list(p_orb) + list(gp)))
    mask = np.asarray(ch.mask, dtype=bool)
    x, ep = np.log(np.asarray(ch.wl, dtype=np.float64))[mask], epoch_index_of(mask)
    fl, sigma = np.asarray(ch.fl, dtype=np.float64)[mask], np.asarray(ch.sigma, dtype=np.float64)[mask]
    M = 2 * ch.n_pix
    try:
        for kind in ("one", "flux"):
            base = {"order": 1, "sd": [0.05, 0.025], "weight": kind}
            weight = fl if kind == "flux" else None
            for get in (True, False, "diag"):
                out = retrieve.retrieve_components("SB2", ch, pars, get_Sigma=get, baseline=base)
                ref = cov.predict_marginal(out["lwls"], fl, sigma, [out["lwl_predict"]] * 2, [0.0, 0.0], gp, x, ep, 1, base["sd"], weight,
                                           mode=0, want_sigma=get)
                mu = ref if get is False else ref[0]
                assert _same_bits(out["mu"], mu) and _same_bits(out["mu_g"], mu[M:])
                if get is True:
                    assert _same_bits(out["Sigma"], ref[1]) and _same_bits(out["sigma_f"], np.sqrt(np.diag(ref[1]))[:M])
                elif get == "diag":
                    assert out["Sigma"] is None and _same_bits(out["sigma_g"], np.sqrt(ref[1])[M:])
                else:
                    assert out["Sigma"] is None and "sigma_f" not in out
        with pytest.raises(ValueError):
            retrieve.retrieve_components("SB2", ch, pars, baseline={"order": 1})
        # the continuum's uncertainty is in the error bars: nowhere smaller than the plain ones
        plain = retrieve.retrieve_components("SB2", ch, pars, get_Sigma="diag")
        marg = retrieve.retrieve_components("SB2", ch, pars, get_Sigma="diag", baseline={"order": 1, "sd": [0.05, 0.025]})
        assert np.all(marg["sigma_f"] ** 2 >= plain["sigma_f"] ** 2 - TOL["var"] * max(gp[0], gp[2]) ** 2)
        # baseline=None: the plain path, untouched
        none = retrieve.retrieve_components("SB2", ch, pars, baseline=None)
        old = cov.predict_f_g(none["lwls"][0], none["lwls"][1], fl, sigma, none["lwl_predict"], none["lwl_predict"], 0.0, gp[0], gp[1], 0.0,
                              gp[2], gp[3])
        assert _same_bits(none["mu"], old[0]) and _same_bits(none["Sigma"], old[1])
        again = retrieve.retrieve_components("SB2", ch, pars)
        assert _same_bits(none["mu"], again["mu"]) and _same_bits(none["Sigma"], again["Sigma"]) and sorted(none) == sorted(again)
    finally:
        cov.release_handles()
