"""GPU tests of leave-one-out cross-validation of the likelihood (psoap_chunk_loo, psoap_amd/csrc/loo_kernels.hpp).

The cases of tests/loo_reference.py -- the smallest shapes at which the band kernel, the scatter or the block batch can go
wrong -- against the long-double reference, output by output: pix_mean and ep_resid absolute; pix_var, ep_chi2 and loo_logp
relative; pix_logp and ep_logp relative to max(1, |value|).

The tolerance is derived, not fitted: the float64 SciPy evaluation of the same formulas (cho_factor / cho_solve,
loo_reference.loo_f64) measured against the long-double one on these very cases (python tests/loo_reference.py):

    case           pix_mean    pix_var   pix_logp   loo_logp   ep_resid    ep_chi2    ep_logp
    a-N100-c2      2.83e-15   2.93e-14   1.51e-13   1.02e-15   1.93e-15   3.03e-14   3.15e-15
    b-N128-c1      5.15e-16   2.89e-14   2.31e-14   6.72e-16   4.18e-15   8.09e-15   7.56e-16
    c-N129-c2      9.38e-16   2.63e-14   4.85e-14   5.84e-16   3.53e-15   7.59e-15   7.71e-17
    d-N384-c1      5.85e-15   9.46e-14   2.79e-13   2.70e-15   3.40e-15   1.48e-14   3.51e-15
    e-N700-c3      3.58e-15   1.23e-13   3.11e-13   2.03e-15   4.91e-15   6.50e-14   7.74e-16
    f-N300-c2      3.91e-15   9.95e-14   1.76e-13   1.16e-15   4.10e-15   2.56e-14   1.70e-15
    max            5.85e-15   1.23e-13   3.11e-13   2.70e-15   4.91e-15   6.50e-14   3.51e-15

The device sums in another order and fuses multiply-adds but is fp64 throughout: it gets the largest measured value of each
output times the project's margin of 8 (tests/test_gpu_grad.py).  Nothing is fitted to the device's own results.

ChunkWorker.loo is compared with the reference on the grids of the LONG-DOUBLE orbit, while the worker shifts its grid in
float64: half an ulp of a ln-wavelength (9e-16) moves an element of K by 2 |p_c| d 9e-16 ~ 3e-11 of itself at the benchmark
length scales, which no evaluation on float64 grids can undo.  The grid difference demands a wider margin there, measured
the same way: loo_f64 on the float64 grids (the long-double velocities rounded, shifted as the worker shifts them) against
loo_ext on the long-double grids, on the SB2 chunk of that test (loo_reference.planted):

    SB2-N240       2.89e-11   1.70e-10   2.34e-09   8.00e-12   3.32e-11   8.30e-11   2.76e-11

again times 8.  (The same float64 evaluation against loo_ext on ITS OWN grids: 1.14e-14 .. 1.15e-12.)
"""
import ctypes

import numpy as np
import pytest

import loo_reference as lr
from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu

MARGIN = 8
F64 = {"pix_mean": 5.85e-15, "pix_var": 1.23e-13, "pix_logp": 3.11e-13, "loo_logp": 2.70e-15, "ep_resid": 4.91e-15,
       "ep_chi2": 6.50e-14, "ep_logp": 3.51e-15}        # the table above, last row
TOL = {k: MARGIN * v for k, v in F64.items()}
F64_ORBIT = {"pix_mean": 2.89e-11, "pix_var": 1.70e-10, "pix_logp": 2.34e-09, "loo_logp": 8.00e-12, "ep_resid": 3.32e-11,
             "ep_chi2": 8.30e-11, "ep_logp": 2.76e-11}        # the SB2 row above: float64 grids against long-double grids
TOL_ORBIT = {k: MARGIN * v for k, v in F64_ORBIT.items()}
PIXEL_FIELDS = ("pix_mean", "pix_var", "pix_logp", "pix_z")
EPOCH_FIELDS = ("ep_resid", "ep_chi2", "ep_logp", "ep_npix")


def _handle(ch, **kw):
    from psoap_amd.chunk import ChunkHandle
    return ChunkHandle(ch.fl, ch.sigma, **kw)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_result(a, b, fields=PIXEL_FIELDS + EPOCH_FIELDS):
    return _same_bits(a.lnp, b.lnp) and _same_bits(a.loo_logp, b.loo_logp) and \
        all(_same_bits(getattr(a, f), getattr(b, f)) for f in fields)


def _check(name, got, ref, tol=TOL):
    err = lr.errors(got, ref)
    print(f"{name}: " + ", ".join(f"{k} {v:.2e} ({tol[k]:.2e})" for k, v in err.items()))
    for k, v in err.items():
        assert v <= tol[k], (name, k, v, tol[k])


@pytest.mark.parametrize("case", lr.CASES, ids=lr.case_id)
def test_loo_against_long_double(case):
    ch, gp, ref = lr.case_chunk(case), lr.case_gp(case), lr.case_ext(case)
    with _handle(ch) as h:
        got = h.loo(ch.lwls, gp, lr.MU_GP, ch.epoch_index, ch.n_epochs)
        again = h.loo(ch.lwls, gp, lr.MU_GP, ch.epoch_index, ch.n_epochs)
        lnp = h.lnlike_grad(ch.lwls, gp, lr.MU_GP)[0]
        pixels_only = h.loo(ch.lwls, gp, lr.MU_GP)
    assert _same_bits(got.lnp, lnp) and np.isfinite(lnp)                      # the bits of lnlike_grad
    assert _same_result(got, again)                                          # two calls, the same bits
    assert _same_result(got, pixels_only, PIXEL_FIELDS)                       # the pixel outputs do not depend on the epochs
    assert pixels_only.ep_resid is None and pixels_only.ep_chi2 is None and pixels_only.ep_npix is None
    assert got.ep_npix.dtype == np.int32 and list(got.ep_npix) == list(ref.ep_npix)
    for e in np.flatnonzero(ref.ep_npix == 0):                               # an empty epoch: exact zeros
        assert _same_bits(got.ep_chi2[e], np.float64(0.0)) and _same_bits(got.ep_logp[e], np.float64(0.0))
    for f in PIXEL_FIELDS + EPOCH_FIELDS[:3]:
        assert np.all(np.isfinite(getattr(got, f))), f
    _check(lr.case_id(case), got, ref)
    z_err = float(np.max(np.abs(np.asarray(got.pix_z, dtype=np.longdouble) - ref.pix_z) / np.maximum(1, np.abs(ref.pix_z))))
    assert z_err <= TOL["pix_logp"], z_err                                    # derived from pix_mean and pix_var in Python


def test_raw_abi_null_outputs_and_null_epoch():
    from psoap_amd import _lib
    case = lr.case_named("c")
    ch, gp = lr.case_chunk(case), lr.case_gp(case)
    dp, ip = _lib.dptr, lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    lw, g, ep = np.ascontiguousarray(ch.lwls), np.ascontiguousarray(gp), np.ascontiguousarray(ch.epoch_index, dtype=np.int32)
    with _handle(ch) as h:
        full = h.loo(ch.lwls, gp, lr.MU_GP, ch.epoch_index, ch.n_epochs)
        L = h._L
        chi2, var, lnp = np.empty(2), np.empty(ch.fl.shape[0]), np.empty(1)
        # everything NULL but ep_chi2; then pix_var and lnp alone with epoch == NULL (the ep_* pointers are ignored)
        assert L.psoap_chunk_loo(h._h, 2, dp(lw), dp(g), lr.MU_GP, ip(ep), 2, None, None, None, None, None, None, dp(chi2), None,
                                 None) == 0
        junk = np.full(2, 7.0)
        assert L.psoap_chunk_loo(h._h, 2, dp(lw), dp(g), lr.MU_GP, None, 0, dp(lnp), None, None, dp(var), None, None, dp(junk), None,
                                 None) == 0
        assert L.psoap_chunk_loo(h._h, 2, dp(lw), dp(g), lr.MU_GP, None, 0, None, None, None, None, None, None, None, None, None) == 0
    assert _same_bits(chi2, full.ep_chi2) and _same_bits(var, full.pix_var) and _same_bits(lnp[0], np.float64(full.lnp))
    assert list(junk) == [7.0, 7.0]


def test_conventions_negative_amplitude_refusals_open_stream_release():
    from psoap_amd._lib import PsoapError
    from psoap_amd.chunk import ChunkHandle
    case = lr.case_named("f")
    ch, gp, c = lr.case_chunk(case), lr.case_gp(case), case[2]
    N = ch.fl.shape[0]
    with _handle(ch) as h:
        good = h.loo(ch.lwls, gp, lr.MU_GP, ch.epoch_index, ch.n_epochs)
        neg = gp.copy()
        neg[0] = -neg[0]
        bad = h.loo(ch.lwls, neg, lr.MU_GP, ch.epoch_index, ch.n_epochs)          # status 0: no exception
        assert bad.lnp == -np.inf and np.isnan(bad.loo_logp)
        for f in PIXEL_FIELDS + EPOCH_FIELDS[:3]:
            assert np.all(np.isnan(getattr(bad, f))), f
        assert list(bad.ep_npix) == [100, 100, 100]
        split = ch.epoch_index.copy()
        split[-1] = split[0]
        with pytest.raises(PsoapError, match="not contiguous"):
            h.loo(ch.lwls, gp, lr.MU_GP, split, ch.n_epochs)
        with pytest.raises(PsoapError, match="out of range"):
            h.loo(ch.lwls, gp, lr.MU_GP, ch.epoch_index, 2)
        with pytest.raises(PsoapError, match="n_epochs"):
            h.loo(ch.lwls, gp, lr.MU_GP, ch.epoch_index, 0)
        h.stream_open(c, 1)
        try:
            with pytest.raises(PsoapError, match="open stream"):
                h.loo(ch.lwls, gp, lr.MU_GP, ch.epoch_index, ch.n_epochs)
        finally:
            h.stream_close()
        # release, twice, then another call: the workspace comes back, and so do the bits
        h.loo_release()
        h.loo_release()
        assert _same_result(h.loo(ch.lwls, gp, lr.MU_GP, ch.epoch_index, ch.n_epochs), good)
    # not positive definite: zero noise and two identical pixels
    lw = ch.lwls.copy()
    lw[:, 1] = lw[:, 0]
    with ChunkHandle(ch.fl, np.zeros_like(ch.sigma)) as h:
        bad = h.loo(lw, gp, lr.MU_GP, ch.epoch_index, ch.n_epochs)
    assert bad.lnp == -np.inf and np.all(np.isnan(bad.pix_mean)) and np.all(np.isnan(bad.ep_chi2)) and bad.pix_mean.shape == (N,)


def test_loo_leaves_the_handle_as_it_was():
    """an uploaded batch evaluates to the same bits before and after a loo call on the same handle"""
    case = lr.case_named("f")
    lc, gp = lr.case_chunk(case), lr.case_gp(case)
    ch = syn.make_chunk(2, 3, 100, seed=9300)
    gps = syn.make_walkers(2, 4, seed=9301)
    lw = syn.walker_lwls(ch, syn.make_walker_velocities(ch, 4, seed=9302))
    with _handle(lc, max_batch=4) as h:
        before = h.lnlike_batch(lw, gps, 0.9)
        h.upload(lw[::-1].copy(), gps[::-1].copy(), 0.9)
        h.loo(lc.lwls, gp, lr.MU_GP, lc.epoch_index, lc.n_epochs)
        h.eval()
        pending = h.fetch()
        after = h.lnlike_batch(lw, gps, 0.9)
    assert _same_bits(before, after) and _same_bits(pending, before[::-1])


def test_covariance_loo_goes_through_the_cached_handle():
    from psoap_amd import covariance
    case = lr.case_named("a")
    ch, gp = lr.case_chunk(case), lr.case_gp(case)
    try:
        res = covariance.loo(ch.lwls, ch.fl, ch.sigma, gp, lr.MU_GP, ch.epoch_index)
        cached = list(covariance._handles.values())
        again = covariance.loo(ch.lwls, ch.fl, ch.sigma, gp, lr.MU_GP, ch.epoch_index)
        assert [id(h) for h in covariance._handles.values()] == [id(h) for h in cached]
    finally:
        covariance.release_handles()
    assert _same_result(res, again)
    _check("covariance.loo a", res, lr.case_ext(case))


# ---- lnprob(p): grids from the orbit -------------------------------------------------------------------------------------
def _planted_worker(fix=()):
    from psoap_amd.lnprob import ChunkWorker
    from psoap_amd.utils import registered_params
    ch, p_orb, gp, lwls = lr.planted()
    full = dict(zip(registered_params["SB2"], list(p_orb) + list(gp)))
    w = ChunkWorker("SB2", ch.lwl, ch.fl, ch.sigma, ch.epoch_index, ch.dates, fix_params=list(fix), defaults=full)
    p = np.array([full[n] for n in registered_params["SB2"] if n not in fix])
    return ch, w, p, gp, lwls


def test_worker_loo_against_long_double_on_the_long_double_orbit():
    """SB2, 6 epochs x 40 pixels, orbit from synthetic.make_orbit_proposals: ChunkWorker.loo(p) against the reference on the
    grids shifted by the long-double orbit, at the margin the float64 grids demand (TOL_ORBIT: the module's docstring)."""
    ch, w, p, gp, lwls = _planted_worker(fix=("gamma",))
    try:
        got = w.loo(p, lr.MU_GP)
        lnp = w.lnprob(p, lr.MU_GP)
    finally:
        w.close()
    ref = lr.loo_ext(lwls, ch.fl, ch.sigma, gp, lr.MU_GP, ch.epoch_index, lr.PLANT_EPOCHS)
    assert list(got.ep_npix) == [lr.PLANT_PIX] * lr.PLANT_EPOCHS
    assert abs(got.lnp - lnp) <= 1e-9 * abs(lnp)
    _check("SB2 worker", got, ref, TOL_ORBIT)


def test_planted_outliers_are_found_and_become_one_mask_row(tmp_path):
    from psoap_amd import data, lnprob
    ch, w, p, _, _ = _planted_worker()
    try:
        found = lnprob.loo_outliers([w], p, mu_GP=lr.MU_GP)
    finally:
        w.close()
    assert len(found) == 1
    assert list(found[0]["pixels"]) == [lr.PLANT_PIXEL] and list(found[0]["epochs"]) == [lr.PLANT_EPOCH]
    rows = lnprob.loo_mask_rows([(5190.0, 5200.0, ch.dates)], found)
    assert len(rows) == 1 and rows[0][:2] == (5190.0, 5200.0)
    assert rows[0][2] < ch.dates[lr.PLANT_EPOCH] < rows[0][3] and abs((rows[0][3] - rows[0][2]) - 0.2) < 1e-6
    fname = str(tmp_path / "masks.dat")
    data.write_mask_table(fname, rows)
    back = data.read_mask_table(fname)
    assert len(back) == 1 and back[0][2] < ch.dates[lr.PLANT_EPOCH] < back[0][3]


def test_faster_than_light_orbit_and_server_refusal(monkeypatch):
    from psoap_amd._lib import PsoapError
    ch, w, p, gp, _ = _planted_worker()
    try:
        p_orb = np.array(lr.planted()[1])
        p_orb[1] = 4.0e5                                   # K in km/s: |v| >= c
        res = w.loo_orbits(p_orb, gp, lr.MU_GP)
        assert res.lnp == -np.inf and np.all(np.isnan(res.pix_mean)) and np.all(np.isnan(res.ep_chi2))
        assert list(res.ep_npix) == [lr.PLANT_PIX] * lr.PLANT_EPOCHS
        monkeypatch.setenv("PSOAP_GPU_SERVER", "auto")
        with pytest.raises(PsoapError, match="PSOAP_GPU_SERVER"):
            w.loo(p, lr.MU_GP)
    finally:
        w.close()
