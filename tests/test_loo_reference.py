"""CPU tests of the leave-one-out formulas and of their host-side surface (tests/loo_reference.py, psoap_amd.lnprob,
psoap_amd.data): no GPU.

The closed forms in long double against the brute-force route that really deletes a pixel or an epoch and conditions on the
rest: 1e-10 absolute on means and residuals, 1e-9 relative on ep_chi2 -- three orders above the measured agreement (1e-15 ..
1e-12); they guard the formulas, not the rounding."""
import numpy as np
import pytest

import loo_reference as lr
import orbit_ext as oe

_LD = np.longdouble
needs_ext = pytest.mark.skipif(not oe.have_ext(), reason=oe.skip_reason())

ABS_BOUND, CHI2_REL_BOUND = 1e-10, 1e-9


def _epoch_check(case, epochs):
    ch, gp, ref = lr.case_chunk(case), lr.case_gp(case), lr.case_ext(case)
    for e in epochs:
        I = np.flatnonzero(ch.epoch_index == e)
        resid, chi2 = lr.delete_epoch(ch.lwls, ch.fl, ch.sigma, gp, lr.MU_GP, I)
        d_res = float(np.max(np.abs(resid - ref.ep_resid[I])))
        d_chi = float(abs(chi2 - ref.ep_chi2[e]) / chi2)
        print(f"{lr.case_id(case)} epoch {e} ({I.size} px): resid {d_res:.2e}, chi2 {d_chi:.2e}")
        assert d_res <= ABS_BOUND and d_chi <= CHI2_REL_BOUND
        assert ref.ep_npix[e] == I.size


@needs_ext
def test_every_pixel_of_case_a_against_deleting_it():
    case = lr.case_named("a")
    ch, gp, ref = lr.case_chunk(case), lr.case_gp(case), lr.case_ext(case)
    worst_m = worst_v = 0.0
    for i in range(ch.fl.shape[0]):
        mean, var = lr.delete_pixel(ch.lwls, ch.fl, ch.sigma, gp, lr.MU_GP, i)
        worst_m = max(worst_m, float(abs(mean - ref.pix_mean[i])))
        worst_v = max(worst_v, float(abs(var - ref.pix_var[i]) / var))
        # the log predictive density of the deleted pixel under that prediction
        logp = _LD(-0.5) * (np.log(_LD(8) * np.arctan(_LD(1)) * var) + (_LD(ch.fl[i]) - mean) ** 2 / var)
        assert abs(logp - ref.pix_logp[i]) <= 1e-9 * max(1.0, abs(float(logp)))
    print(f"case a, 100 pixels: mean {worst_m:.2e}, var (relative) {worst_v:.2e}")
    assert worst_m <= ABS_BOUND and worst_v <= CHI2_REL_BOUND
    assert float(abs(ref.loo_logp - np.sum(ref.pix_logp))) <= 1e-12 * abs(float(ref.loo_logp))


@needs_ext
@pytest.mark.parametrize("name, epochs", [("a", (0, 3)), ("c", (0, 1)), ("f", (2, 1))])
def test_first_last_and_one_pixel_epochs_against_deleting_them(name, epochs):
    """case a: first and last; case c: the first (128 pixels) and the last, which is the one-pixel epoch; case f: the first
    and the last run of the flattened order (ids 2 and 1)"""
    _epoch_check(lr.case_named(name), epochs)


@needs_ext
def test_a_one_pixel_epoch_is_that_pixel_and_an_empty_epoch_is_zero():
    ref_c = lr.case_ext(lr.case_named("c"))
    assert abs(ref_c.ep_resid[128] - (lr.case_chunk(lr.case_named("c")).fl[128] - ref_c.pix_mean[128])) <= 1e-15
    assert abs(ref_c.ep_logp[1] - ref_c.pix_logp[128]) <= 1e-15 * abs(ref_c.ep_logp[1])
    ch = lr.case_chunk(lr.case_named("e"))
    assert list(np.bincount(ch.epoch_index, minlength=5)) == [1, 299, 0, 130, 270]


@needs_ext
def test_planted_outliers_are_exactly_what_the_reference_flags():
    """the inputs of the GPU test (tests/test_gpu_loo.py): +0.3 on one pixel, +0.05 on every pixel of one epoch of a chunk
    drawn from its own GP -- the long-double reference flags that pixel and that epoch and nothing else"""
    ch, _, gp, lwls = lr.planted()
    ref = lr.loo_ext(lwls, ch.fl, ch.sigma, gp, lr.MU_GP, ch.epoch_index, lr.PLANT_EPOCHS)
    pixels, epochs = lr.flag(ref)
    assert list(pixels) == [lr.PLANT_PIXEL] and list(epochs) == [lr.PLANT_EPOCH]
    assert ch.epoch_index[lr.PLANT_PIXEL] == lr.PLANT_EPOCH


def test_write_mask_table_round_trips_with_the_reference_header_and_formats(tmp_path):
    from psoap_amd import data
    rows = [(5160.0, 5190.04, 2455123.456789, 2455123.656789), (5200.26, 5230.0, 2455300.0, 2455300.2)]
    fname = str(tmp_path / "masks.dat")
    data.write_mask_table(fname, rows)
    text = open(fname).read().splitlines()
    assert text[0] == "wl0 wl1 t0 t1"
    assert text[1] == "5160.0 5190.0 2455123.46 2455123.66" and text[2] == "5200.3 5230.0 2455300.00 2455300.20"
    back = data.read_mask_table(fname)
    assert back == [(5160.0, 5190.0, 2455123.46, 2455123.66), (5200.3, 5230.0, 2455300.0, 2455300.2)]
    data.write_mask_table(fname, [])
    assert data.read_mask_table(fname) == []


def test_loo_mask_rows_pads_dates_by_a_tenth_of_a_day():
    from psoap_amd import lnprob
    dates = np.array([2455001.0, 2455002.5, 2455010.25])
    found = [{"pixels": np.array([3]), "epochs": np.array([2, 0])}, {"pixels": np.array([], dtype=int), "epochs": np.array([], dtype=int)}]
    meta = [(5160.0, 5190.0, dates), (5190.0, 5220.0, dates)]
    rows = lnprob.loo_mask_rows(meta, found)
    assert rows == [(5160.0, 5190.0, 2455010.25 - 0.1, 2455010.25 + 0.1), (5160.0, 5190.0, 2455001.0 - 0.1, 2455001.0 + 0.1)]
    assert lnprob.loo_mask_rows(meta, found, pad_days=0.5)[0][2:] == (2455009.75, 2455010.75)


def test_python_surface_and_degenerate_input_without_gpu():
    """-inf / NaN before any device work for a negative hyper-parameter, as ``lnlike_grad``; l == 0 raises"""
    from psoap_amd import covariance, lnprob
    from psoap_amd.chunk import ChunkHandle, LooResult
    assert callable(ChunkHandle.loo) and callable(ChunkHandle.loo_release)
    assert callable(lnprob.ChunkWorker.loo) and callable(lnprob.ChunkWorker.loo_orbits) and callable(lnprob.loo_outliers)
    x = np.linspace(8.5, 8.5001, 6)
    ep = np.array([0, 0, 0, 2, 2, 2])
    res = covariance.loo([x, x], x, x, [0.2, 5.0, -0.1, 7.0], epoch_index=ep)
    assert isinstance(res, LooResult) and res.lnp == -np.inf and np.isnan(res.loo_logp)
    for v in (res.pix_mean, res.pix_var, res.pix_logp, res.pix_z, res.ep_resid):
        assert v.shape == (6,) and np.all(np.isnan(v))
    assert np.all(np.isnan(res.ep_chi2)) and np.all(np.isnan(res.ep_logp)) and list(res.ep_npix) == [3, 0, 3]
    assert covariance.loo([x], x, x, [-0.2, 5.0]).ep_chi2 is None
    with pytest.raises(ZeroDivisionError):
        covariance.loo([x], x, x, [0.2, 0.0])
    with pytest.raises(ValueError):
        covariance.loo([x], x, x, [np.nan, 5.0])
