"""GPU tests of the component spectra at a date under the time-variable kernel (psoap_chunk_predict_tv, _predict_tv_var;
k_fill_region_tv in psoap_amd/csrc/predict_kernels.hpp, predict_tv_run in predict_host.hpp).

The cases of tests/timevar_predict_reference.py -- the data of timevar_reference.CASES at the smallest shapes where a tile
edge of either block of [K | Cx^T] can go wrong, with one date, two dates, a date on an epoch, between two and beyond the
span -- against the long-double reference on the dense matrices, output by output: mu absolute; Sigma and the variances
absolute in units of the largest prior variance.

The tolerance is derived, not fitted: the float64 SciPy evaluation of the device's own route
(timevar_predict_reference.tv_predict_f64) measured against the long-double one on these very cases
(python tests/timevar_predict_reference.py):

    case                                     mu      Sigma        var
    N100-c2-mode0-M50-epoch            1.89e-15   1.60e-15   4.18e-16
    N100-c2-mode1-M130-mid             1.66e-15   1.21e-15   7.34e-16
    N300-c1-mode2-M129-one             2.46e-15   2.17e-15   1.33e-15
    N129-c2-mode0-M65-two              2.53e-15   1.26e-15   7.08e-16
    N300-c3-mode0-M43-beyond           1.10e-15   2.91e-16   1.67e-16
    N300-c2-perm-mode0-M100-two        7.78e-15   2.80e-15   1.33e-15
    N520-c2-mode0-M64-two              3.91e-15   1.55e-15   1.36e-15
    max                                7.78e-15   2.80e-15   1.36e-15

The device sums in another order and fuses multiply-adds but is fp64 throughout: it gets the largest measured value of each
output times the project's margin of 8 (tests/test_gpu_grad.py).  Nothing is fitted to the device's own results
(profiles/predict_timevar.md has them).

Two rules make the rest exact.  Rule 1: with every tau = +inf the outputs have the bits of the plain predict on the staged
route -- run in a child process, PSOAP_SHARE_POLICY is read once per process.  Rule 2: a component with a finite tau whose
every temporal argument is <= -746 gets its prior back exactly.
"""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import timevar_predict_reference as tp
import timevar_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

MARGIN = 8
F64 = {"mu": 7.78e-15, "Sigma": 2.80e-15, "var": 1.36e-15}          # the table above, last row
TOL = {k: MARGIN * v for k, v in F64.items()}
LD = np.longdouble
U53 = 2.0 ** -53


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _handle(d, flux=None):
    from psoap_amd.chunk import ChunkHandle
    h = ChunkHandle(d.fl if flux is None else np.full_like(d.fl, flux), d.sigma)
    h.set_times(d.times)
    return h


def _call(pc, **kw):
    """-> (mode, lwls, pred, t_pred, mus, gp, tau) of a case: what ``predict_tv`` takes"""
    mode, lwls, _times, _fl, _sigma, pred, t_pred, mus, gp, tau = tp.pcase_args(pc, **kw)
    return mode, lwls, pred, t_pred, mus, gp, tau


@functools.lru_cache(maxsize=None)
def device(pc):
    """every form of one case, once per session: -> dict(full=(mu, Sigma), mean=mu, diag=(mu, var))"""
    args = _call(pc)
    with _handle(tr.case_data(tp.tv_case(pc))) as h:
        return {"full": h.predict_tv(*args), "mean": h.predict_tv(*args, want_sigma=False), "diag": h.predict_tv(*args, want_sigma="diag")}


def _check(name, err):
    print(f"{name}: " + ", ".join(f"{k} {v:.2e} ({TOL[k]:.2e})" for k, v in err.items()))
    for k, v in err.items():
        assert v <= TOL[k], (name, k, v, TOL[k])


# ---- parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", tp.PCASES, ids=tp.pcase_id)
def test_predict_tv_against_long_double(pc):
    got, ref = device(pc), tp.pcase_ext(pc)
    mu, Sigma = got["full"]
    R = ref.mu.shape[0]
    assert mu.shape == (R,) and Sigma.shape == (R, R) and got["diag"][1].shape == (R,)
    _check(tp.pcase_id(pc), tp.errors(mu, Sigma, got["diag"][1], ref))


# ---- invariances ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", tp.PCASES, ids=tp.pcase_id)
def test_the_three_forms_agree(pc):
    got = device(pc)
    (mu, Sigma), (mu_d, _var) = got["full"], got["diag"]
    assert _same_bits(mu, got["mean"]) and _same_bits(mu, mu_d)
    assert _same_bits(Sigma, Sigma.T)


# ---- rule 1: tau = inf is the static predict on the staged route, bit for bit ------------------------------------------------
_RULE1 = r'''
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import timevar_predict_reference as tp
import timevar_reference as tr
from psoap_amd import _lib
from psoap_amd.chunk import ChunkHandle

def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()

done = []
for k in %(cases)r:
    pc = tp.PCASES[k]
    mode, lwls, times, fl, sigma, pred, t_pred, mus, gp, tau = tp.pcase_args(pc)
    inf = np.full(lwls.shape[0], np.inf)
    with ChunkHandle(fl, sigma) as h:
        h.set_times(times)
        mu, Sigma = h.predict(mode, lwls, pred, mus, gp)
        R = mu.shape[0]
        z = np.random.default_rng(5 + k).standard_normal((3, R))
        draws = h.predict_draw(3, z=z)
        mu_d, var = h.predict(mode, lwls, pred, mus, gp, want_sigma="diag")
        mu_m = h.predict(mode, lwls, pred, mus, gp, want_sigma=False)
        tmu, tSigma = h.predict_tv(mode, lwls, pred, t_pred, mus, gp, inf)
        tdraws = h.predict_draw(3, z=z)
        tmu_d, tvar = h.predict_tv(mode, lwls, pred, t_pred, mus, gp, inf, want_sigma="diag")
        tmu_m = h.predict_tv(mode, lwls, pred, t_pred, mus, gp, inf, want_sigma=False)
        # any other finite dates: the same bits
        smu, sSigma = h.predict_tv(mode, lwls, pred, t_pred[::-1] * 3.0 - 11.0, mus, gp, inf)
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(Sigma)) and np.all(np.isfinite(draws)), tp.pcase_id(pc)
    for name, a, b in (("mu", mu, tmu), ("Sigma", Sigma, tSigma), ("draws", draws, tdraws), ("mu (diag)", mu_d, tmu_d), ("var", var, tvar),
                       ("mu (alone)", mu_m, tmu_m), ("mu (other dates)", mu, smu), ("Sigma (other dates)", Sigma, sSigma)):
        assert same(a, b), (tp.pcase_id(pc), name, float(np.max(np.abs(np.asarray(a) - np.asarray(b)))))
    done.append(tp.pcase_id(pc))
stats = _lib.share_stats()
print("RESULT " + json.dumps({"done": done, "staged_policy": stats["staged_policy"], "dag_launches": stats["dag_launches"]}))
'''


def test_rule_1_infinite_tau_is_the_static_predict_on_the_staged_route(tmp_path):
    """modes 0 (two and three components), 1 and 2 in ONE fresh child under PSOAP_SHARE_POLICY=staged: mu, Sigma, the variances
    and the draws for a fixed z after each call.  The child stops at its first failed assertion."""
    cases = [3, 4, 1, 2]          # N129-c2 mode 0 (two dates), N300-c3 mode 0, N100-c2 mode 1, N300-c1 mode 2
    assert [tp.PCASES[k][1] for k in cases] == [0, 0, 1, 2]
    code = _RULE1 % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "cases": cases}
    env = dict(os.environ, PSOAP_SHARE_POLICY="staged", PSOAP_LOCK_DIR=str(tmp_path / "locks"))
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    line, = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
    out = json.loads(line[len("RESULT "):])
    assert out["done"] == [tp.pcase_id(tp.PCASES[k]) for k in cases]
    assert out["staged_policy"] >= 1 and out["dag_launches"] == 0, out      # the plain calls did take the staged route


# ---- rule 2: a date out of reach returns the prior exactly -----------------------------------------------------------------------
def _far(d):
    """a date from which every pixel is further than sqrt(2 * 746) of the largest finite tau (plus a percent)"""
    return float(np.max(d.times) + 1.01 * np.sqrt(2 * 746.0) * np.max(d.tau[np.isfinite(d.tau)]))


def _device_prior(pred_k, t_pred, gp_k, tau_k):
    """the prior block of one component from the device's OTHER time-variable fill (k_fill_sym_tv, tests/test_gpu_timevar.py)"""
    from psoap_amd import matrix_functions as mf
    A = np.empty((pred_k.shape[0], pred_k.shape[0]))
    mf.fill_V11_timevar(A, pred_k[None, :], t_pred, gp_k, [tau_k])
    return A


def test_rule_2_one_component_out_of_reach():
    pc = tp.PCASES[2]               # N300-c1, mode 2, M = 129
    d = tr.case_data(tp.tv_case(pc))
    mode, lwls, pred, t_pred, mus, gp, tau = _call(pc, dates=[_far(d)])
    assert np.all(np.isfinite(tau)) and np.all(tp.cross_args_f64(lwls, d.times, pred, t_pred, gp, tau) <= -746.0)
    with _handle(d) as h:
        mu, Sigma = h.predict_tv(mode, lwls, pred, t_pred, mus, gp, tau)
        mu_d, var = h.predict_tv(mode, lwls, pred, t_pred, mus, gp, tau, want_sigma="diag")
    assert _same_bits(mu, np.full(pc[2], mus[0])) and _same_bits(mu_d, mu)
    assert _same_bits(Sigma, _device_prior(pred[0], t_pred, gp[:2], tau[0]))
    assert _same_bits(var, np.full(pc[2], gp[0] * gp[0]))
    assert _same_bits(np.diag(Sigma).copy(), var)


def test_rule_2_the_finite_component_of_two_out_of_reach():
    pc = tp.PCASES[0]               # N100-c2, mode 0, M = 50: tau = (0.25 span, inf)
    d = tr.case_data(tp.tv_case(pc))
    M = pc[2]
    mode, lwls, pred, t_pred, mus, gp, tau = _call(pc, dates=[_far(d)])
    assert np.isfinite(tau[0]) and np.isinf(tau[1])
    assert np.all(tp.cross_args_f64(lwls, d.times, pred, t_pred, gp, tau)[0] <= -746.0)
    with _handle(d) as h:
        mu, Sigma = h.predict_tv(mode, lwls, pred, t_pred, mus, gp, tau)
        _mu_d, var = h.predict_tv(mode, lwls, pred, t_pred, mus, gp, tau, want_sigma="diag")
    assert _same_bits(mu[:M], np.full(M, mus[0]))
    assert _same_bits(Sigma[:M, :M], _device_prior(pred[0], t_pred, gp[:2], tau[0]))
    assert np.all(Sigma[:M, M:] == 0.0) and np.all(Sigma[M:, :M] == 0.0)
    assert _same_bits(var[:M], np.full(M, gp[0] * gp[0]))
    # the static component is conditioned as ever: the whole result against the long-double reference
    assert np.max(np.abs(mu[M:] - mus[1])) > 1e-3
    ref = tp.tv_predict_ext(*tp.pcase_args(pc, dates=[_far(d)]), L=tp.pcase_factor(pc))
    _check("N100-c2 far", tp.errors(mu, Sigma, var, ref))


# ---- conventions --------------------------------------------------------------------------------------------------------------
def test_refusals():
    from psoap_amd._lib import PsoapError
    from psoap_amd.chunk import ChunkHandle
    pc = tp.PCASES[0]
    d = tr.case_data(tp.tv_case(pc))
    mode, lwls, pred, t_pred, mus, gp, tau = _call(pc)
    with ChunkHandle(d.fl, d.sigma) as h:
        for want in (True, "diag"):
            with pytest.raises(PsoapError, match="call psoap_chunk_set_times first"):
                h.predict_tv(mode, lwls, pred, t_pred, mus, gp, tau, want_sigma=want)
        h.set_times(d.times)
        good = h.predict_tv(mode, lwls, pred, t_pred, mus, gp, tau)
        for bad in (0.0, -1.0, np.nan):
            with pytest.raises(PsoapError, match="every tau must be a time scale"):
                h.predict_tv(mode, lwls, pred, t_pred, mus, gp, [tau[0], bad])
        for bad in (np.inf, -np.inf, np.nan):
            t_bad = t_pred.copy()
            t_bad[-1] = bad
            with pytest.raises(PsoapError, match="t_pred must be finite"):
                h.predict_tv(mode, lwls, pred, t_bad, mus, gp, tau)
        with pytest.raises(PsoapError, match="mode 2"):
            h.predict_tv(2, lwls, pred, t_pred, mus, gp, tau)
        with pytest.raises(PsoapError, match="mode 0"):
            h.predict_tv(0, lwls[:1], pred[:1], t_pred, mus[:1], gp[:2], tau[:1])
        with pytest.raises(PsoapError, match="mode 1"):
            h.predict_tv(1, lwls[:1], pred[:1], t_pred, mus[:1], gp[:2], tau[:1])
        h.stream_open(2, 1)
        try:
            with pytest.raises(PsoapError, match="open stream"):
                h.predict_tv(mode, lwls, pred, t_pred, mus, gp, tau)
        finally:
            h.stream_close()
        ep = np.zeros(d.fl.shape[0], dtype=np.int64)
        h.set_baseline(0, d.lwls[0], ep, 1, [0.05])
        with pytest.raises(PsoapError, match="the time-variable kernel under the marginalised continuum is not built yet"):
            h.predict_tv(mode, lwls, pred, t_pred, mus, gp, tau)
    with _handle(d) as h:      # (a refused call leaves nothing behind: a fresh handle gives the same bits)
        again = h.predict_tv(mode, lwls, pred, t_pred, mus, gp, tau)
        assert _same_bits(good[0], again[0]) and _same_bits(good[1], again[1])
        t = h.predict_timings()
        assert t["flops"] > 0 and t["device_ms"] > 0 and t["factor_ms"] > 0
        h.set_profiling(True)
        h.predict_tv(mode, lwls, pred, t_pred, mus, gp, tau)
        booked = h.timings()
        print(booked)
    d3 = tr.case_data(tp.tv_case(tp.PCASES[4]))
    with _handle(d3) as h:
        with pytest.raises(PsoapError, match="three components"):
            h.predict_tv(1, d3.lwls, np.tile(d3.lwls[0], (3, 1)), d3.times, [tr.MU_GP], d3.gp, d3.tau)


def test_a_data_covariance_that_is_not_positive_definite_raises_and_the_handle_stays_usable():
    """zero noise and two identical pixels at one time: status 1 and NaN through the raw ABI, LinAlgError from every form of
    the wrapper; with the noise back the handle gives the bits of a fresh one"""
    from psoap_amd import _lib
    pc = tp.PCASES[0]
    d = tr.case_data(tp.tv_case(pc))
    mode, lwls, pred, t_pred, mus, gp, tau = _call(pc)
    lw, times = lwls.copy(), d.times.copy()
    lw[:, 1] = lw[:, 0]
    times[1] = times[0]
    R = 2 * pc[2]
    with _handle(d) as h:
        h.set_data(d.fl, np.zeros_like(d.sigma))
        h.set_times(times)
        for want in (True, False, "diag"):
            with pytest.raises(np.linalg.LinAlgError):
                h.predict_tv(mode, lw, pred, t_pred, mus, gp, tau, want_sigma=want)
        with pytest.raises(_lib.PsoapError, match="no predict call has formed Sigma"):
            h.predict_draw(1, seed=1)
        mu, Sigma, var, status = np.zeros(R), np.zeros((R, R)), np.zeros(R), ctypes.c_int(-1)
        a = [_lib.as_f64(v) for v in (lw, pred, t_pred, mus, gp, tau)]
        rc = _lib.load().psoap_chunk_predict_tv(h._h, mode, 2, pc[2], *[_lib.dptr(v) for v in a], _lib.dptr(mu), _lib.dptr(Sigma),
                                                ctypes.byref(status))
        assert (rc, status.value) == (0, 1) and np.all(np.isnan(mu)) and np.all(np.isnan(Sigma))
        status = ctypes.c_int(-1)
        rc = _lib.load().psoap_chunk_predict_tv_var(h._h, mode, 2, pc[2], *[_lib.dptr(v) for v in a], _lib.dptr(mu), _lib.dptr(var),
                                                    ctypes.byref(status))
        assert (rc, status.value) == (0, 1) and np.all(np.isnan(mu)) and np.all(np.isnan(var))
        h.set_data(d.fl, d.sigma)
        h.set_times(d.times)
        after = h.predict_tv(mode, lwls, pred, t_pred, mus, gp, tau)
    fresh = device(pc)["full"]
    assert _same_bits(after[0], fresh[0]) and _same_bits(after[1], fresh[1])


# ---- draws ----------------------------------------------------------------------------------------------------------------------
def test_draws_follow_the_time_variable_posterior():
    """after predict_tv with Sigma, out = mu + U^T z with U^T U = Sigma + nugget I of the device's own mu and Sigma, within the
    bounds of tests/test_gpu_draw.py: with z = I the factor's backward error 4 (R + 2) 2^-53 sqrt(A_ii A_jj); the product
    (R + 2) 2^-53 |L||z|.  As there, a flux equal to the offset and prior means 0 make mu == 0 exactly, so that out IS the
    product; that the mean of the real flux is added with one rounding is asserted on its own."""
    import draw_reference as dr
    pc = tp.PCASES[3]              # N129-c2, mode 0, two dates: R = 130, the covariance between the dates in Sigma
    d = tr.case_data(tp.tv_case(pc))
    mode, lwls, pred, t_pred, _mus, gp, tau = _call(pc)
    zero = np.zeros(2)
    nugget = 1e-8
    with _handle(d, flux=1.0) as h:
        mu, Sigma = h.predict_tv(mode, lwls, pred, t_pred, zero, gp, tau)
        R = mu.shape[0]
        assert np.all(mu == 0.0)
        eye = h.predict_draw(R, z=np.eye(R), nugget=nugget)
        z = np.random.default_rng(91).standard_normal((5, R))
        prod = h.predict_draw(5, z=z, nugget=nugget)
    assert np.all(np.isfinite(eye)) and np.all(np.tril(eye, -1) == 0.0)
    A = Sigma.astype(LD) + LD(nugget) * np.eye(R, dtype=LD)
    L = eye.astype(LD).T
    dd = np.sqrt(np.diag(A))
    worst = float(np.max(np.abs(dr.gram(L) - A) / np.outer(dd, dd)) / (U53 * (R + 2)))
    print(f"factor: max |L L^T - A| / (sqrt(A_ii A_jj) (R + 2) 2^-53) = {worst:.3f} (bound 4)")
    assert np.all(np.diag(L) > 0) and worst <= 4.0
    scale = np.abs(z).astype(LD) @ np.abs(L).T
    worst = float(np.max(np.abs(prod.astype(LD) - z.astype(LD) @ L.T) / scale) / (U53 * (R + 2)))
    print(f"product: max |out - L z| / ((R + 2) 2^-53 |L||z|) = {worst:.3f} (bound 1)")
    assert worst <= 1.0
    # the covariance between the two dates is in Sigma: with tau = 2 span the same wavelength at both dates is correlated
    assert abs(Sigma[0, 33]) > 0.1 * Sigma[0, 0]
    with _handle(d) as h:
        mu_r, Sigma_r = h.predict_tv(mode, lwls, pred, t_pred, zero, gp, tau)
        assert _same_bits(Sigma_r, Sigma) and np.max(np.abs(mu_r)) > 1e-2
        assert _same_bits(h.predict_draw(5, z=z, nugget=nugget), prod + mu_r[None, :])


# ---- the Python forms -------------------------------------------------------------------------------------------------------------
def _chunk2d(s):
    from psoap_amd import data as pdata

    def full(v, fill):
        out = np.full(s.mask.shape, fill)
        out[s.mask] = v
        return out
    date = np.broadcast_to(s.dates[:, None], s.mask.shape).copy()
    return pdata.Chunk(np.exp(full(s.lwl, 8.5)), full(s.fl, 1.0), full(s.sigma, 1.0), date, s.mask.copy())


def test_python_layer():
    from psoap_amd import covariance, retrieve, synthetic as syn
    from psoap_amd.chunk import ChunkHandle
    from psoap_amd.utils import registered_params
    s = syn.make_chunk(2, 6, 24, seed=893, masked_fraction=0.1)
    p_orb = syn.make_orbit_proposals("SB2", 1, seed=894)[0]
    pars = dict(zip(registered_params["SB2"], list(p_orb) + list(syn.GP_BASE[2])))
    M = 2 * s.n_pix
    span = float(s.dates.max() - s.dates.min())
    tau = np.array([0.5 * span, np.inf])
    dates = np.array([s.dates.min() + 0.3 * span, s.dates[3]])
    res = retrieve.retrieve_components_at("SB2", _chunk2d(s), pars, tau, dates)
    assert res["Sigma"] is None and res["mu"].shape == (2 * 2 * M,) and np.array_equal(res["dates"], dates)
    for k in "fg":
        assert res["mu_" + k].shape == (2, M) and res["sigma_" + k].shape == (2, M)
    # the handle call, bit for bit
    lwls = res["lwls"]
    times = s.dates[s.epoch_index] - s.dates.min()
    t_pred = np.repeat(dates - s.dates.min(), M)
    pred = np.tile(res["lwl_predict"], (2, 2))
    with ChunkHandle(s.fl, s.sigma) as h:
        h.set_times(times)
        mu, var = h.predict_tv(0, lwls, pred, t_pred, [0.0, 0.0], list(syn.GP_BASE[2]), tau, want_sigma="diag")
        mu_S, Sigma = h.predict_tv(0, lwls, pred, t_pred, [0.0, 0.0], list(syn.GP_BASE[2]), tau)
        drawn = h.predict_draw(3, seed=7)
        singles = [h.predict_tv(0, lwls, pred[:, :M], t_pred[d * M:(d + 1) * M], [0.0, 0.0], list(syn.GP_BASE[2]), tau, want_sigma=False)
                   for d in range(2)]
    assert _same_bits(res["mu"], mu) and _same_bits(mu_S, mu)
    assert _same_bits(np.concatenate([res["sigma_f"].ravel(), res["sigma_g"].ravel()]), np.sqrt(var))
    assert _same_bits(res["mu_f"], mu[:2 * M].reshape(2, M)) and _same_bits(res["mu_g"], mu[2 * M:].reshape(2, M))
    # (n_dates, M): row d is the single-date call at dates[d] -- the same conditional mean from another column layout -- at the
    # parity bound
    for d in range(2):
        assert np.max(np.abs(res["mu_f"][d] - singles[d][:M])) <= TOL["mu"]
        assert np.max(np.abs(res["mu_g"][d] - singles[d][M:])) <= TOL["mu"]
    # covariance.predict_timevar takes the dates in the unit and from the origin of the times
    got = covariance.predict_timevar(lwls, s.fl, s.sigma, pred, np.repeat(dates, M), [0.0, 0.0], syn.GP_BASE[2], tau, s.dates[s.epoch_index])
    assert _same_bits(got[0], mu) and _same_bits(got[1], Sigma)
    full = retrieve.retrieve_components_at("SB2", _chunk2d(s), pars, tau, dates, get_Sigma=True, n_draws=3, seed=7)
    assert _same_bits(full["mu"], mu) and _same_bits(full["Sigma"], Sigma)
    assert full["f_draws"].shape == (3, 2, M) and full["g_draws"].shape == (3, 2, M)
    assert _same_bits(np.concatenate([full["f_draws"].reshape(3, -1), full["g_draws"].reshape(3, -1)], axis=1), drawn)
    assert _same_bits(full["sigma_f"], np.sqrt(np.diag(Sigma))[:2 * M].reshape(2, M))
    with pytest.raises(ValueError):
        retrieve.retrieve_components_at("SB2", _chunk2d(s), pars, tau, dates, n_draws=2)
    # the default of predict_draws is the static posterior, as before
    _mu0, _S0, d0 = covariance.predict_draws(lwls, s.fl, s.sigma, pred[:, :M], [0.0, 0.0], syn.GP_BASE[2], 2, 7)
    with ChunkHandle(s.fl, s.sigma) as h:
        h.predict(0, lwls, pred[:, :M], [0.0, 0.0], list(syn.GP_BASE[2]))
        assert _same_bits(d0, h.predict_draw(2, seed=7))
