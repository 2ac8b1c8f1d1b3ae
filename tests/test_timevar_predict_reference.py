"""CPU checks of the references for the component spectra at a date (tests/timevar_predict_reference.py): the long-double
evaluation against the oracle's static predict at tau = inf and against the conditional read off the inverse of the joint
covariance of data and prediction at finite tau; the float64 twin inside the bound the GPU test derives from it; six seeded
defects of the cross and prior fills, each rejected by that bound; and the boundary -- both entry points declared in
include/psoap_gp.h, bound in psoap_amd._lib.SIGNATURES with the declared argument lists, exported and reachable from Python."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import timevar_predict_reference as tp
import timevar_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LD = np.longdouble
NAMES = ("psoap_chunk_predict_tv", "psoap_chunk_predict_tv_var")
MARGIN = 8


def test_the_cases_are_those_of_the_likelihood_and_cross_the_tile_edges():
    ids = {tr.case_id(c) for c in tr.CASES}
    assert all(pc[0] in ids for pc in tp.PCASES) and len(tp.PCASES) == 7
    shapes = []
    for pc in tp.PCASES:
        mode, lwls, _t, _fl, _s, pred, t_pred, mus, _gp, tau = tp.pcase_args(pc)
        c, N = lwls.shape
        assert pred.shape == (c, pc[2]) and t_pred.shape == (pc[2],) and np.all(np.isfinite(t_pred))
        assert np.any(np.isfinite(tau)), "every case has a component with a finite tau"
        shapes.append((N, c * pc[2] if mode == 0 else pc[2], len(set(t_pred.tolist()))))
    assert shapes == [(100, 100, 1), (100, 130, 1), (300, 129, 1), (129, 130, 2), (300, 129, 1), (300, 200, 2), (520, 128, 2)]
    assert np.count_nonzero(tp.pcase_pred(tp.PCASES[3])[1] == tp.pcase_dates(tp.PCASES[3])[0]) == 33
    # the permuted case's times are in no epoch order; the one beyond the span lies a span behind the last epoch
    assert np.any(np.diff(tr.case_data(tp.tv_case(tp.PCASES[5])).times) < 0)
    d = tr.case_data(tp.tv_case(tp.PCASES[4]))
    assert tp.pcase_dates(tp.PCASES[4])[0] == 2.0 * d.span


@pytest.mark.parametrize("pc", tp.PCASES, ids=tp.pcase_id)
def test_static_limit_is_the_oracles_predict(pc):
    """tau = inf: q = -0, the added term is -0 and every argument keeps its bits -- the long-double evaluation IS
    oracle.predict_ext, whatever the dates"""
    import oracle
    mode, lwls, times, fl, sigma, pred, t_pred, mus, gp, tau = tp.pcase_args(pc, tau=np.full(tp.tv_case(pc)[1][1], np.inf))
    got = tp.tv_predict_ext(mode, lwls, times, fl, sigma, pred, t_pred, mus, gp, tau)
    mu, Sigma = oracle.predict_ext(mode, lwls, fl, sigma, pred, mus, gp)
    assert np.array_equal(got.mu, mu) and np.array_equal(got.Sigma, Sigma)


def _joint_case(c, mode):
    """a small problem whose joint covariance of data and prediction is well conditioned: 48 pixels of an N100-c2 / N300-c1
    chunk, 6 prediction points per date a length scale and a half apart, two dates"""
    d = tr.case_data(tp.tv_case(("N100-c2",) if c == 2 else ("N300-c1",)))
    keep = slice(0, 48)
    lwls, times = d.lwls[:, keep], d.times[keep]
    step = 1.5 * max(d.gp[1::2]) / tr.C_KMS
    grid = np.min(lwls[0]) + step * np.arange(6)
    pred = np.tile(np.concatenate([grid, grid + 0.3 * step]), (c, 1))
    t_pred = np.concatenate([np.full(6, 0.3 * d.span), np.full(6, 0.8 * d.span)])
    mus = np.array([0.3, 0.2][:c]) if mode == 0 else np.array([tr.MU_GP])
    tau = np.array([0.25, 2.0][:c]) * d.span
    return mode, lwls, times, d.fl[keep], d.sigma[keep], pred, t_pred, mus, d.gp, tau


@pytest.mark.parametrize("c,mode", [(2, 0), (2, 1), (1, 2)])
def test_finite_tau_is_the_conditional_of_the_joint_gaussian(c, mode):
    """[fl; f*] ~ N([offset; m0], J), J = [[K, Ct], [Ct^T, A]].  With P = J^-1: Sigma = P_pp^-1, mu = m0 - P_pp^-1 P_pd r -- no
    Schur complement, no solve with K alone"""
    import oracle
    args = _joint_case(c, mode)
    mode, lwls, times, fl, sigma, pred, t_pred, mus, gp, tau = args
    ref = tp.tv_predict_ext(*args)
    Ct, A, m0, offset = tp.pieces(_LD, mode, lwls, times, pred, t_pred, mus, gp, tau)
    K = tp.data_cov_ext(lwls, times, sigma, gp, tau)
    N, R = Ct.shape
    J = np.block([[K, Ct], [Ct.T, A]])
    Li = oracle._fsolve_ext(oracle._chol_ext(J), np.eye(N + R, dtype=_LD))
    P = Li.T @ Li
    Lp = oracle._chol_ext(P[N:, N:])
    Lpi = oracle._fsolve_ext(Lp, np.eye(R, dtype=_LD))
    Sigma = Lpi.T @ Lpi
    mu = m0 - Sigma @ (P[N:, :N] @ (np.asarray(fl, dtype=_LD) - offset))
    cond = float(np.linalg.cond(np.asarray(J, dtype=np.float64)))
    eps = float(np.finfo(_LD).eps)
    unit = float(ref.prior_max)
    print(f"c {c} mode {mode}: cond(J) {cond:.2e}")
    # two inversions in long double: a few cond(J) eps, in the units of the outputs
    assert cond < 1e9
    assert float(np.max(np.abs(mu - ref.mu))) <= 64 * cond * eps * float(np.max(np.abs(fl)))
    assert float(np.max(np.abs(Sigma - ref.Sigma))) <= 64 * cond * eps * unit


# the float64 twin against the long-double evaluation on the cases (python tests/timevar_predict_reference.py, last row)
F64 = {"mu": 7.78e-15, "Sigma": 2.80e-15, "var": 1.36e-15}


def test_the_table_of_the_gpu_test_is_the_measured_one():
    import test_gpu_timevar_predict as gpu
    rows = tp.measure_f64()
    worst = {k: max(r[1][k] for r in rows) for k in tp.OUTPUTS}
    print(worst)
    for k in tp.OUTPUTS:
        assert gpu.F64[k] == F64[k] and gpu.MARGIN == MARGIN
        # another BLAS rounds otherwise, so not to the digit: the recorded row is neither stale nor generous
        # (the convention of tests/test_calibration_reference.py)
        assert F64[k] / MARGIN <= worst[k] <= MARGIN * F64[k], (k, worst[k], F64[k])


@pytest.mark.parametrize("defect", tp.DEFECTS)
def test_seeded_defects_are_rejected(defect):
    """each fault a fill kernel or its host step can have, seeded into the long-double evaluation of the three-component case
    (tau = 0.25 span, inf, 2 span; the date a span beyond the last epoch) and of the two-date case (one date hides a missing
    factor in A, an infinite tau hides the dates of its block): the bound of the GPU test rejects it in one of the two"""
    caught = False
    for pc in (tp.PCASES[4], tp.PCASES[3]):
        bad = tp.tv_predict_ext(*tp.pcase_args(pc), defect=defect, L=tp.pcase_factor(pc))
        with np.errstate(over="ignore", invalid="ignore"):
            err = tp.errors(bad.mu, bad.Sigma, bad.var, tp.pcase_ext(pc))
        print(defect, tp.pcase_id(pc), err)
        caught = caught or any(not (err[k] <= MARGIN * F64[k]) for k in tp.OUTPUTS)
    assert caught, defect


def test_an_out_of_reach_date_has_arguments_below_the_underflow():
    """rule 2's premise on the twin: N300-c1 with tau = 0.25 span and a date far out -- every argument of the cross block is
    <= -746, where the device's exp() is exactly +0"""
    pc = tp.PCASES[2]
    d = tr.case_data(tp.tv_case(pc))
    far = float(np.max(d.times) + np.sqrt(2 * 746.0) * np.max(d.tau[np.isfinite(d.tau)]) * 1.01)
    mode, lwls, times, fl, sigma, pred, t_pred, mus, gp, tau = tp.pcase_args(pc, dates=[far])
    assert np.all(tp.cross_args_f64(lwls, times, pred, t_pred, gp, tau) <= -746.0)
    f = tp.tv_predict_f64(mode, lwls, times, fl, sigma, pred, t_pred, mus, gp, tau)
    _Ct, A, m0, _off = tp.pieces(np.float64, mode, lwls, times, pred, t_pred, mus, gp, tau)
    assert np.array_equal(f.mu, m0) and np.array_equal(f.Sigma, A) and np.all(f.var == gp[0] * gp[0])


# ---- the boundary -------------------------------------------------------------------------------------------------------
def _declaration(name):
    text = open(os.path.join(ROOT, "include", "psoap_gp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/psoap_gp.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entry_points_are_declared_bound_and_exported():
    from psoap_amd import _lib, build
    L = ctypes.CDLL(build.build())
    dp, vp = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
    as_ctype = {"psoap_chunk *": vp, "int": ctypes.c_int, "const double *": dp, "double *": dp, "int *": ctypes.POINTER(ctypes.c_int)}
    for name in NAMES:
        args = _declaration(name)
        assert hasattr(L, name), f"{name} is not exported by libpsoap_gp.so"
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        assert [as_ctype[re.sub(r"\s*\w+$", "", a).strip()] for a in args] == list(argtypes), (name, args)
        assert len(args) == 13
        assert [a.split()[-1].lstrip("*") for a in args][:10] == ["h", "mode", "c", "M", "lwl", "lwl_pred", "t_pred", "mu_c", "gp", "tau"]


def test_python_surface_exists():
    from psoap_amd import covariance, retrieve
    from psoap_amd.chunk import ChunkHandle
    assert list(inspect.signature(ChunkHandle.predict_tv).parameters) == ["self", "mode", "lwls", "lwls_predict", "t_predict", "mu_c",
                                                                           "gp", "tau", "want_sigma"]
    assert list(inspect.signature(covariance.predict_timevar).parameters) == ["lwls", "fl", "sigma", "lwls_predict", "t_predict", "mus",
                                                                               "gp", "tau", "times", "mode", "want_sigma"]
    sig = inspect.signature(covariance.predict_draws)
    assert "timevar" in sig.parameters and sig.parameters["timevar"].default is None
    sig = inspect.signature(retrieve.retrieve_components_at)
    assert list(sig.parameters) == ["model", "chunk", "parameters", "tau", "dates", "n_pix_predict", "get_Sigma", "n_draws", "seed",
                                    "nugget"]
    assert (sig.parameters["get_Sigma"].default, sig.parameters["n_draws"].default, sig.parameters["nugget"].default) == ("diag", 0, 1e-8)


def test_refusals_that_need_no_device():
    from psoap_amd import _lib
    L = _lib.load()
    x = np.zeros(4)
    p = _lib.dptr(x)
    st = ctypes.c_int(0)
    assert L.psoap_chunk_predict_tv(None, 0, 2, 2, p, p, p, p, p, p, p, None, ctypes.byref(st)) != 0
    assert L.psoap_last_error() == b"psoap_chunk_predict_tv: bad arguments"
    assert L.psoap_chunk_predict_tv_var(None, 0, 2, 2, p, p, p, p, p, p, p, None, ctypes.byref(st)) != 0
    assert L.psoap_last_error() == b"psoap_chunk_predict_tv_var: var_out is required"
