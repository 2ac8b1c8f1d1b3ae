"""CPU checks of the references for the Fisher information and the leave-one-out under the time-variable kernel
(tests/timevar_fisher_reference.py) that tests/test_gpu_timevar_fisher.py is measured against, of the algebra of
``covariance.timevar_laplace``, of the pure-host refusals (psoap_amd/csrc/predict_plan.hpp: tv_analysis_check,
fisher_tv_check) and of the ctypes declarations of the two entries.

The time-scale column of K_t is checked against something that does not share its derivation: the central difference of
``timevar_reference.matrix_ext`` in tau_c.  A central difference is second order, so halving the step divides its discrepancy
from the analytic K_t by 4 (between 3 and 5 here, the margin tests/test_fisher_reference.py uses for l); a wrong term leaves a
discrepancy that does not fall.

The bound on F is the one the GPU test uses -- 8 x the largest error of the float64 twin against the long-double reference
(python tests/timevar_fisher_reference.py; the table is in tests/test_gpu_timevar_fisher.py) -- and six planted defects of K_t
or of the contraction show that it rejects a wrong formula.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fisher_reference as fr
import timevar_fisher_reference as tf
import timevar_reference as tr
from test_plan_host import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LD = np.longdouble
MARGIN = 8
TOL = {"F": MARGIN * 3.39e-14, "mu": MARGIN * 1.82e-15}        # tests/test_gpu_timevar_fisher.py: the table's last row


def _case(name):
    return next(c for c in tf.CASES if tf.case_id(c) == name)


def test_the_cases_are_timevar_references_without_n520():
    assert [tf.case_id(c) for c in tf.CASES] == ["N100-c2", "N128-c2", "N129-c2", "N300-c1", "N300-c2", "N300-c3", "N300-c2-perm"]
    for case in tf.CASES:
        tan_lwl, tan_gp, tan_tau = tf.case_tangents(case)
        c = case[1][1]
        assert tan_gp.shape == (3 * c + 3, 2 * c) and tan_tau.shape == (3 * c + 3, c) and tan_lwl.shape[0] == 3 * c + 3
        assert np.array_equal(tan_tau[2 * c:3 * c], np.eye(c)) and np.all(tan_lwl[:3 * c] == 0.0)
        assert all(np.max(np.abs(tan_lwl[t])) > 0 for t in range(3 * c, 3 * c + 3))


@pytest.mark.parametrize("case", tf.CASES, ids=tf.case_id)
def test_tau_column_of_the_tangent_matrix_is_the_derivative_of_matrix_ext(case):
    d = tf.case_data(case)
    c, N = d.lwls.shape
    for k in range(c):
        dtau = np.zeros(c)
        dtau[k] = 1.0
        Kt = tf.tangent_matrix_tv(d.lwls, d.times, d.gp, d.tau, np.zeros((c, N)), np.zeros(2 * c), dtau, _LD)
        assert np.array_equal(Kt, Kt.T)
        if not np.isfinite(d.tau[k]):
            assert np.all(Kt == 0)                     # tau = inf: K does not depend on it
            continue
        assert np.max(np.abs(Kt)) > 0

        def discrepancy(h):
            up, dn = d.tau.astype(_LD), d.tau.astype(_LD)
            up[k], dn[k] = up[k] + _LD(h), dn[k] - _LD(h)
            diff = (tr.matrix_ext(d.lwls, d.times, d.gp, up) - tr.matrix_ext(d.lwls, d.times, d.gp, dn)) / (_LD(2) * _LD(h))
            return float(np.max(np.abs(diff - Kt)))

        h = 0.02 * d.tau[k]
        e1, e2 = discrepancy(h), discrepancy(h / 2)
        print(f"{tf.case_id(case)} tau_{k}: max |K_t| {float(np.max(np.abs(Kt))):.3e}, discrepancy {e1:.3e} at h, {e2:.3e} at h/2, "
              f"ratio {e1 / e2:.3f}")
        assert 3.0 <= e1 / e2 <= 5.0, (k, e1, e2)


@pytest.mark.parametrize("case", tf.CASES, ids=tf.case_id)
def test_float64_twin_within_the_derived_bound_of_the_long_double_reference(case):
    d = tf.case_data(case)
    F, F_mu = tf.case_ext(case)
    f, f_mu = tf.fisher_tv_f64(d.lwls, d.times, d.sigma, d.gp, d.tau, *tf.case_tangents(case))
    err = {"F": tf.rel_to_scale(f, F), "mu": float(abs(_LD(f_mu) - F_mu) / F_mu)}
    print(f"{tf.case_id(case)}: " + ", ".join(f"{k} {v:.2e} (bound {TOL[k]:.2e})" for k, v in err.items()))
    assert err["F"] <= TOL["F"] and err["mu"] <= TOL["mu"]
    assert np.array_equal(F, F.T) and F_mu > 0
    c = d.lwls.shape[0]
    for k in range(c):                                 # the time scale of a static component carries no information
        assert (not np.isfinite(d.tau[k])) == bool(np.all(F[2 * c + k] == 0)) == bool(np.all(f[2 * c + k] == 0))


@pytest.mark.parametrize("name", ["N100-c2", "N129-c2", "N300-c3"])
def test_tau_inf_is_the_static_fisher_in_the_shared_entries(name):
    """with every tau = inf the covariance derivatives ARE ``fisher_reference.tangent_matrix``'s, F from the same K has the same
    bits whatever the time-scale tangents hold, and it agrees with ``fisher_reference.fisher_f64`` (whose K comes from the
    oracle's fill) within the bound"""
    case = _case(name)
    d = tf.case_data(case)
    c = d.lwls.shape[0]
    tan_lwl, tan_gp, tan_tau = tf.case_tangents(case)
    inf = np.full(c, np.inf)
    shared = [t for t in range(3 * c + 3) if not np.any(tan_tau[t])]
    for t in shared:
        assert np.array_equal(tf.tangent_matrix_tv(d.lwls, d.times, d.gp, inf, tan_lwl[t], tan_gp[t], tan_tau[t]),
                              fr.tangent_matrix(d.lwls, d.gp, tan_lwl[t], tan_gp[t]))
    f, f_mu = tf.fisher_tv_f64(d.lwls, d.times, d.sigma, d.gp, inf, tan_lwl, tan_gp, tan_tau)
    K = tr.matrix_f64(d.lwls, d.times, d.gp, inf, d.sigma)
    g, g_mu = fr.fisher_from_matrices(K, [fr.tangent_matrix(d.lwls, d.gp, tan_lwl[t], tan_gp[t]) for t in shared])
    assert np.array_equal(f[np.ix_(shared, shared)], g) and f_mu == g_mu
    assert np.all(f[2 * c:3 * c] == 0) and np.all(f[:, 2 * c:3 * c] == 0)
    s, s_mu = fr.fisher_f64(d.lwls, d.sigma, d.gp, tan_lwl[shared], tan_gp[shared])
    assert fr.rel_to_scale(g, s) <= TOL["F"] and abs(g_mu - s_mu) <= TOL["mu"] * s_mu


@pytest.mark.parametrize("defect", tf.DEFECTS)
def test_a_planted_defect_is_rejected_by_the_bound(defect):
    """N300-c2 (three tiles, tau = (inf, 0.25 span)): each wrong formula, put into the float64 twin, misses the bound the sound
    twin keeps"""
    case = _case("N300-c2")
    d = tf.case_data(case)
    F, _ = tf.case_ext(case)
    f, _ = tf.fisher_tv_f64(d.lwls, d.times, d.sigma, d.gp, d.tau, *tf.case_tangents(case), defect=defect)
    err = tf.rel_to_scale(f, F)
    print(f"{defect}: {err:.2e} (bound {TOL['F']:.2e})")
    assert err > TOL["F"]


def test_leave_one_out_twin_and_planted_variability():
    """the float64 leave-one-out against the long-double one on N129-c2, within 8 x the table of
    tests/test_gpu_timevar_fisher.py; at tau = inf it is ``loo_reference.loo_f64`` on the same K; and the planted drift: the epoch
    farthest in time from the others fits the time-variable model and not the static one"""
    import loo_reference as lr
    from test_gpu_timevar_fisher import LOO_TOL, PLANT_CPU
    case = _case("N129-c2")
    d = tf.case_data(case)
    ep, ne = tf.case_epochs(case)
    err = lr.errors(tf.loo_tv_f64(d.lwls, d.times, d.fl, d.sigma, d.gp, d.tau, tf.MU_GP, ep, ne), tf.case_loo_ext(case))
    assert all(err[k] <= LOO_TOL[k] for k in lr.OUTPUTS), err
    d, fl, tau, ep, ne, far = tf.planted()
    npix = np.bincount(ep, minlength=ne)
    tv = tf.loo_tv_f64(d.lwls, d.times, fl, d.sigma, d.gp, tau, tf.MU_GP, ep, ne).ep_chi2[far] / npix[far]
    st = lr.loo_f64(d.lwls, fl, d.sigma, d.gp, tf.MU_GP, ep, ne).ep_chi2[far] / npix[far]
    print(f"epoch {far}: chi2 / npix {tv:.4f} time-variable, {st:.4f} static")
    assert far == PLANT_CPU["epoch"] and abs(tv - PLANT_CPU["tv"]) < 5e-4 and abs(st - PLANT_CPU["static"]) < 5e-3
    assert 2 * abs(tv - 1) < abs(st - 1)              # a factor of two to spare


def test_timevar_laplace_algebra_on_the_float64_fisher():
    from psoap_amd.covariance import _laplace_from_fisher
    case = _case("N300-c3")                            # tau = (0.25 span, inf, 2 span)
    d = tf.case_data(case)
    c = 3
    eye = np.eye(3 * c)
    F, _ = tf.fisher_tv_f64(d.lwls, d.times, d.sigma, d.gp, d.tau, np.zeros((3 * c, c, d.lwls.shape[1])), eye[:, :2 * c],
                            eye[:, 2 * c:])
    free = np.isfinite(d.tau)
    cov, sd_gp, sd_tau = _laplace_from_fisher(F, d.gp, d.tau, free)
    idx = [0, 1, 2, 3, 4, 5, 6, 8]
    theta = np.concatenate([d.gp, d.tau])[idx]
    F_log = F[np.ix_(idx, idx)] * np.outer(theta, theta)        # the chain rule to log parameters, on the free ones
    assert cov.shape == (8, 8) and np.allclose(cov @ F_log, np.eye(8), rtol=0, atol=1e-8)
    assert np.allclose(sd_gp, d.gp * np.sqrt(np.diag(cov)[:6]), rtol=1e-14)
    assert np.isnan(sd_tau[1]) and np.allclose(sd_tau[[0, 2]], d.tau[[0, 2]] * np.sqrt(np.diag(cov)[6:]), rtol=1e-14)
    assert np.all(sd_gp > 0) and np.all(sd_tau[[0, 2]] > 0)
    # a tau held fixed: its row leaves, the others' standard deviations can only shrink
    cov2, sd_gp2, sd_tau2 = _laplace_from_fisher(F, d.gp, d.tau, [True, False, False])
    assert cov2.shape == (7, 7) and np.isnan(sd_tau2[1]) and np.isnan(sd_tau2[2])
    assert np.all(sd_gp2 <= sd_gp * (1 + 1e-12)) and sd_tau2[0] <= sd_tau[0] * (1 + 1e-12)
    # a free tau = inf has an exactly-zero row: singular; so has a NaN F
    with pytest.raises(ValueError):
        _laplace_from_fisher(F, d.gp, d.tau, [True, True, True])
    Z = F.copy()
    Z[6, :] = Z[:, 6] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        _laplace_from_fisher(Z, d.gp, d.tau, free)
    with pytest.raises(np.linalg.LinAlgError):
        _laplace_from_fisher(np.full((9, 9), np.nan), d.gp, d.tau, free)


EXPECTED_HOST = """fisher ok : ok
fisher T1 : ok
fisher T32 : ok
fisher T0 : the number of tangents must be between 1 and 32
fisher T33 : the number of tangents must be between 1 and 32
fisher no-arrays : bad arguments
fisher c0 : number of components must be 1, 2 or 3
fisher c4 : number of components must be 1, 2 or 3
fisher no-times : call psoap_chunk_set_times first
fisher open-stream : the handle has an open stream (psoap_stream_close first)
fisher baseline : the handle has a baseline (psoap_chunk_set_baseline): the time-variable kernel under the marginalised continuum is not built yet
loo ok : ok
loo no-arrays : bad arguments
loo c4 : number of components must be 1, 2 or 3
loo no-times : call psoap_chunk_set_times first
loo open-stream : the handle has an open stream (psoap_stream_close first)
loo baseline : the handle has a baseline (psoap_chunk_set_baseline): the time-variable kernel under the marginalised continuum is not built yet
"""


def test_pure_host_refusals(tmp_path):
    """no times, open stream, baseline, T out of range: tests/host/tv_analysis_host_check.cpp, a plain build of the header"""
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    exe = str(tmp_path / "tv_analysis_host_check")
    source = os.path.join(ROOT, "tests", "host", "tv_analysis_host_check.cpp")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], "-std=c++17", "-O1", "-Wall", "-Wextra", source, "-o", exe],
                        capture_output=True, text=True, cwd=str(tmp_path))
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stdout == EXPECTED_HOST


def test_ctypes_declarations_of_the_two_entries():
    from psoap_amd import _lib
    res, args = _lib.SIGNATURES["psoap_chunk_fisher_tv"]
    assert res is ctypes.c_int and len(args) == 11 and args[5] is ctypes.c_int and args.count(_lib._dp) == 8
    res, args = _lib.SIGNATURES["psoap_chunk_loo_tv"]
    assert res is ctypes.c_int and len(args) == 17 and args[5] is ctypes.c_double and args[7] is ctypes.c_int
    assert args[6] is _lib._i32p and args[16] is _lib._i32p
    header = open(os.path.join(ROOT, "include", "psoap_gp.h")).read()
    assert "int psoap_chunk_fisher_tv(" in header and "int psoap_chunk_loo_tv(" in header
    from psoap_amd.chunk import ChunkHandle
    from psoap_amd import covariance
    assert callable(ChunkHandle.fisher_tv) and callable(ChunkHandle.loo_tv)
    assert all(callable(getattr(covariance, n)) for n in ("fisher_information_timevar", "timevar_laplace", "loo_timevar"))
