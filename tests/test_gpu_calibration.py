"""GPU: the device calibration solve (two augmented Cholesky passes, psoap_amd/csrc/calibrate_kernels.hpp) against a
long-double reference, against vectors from the reference program and against the CPU oracle.

The cases of tests/calibration_reference.py -- the smallest shapes at which a fill, a padding row, a slab of the transposed
GEMV, a column of the augmented tile or the write of C' into the second pass's matrix can go wrong -- compared output by
output: fl_cor relative to max|fl_cor|, X relative to max|X|.

The tolerance is derived, not fitted: the float64 evaluation of the same formulas (the oracle's fills, SciPy's cho_factor /
cho_solve, numpy's Chebyshev) measured against the long-double one on these very cases (python tests/calibration_reference.py).
``grids``: the reference forms A, B, C in long double from the grids (the kernel form is held to it); ``blocks``: it takes
the float64 A, B, C the explicit form is given; ``static``: the problem optimize_calibration_static poses with a
one-component case's arrays (the Chebyshev abscissa serves as the kernel abscissa of the epoch too), from its grids -- another
problem with another conditioning, so with a row of its own.

    case                  grids:fl_cor       grids:X blocks:fl_cor      blocks:X static:fl_cor      static:X
    a-c1-M9-N9-o0             2.68e-16      2.49e-16      1.25e-16      1.04e-16      1.01e-15      9.66e-16
    b-c1-M128-N128-o15        2.20e-11      3.21e-12      2.20e-11      3.21e-12      4.59e-11      2.06e-11
    c-c2-M129-N258-o5         7.40e-13      1.38e-13      7.39e-13      1.37e-13             -             -
    d-c1-M127-N381-o8         2.16e-13      5.09e-14      2.16e-13      5.08e-14      2.28e-13      5.48e-14
    e-c2-M257-N257-o15        1.14e-11      3.62e-12      1.14e-11      3.62e-12             -             -
    f-c3-M200-N800-o2         3.00e-14      1.41e-14      3.00e-14      1.40e-14             -             -
    g-c2-M130-N60-o3          4.67e-12      3.67e-12      4.67e-12      3.67e-12             -             -
    h-c2-M140-N410-o4         1.56e-13      4.35e-14      1.58e-13      4.38e-14             -             -
    i-c1-M171-N513-o15        3.46e-13      4.22e-13      3.46e-13      4.22e-13      4.24e-13      3.67e-13
    max                       2.20e-11      3.67e-12      2.20e-11      3.67e-12      4.59e-11      2.06e-11
    cycle                     5.63e-14
    cycle_chunk               2.81e-14   (mapped abscissa against the host's u: 3.45e-14)

The device sums in another order and fuses multiply-adds but is fp64 throughout: it gets the ``max`` row times the project's
margin of 8 (tests/test_gpu_grad.py).  Nothing is fitted to the device's own results.  Where a comparison stays against
the float64 oracle or against the vectors the reference program recorded in float64, the bound is (8 + 1) times the row:
the device's error plus the oracle's own (measured on those cases too: at most 1.1e-12, inside the row).

One difference is inside the row on purpose.  The device and numpy map the abscissa as ``off + scl * x`` with |off| ~ 1e4,
which costs about 1e-12 in u and k^2 times that in T_k; the long-double reference evaluates u = (2 x - (a + b)) / (b - a).
That map is the reference program's definition, so the float64 evaluation carries it and so does the bound.

The cycles (five epochs of 90 pixels, two cycles, order 1: ten solves, each fed by the last) have rows of their own: the
float64 loop over the oracle against the long-double loop, times 8.  cycle_calibration_chunk re-evaluates the polynomial on
every pixel on the host with the other form of u; a float64 chunk cycle that uses the solve's mapped abscissa there instead
differs from it by 3.45e-14 of the flux, which is what that difference contributes.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import calibration_reference as cr  # noqa: E402

MARGIN = 8
F64 = {"grids": {"fl_cor": 2.20e-11, "X": 3.67e-12},
       "blocks": {"fl_cor": 2.20e-11, "X": 3.67e-12},
       "static": {"fl_cor": 4.59e-11, "X": 2.06e-11}}        # the table above, the max row
TOL = {lv: {k: MARGIN * v for k, v in row.items()} for lv, row in F64.items()}
TOL_ORACLE = {k: (MARGIN + 1) * v for k, v in F64["blocks"].items()}      # against a float64 evaluation: plus its own error
F64_CYCLE = {"cycle": 5.63e-14, "chunk": 2.81e-14}
TOL_CYCLE = {k: MARGIN * v for k, v in F64_CYCLE.items()}


@pytest.fixture(scope="module")
def ghost():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "golden_host_v1.npz")))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _components(cov, inp, order, mu=1.0):
    return cov.optimize_calibration_components(inp["lwl0"], inp["lwl1"], inp["lwl_cal"], inp["lwls_cal"], inp["fl_cal"],
                                               inp["sigma_cal"], inp["lwls_fixed"], inp["fl_fixed"], inp["sigma_fixed"],
                                               inp["gp"], order=order, mu_GP=mu)


def _explicit(cov, inp, blocks, order, mu=1.0):
    return cov.optimize_calibration(inp["lwl0"], inp["lwl1"], inp["lwl_cal"], inp["fl_cal"], inp["fl_fixed"], *blocks,
                                    order=order, mu_GP=mu)


def _static(cov, inp, order, mu=1.0):
    return cov.optimize_calibration_static(inp["lwl0"], inp["lwl1"], inp["lwl_cal"], inp["fl_cal"], inp["sigma_cal"],
                                           inp["lwls_fixed"][0], inp["fl_fixed"], inp["sigma_fixed"], inp["gp"][0],
                                           inp["gp"][1], order=order, mu_GP=mu)


def _stages(inp, got, ref, order, mu, blocks):
    """where the device leaves the reference, as far as the ABI shows it: the coefficients (everything up to the normal
    equations), the final D X on the host given the device's own X, and for scale what float64 loses at fl' and C'"""
    fl_cor, X = got
    D = np.asarray(inp["fl_cal"], dtype=np.longdouble)[:, None] * \
        cr.cheb_ext(cr.cheb_u_ext(inp["lwl0"], inp["lwl1"], inp["lwl_cal"]), order)
    top = np.max(np.abs(ref.fl_cor))
    f64 = cr.calibrate_f64_route(inp, order, mu, blocks=blocks)
    return {"X (fills, both passes, normal equations)": cr.errors(got, ref)["X"],
            "X per coefficient": [float(v) for v in np.abs(np.asarray(X, dtype=np.longdouble) - ref.X) / np.max(np.abs(ref.X))],
            "fl_cor": cr.errors(got, ref)["fl_cor"],
            "fl_cor against D_ref X_device (the last product alone)":
                float(np.max(np.abs(np.asarray(fl_cor, dtype=np.longdouble) - D @ np.asarray(X, dtype=np.longdouble))) / top),
            "pixel of the largest fl_cor error": int(np.argmax(np.abs(np.asarray(fl_cor, dtype=np.longdouble) - ref.fl_cor))),
            "float64 route at fl', C' and the outputs": {**cr.stage_errors(f64, ref), **cr.errors(f64, ref)}}


def _check(name, got, ref, tol, inp, order, mu=1.0, blocks=None):
    fl_cor, X = got
    assert fl_cor.shape == ref.fl_cor.shape and X.shape == (order + 1,) and fl_cor.dtype == X.dtype == np.float64, name
    assert np.all(np.isfinite(fl_cor)) and np.all(np.isfinite(X)), name
    err = cr.errors(got, ref)
    print(f"{name}: " + ", ".join(f"{k} {v:.2e} ({tol[k]:.2e})" for k, v in err.items()))
    for k, v in err.items():
        assert v <= tol[k], (name, k, v, tol[k], _stages(inp, got, ref, order, mu, blocks))


def _check_oracle(name, got, want, order):
    """against a float64 evaluation (the oracle, or the vectors the reference program recorded)"""
    err = cr.errors(got, cr.Cal(np.asarray(want[0], dtype=np.longdouble), np.asarray(want[1], dtype=np.longdouble)))
    print(f"{name}: " + ", ".join(f"{k} {v:.2e} ({TOL_ORACLE[k]:.2e})" for k, v in err.items()))
    assert got[1].shape == (order + 1,)
    for k, v in err.items():
        assert v <= TOL_ORACLE[k], (name, k, v, TOL_ORACLE[k])


# ---- every form against long double ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cr.CASES, ids=cr.case_id)
def test_calibration_against_long_double(case):
    from psoap_amd import covariance as cov
    inp, blocks = cr.case_inputs(case), cr.case_blocks(case)
    name = cr.case_id(case)
    # kernel form: blocks evaluated on the device, held to blocks formed in long double
    got = _components(cov, inp, case.order, case.mu)
    again = _components(cov, inp, case.order, case.mu)
    assert _same_bits(got[0], again[0]) and _same_bits(got[1], again[1])          # two calls, the same bits
    _check(name + " kernel", got, cr.case_ext(case, "grids"), TOL["grids"], inp, case.order, case.mu)
    # explicit form: held to the long-double solve from the very float64 A, B, C it was given
    got2 = _explicit(cov, inp, blocks, case.order, case.mu)
    again2 = _explicit(cov, inp, blocks, case.order, case.mu)
    assert _same_bits(got2[0], again2[0]) and _same_bits(got2[1], again2[1])
    _check(name + " explicit", got2, cr.case_ext(case, "blocks"), TOL["blocks"], inp, case.order, case.mu, blocks)
    if case.c == 1:
        st = cr.static_inputs(inp)
        gs = _static(cov, inp, case.order, case.mu)
        again_s = _static(cov, inp, case.order, case.mu)
        assert _same_bits(gs[0], again_s[0]) and _same_bits(gs[1], again_s[1])
        _check(name + " static", gs, cr.static_ext(case), TOL["static"], st, case.order, case.mu)


def test_device_calibration_matches_reference(ghost, oracle):
    from psoap_amd import covariance as cov
    from test_calibration_oracle import cal_cases
    for name, c, order, case in cal_cases():
        # kernel form: blocks evaluated on the device
        got = _components(cov, case, order)
        _check_oracle(name + " kernel", got, (ghost[f"cal_{name}_fl"], ghost[f"cal_{name}_X"]), order)
        # explicit form: the reference's signature, caller-filled A, B, C
        blocks = oracle.calibration_blocks(case["lwls_cal"], case["sigma_cal"], case["lwls_fixed"], case["sigma_fixed"],
                                           case["gp"])
        got2 = _explicit(cov, case, blocks, order)
        _check_oracle(name + " explicit", got2, (ghost[f"cal_{name}_fl"], ghost[f"cal_{name}_X"]), order)
        if c == 1:
            gs = _static(cov, case, order)
            _check_oracle(name + " static", gs, (ghost[f"cal_{name}_static_fl"], ghost[f"cal_{name}_static_X"]), order)


def test_calibration_mu_and_larger_problem(oracle):
    from psoap_amd import covariance as cov
    from make_golden_host import cal_case
    case = cal_case(syn, 3, 6, 400, 960, 0.05, 0.9, limit_array=4)        # M ~ 380, N ~ 1520: several tiles
    A, B, C = oracle.calibration_blocks(case["lwls_cal"], case["sigma_cal"], case["lwls_fixed"], case["sigma_fixed"],
                                        case["gp"])
    for order, mu in ((1, 1.0), (4, 0.97)):
        want = oracle.optimize_calibration(case["lwl0"], case["lwl1"], case["lwl_cal"], case["fl_cal"], case["fl_fixed"],
                                           A, B, C, order=order, mu_GP=mu)
        _check_oracle(f"order {order} mu {mu}", _components(cov, case, order, mu), want, order)


@pytest.mark.parametrize("c,ne,npx,order,limit,seed", [
    (1, 2, 9, 0, 1, 971),        # M = 9, N = 9: everything below one tile, constant correction
    (2, 3, 129, 5, 2, 972),      # M = 129 (one past a tile edge), order 5
    (3, 5, 200, 2, 4, 973),      # N = 800, three components
])
def test_calibration_edge_shapes_vs_oracle(oracle, c, ne, npx, order, limit, seed):
    from psoap_amd import covariance as cov
    from make_golden_host import cal_case
    case = cal_case(syn, c, ne, npx, seed, 0.0, 1.04, limit_array=limit)
    A, B, C = oracle.calibration_blocks(case["lwls_cal"], case["sigma_cal"], case["lwls_fixed"], case["sigma_fixed"],
                                        case["gp"])
    want = oracle.optimize_calibration(case["lwl0"], case["lwl1"], case["lwl_cal"], case["fl_cal"], case["fl_fixed"], A, B, C,
                                       order=order)
    _check_oracle("kernel", _components(cov, case, order), want, order)
    _check_oracle("explicit", _explicit(cov, case, (A, B, C), order), want, order)


# ---- refusals and status codes -------------------------------------------------------------------------------------------
def test_calibration_failure_raises():
    from psoap_amd import covariance as cov
    M, N = 40, 90
    rng = np.random.RandomState(0)
    lwl = np.sort(rng.uniform(8.5, 8.501, M))
    B = np.eye(N)
    B[3, 3] = -1.0                                        # not positive definite
    with pytest.raises(np.linalg.LinAlgError):
        cov.optimize_calibration(8.5, 8.501, lwl, np.ones(M), np.ones(N), np.eye(M), B, np.zeros((M, N)))
    with pytest.raises(np.linalg.LinAlgError):            # C' = A - C B^-1 C^T indefinite
        cov.optimize_calibration(8.5, 8.501, lwl, np.ones(M), np.ones(N), -np.eye(M), np.eye(N), np.zeros((M, N)))
    from psoap_amd._lib import PsoapError
    with pytest.raises(PsoapError):
        cov.optimize_calibration(8.5, 8.501, lwl, np.ones(M), np.ones(N), np.eye(M), np.eye(N), np.zeros((M, N)), order=40)


def _raw_explicit(inp, blocks, order, fl_cal=None, mu=1.0):
    from psoap_amd import _lib
    M, N = inp["lwl_cal"].shape[0], inp["fl_fixed"].shape[0]
    arrs = [_lib.as_f64(a) for a in (inp["lwl_cal"], inp["fl_cal"] if fl_cal is None else fl_cal, inp["fl_fixed"], *blocks)]
    fl_cor, X, status = np.empty(M), np.empty(order + 1), ctypes.c_int(-1)
    rc = _lib.load().psoap_calibrate_explicit(_lib.default_device(), M, N, order, float(inp["lwl0"]), float(inp["lwl1"]),
                                              *[_lib.dptr(a) for a in arrs], float(mu), _lib.dptr(fl_cor), _lib.dptr(X),
                                              ctypes.byref(status))
    return rc, status.value


def _raw_kernel(inp, order, fl_cal=None, mu=1.0):
    from psoap_amd import _lib
    c, M = inp["lwls_cal"].shape
    N = inp["fl_fixed"].shape[0]
    arrs = [_lib.as_f64(a) for a in (inp["lwl_cal"], inp["lwls_cal"], inp["fl_cal"] if fl_cal is None else fl_cal,
                                     inp["sigma_cal"], inp["lwls_fixed"], inp["fl_fixed"], inp["sigma_fixed"], inp["gp"])]
    fl_cor, X, status = np.empty(M), np.empty(order + 1), ctypes.c_int(-1)
    rc = _lib.load().psoap_calibrate(_lib.default_device(), c, M, N, order, float(inp["lwl0"]), float(inp["lwl1"]),
                                     *[_lib.dptr(a) for a in arrs], float(mu), _lib.dptr(fl_cor), _lib.dptr(X),
                                     ctypes.byref(status))
    return rc, status.value


def test_calibration_status_2_and_3_then_a_good_call():
    """C' not positive definite (A = -I) and normal equations not positive definite (fl_cal = 0: the design matrix, and
    with it D^T C'^-1 D, is exactly zero, so the first pivot fails ``d > 0`` with no rounding involved): status through the
    raw ABI with a zero return, LinAlgError from the wrappers, and the next well-posed call on the device unaffected"""
    from psoap_amd import covariance as cov
    case = cr.case_named("c")
    inp, blocks, order = cr.case_inputs(case), cr.case_blocks(case), case.order
    A, B, C = blocks
    before = _explicit(cov, inp, blocks, order)
    before_k = _components(cov, inp, order)

    def good(tag):
        after, after_k = _explicit(cov, inp, blocks, order), _components(cov, inp, order)
        assert _same_bits(after[0], before[0]) and _same_bits(after[1], before[1]), tag
        assert _same_bits(after_k[0], before_k[0]) and _same_bits(after_k[1], before_k[1]), tag
        _check(tag + ": explicit after", after, cr.case_ext(case, "blocks"), TOL["blocks"], inp, order, 1.0, blocks)
        _check(tag + ": kernel after", after_k, cr.case_ext(case, "grids"), TOL["grids"], inp, order)

    minus = (-np.eye(case.M), B, C)
    assert _raw_explicit(inp, minus, order) == (0, 2)
    with pytest.raises(np.linalg.LinAlgError):
        _explicit(cov, inp, minus, order)
    good("status 2")
    zeros = np.zeros(case.M)
    assert _raw_explicit(inp, blocks, order, fl_cal=zeros) == (0, 3)
    good("status 3 explicit")
    assert _raw_kernel(inp, order, fl_cal=zeros) == (0, 3)
    good("status 3 kernel")
    dead = dict(inp, fl_cal=zeros)
    with pytest.raises(np.linalg.LinAlgError):
        _explicit(cov, dead, blocks, order)
    with pytest.raises(np.linalg.LinAlgError):
        _components(cov, dead, order)
    with pytest.raises(np.linalg.LinAlgError):
        _static(cov, dict(cr.static_inputs(cr.case_inputs(cr.case_named("a"))), fl_cal=np.zeros(9)), 0)
    good("after the wrappers raised")


def test_calibration_order_and_domain_bounds():
    """order 15 is the highest accepted (cases b, e, i run it against the reference); 16, -1 and an empty or reversed
    domain are refused before anything is launched"""
    from psoap_amd import covariance as cov
    from psoap_amd._lib import PsoapError
    case = cr.case_named("a")
    inp, blocks = cr.case_inputs(case), cr.case_blocks(case)
    assert max(c.order for c in cr.CASES) == 15
    for order in (16, -1):
        with pytest.raises(PsoapError):
            _components(cov, inp, order)
        with pytest.raises(PsoapError):
            _explicit(cov, inp, blocks, order)
    for lwl0, lwl1 in ((inp["lwl1"], inp["lwl0"]), (inp["lwl0"], inp["lwl0"])):
        bad = dict(inp, lwl0=lwl0, lwl1=lwl1)
        with pytest.raises(PsoapError):
            _components(cov, bad, 0)
        with pytest.raises(PsoapError):
            _explicit(cov, bad, blocks, 0)
    _check("after the refusals", _components(cov, inp, case.order), cr.case_ext(case, "grids"), TOL["grids"], inp, case.order)


# ---- the cycles -------------------------------------------------------------------------------------------------------------
def test_cycle_calibration_pulls_epochs_together():
    from psoap_amd import covariance as cov
    from psoap_amd import data as pdata
    lwl, fl, sigma, mask, truth = (a.copy() for a in cr.cycle_case())
    ref, ref_chunk = cr.cycle_refs()
    args = (*cr.CYCLE_GP, cr.CYCLE_N)
    kw = dict(order=cr.CYCLE_ORDER, limit_array=cr.CYCLE_LIMIT)
    out = cov.cycle_calibration(lwl, fl, sigma, *args, **kw)
    spread_before = np.std(fl / truth, axis=0).mean()
    spread_after = np.std(out / truth, axis=0).mean()
    assert out.shape == fl.shape and spread_after < 0.25 * spread_before
    err = cr.cycle_error(out, ref)
    print(f"cycle: {err:.2e} ({TOL_CYCLE['cycle']:.2e})")
    assert np.all(np.isfinite(out)) and err <= TOL_CYCLE["cycle"], (err, TOL_CYCLE["cycle"])
    assert _same_bits(out, cov.cycle_calibration(lwl, fl, sigma, *args, **kw))
    # mask-aware chunk form: masked pixels are corrected with the fitted polynomial too
    ch = pdata.Chunk(lwl.copy(), fl.copy(), sigma.copy(), np.zeros_like(fl), mask)
    ch.lwl = None
    cov.cycle_calibration_chunk(ch, *args, **kw)
    assert np.std(ch.fl / truth, axis=0).mean() < 0.25 * spread_before
    err = cr.cycle_error(ch.fl, ref_chunk)
    print(f"cycle_chunk: {err:.2e} ({TOL_CYCLE['chunk']:.2e})")
    assert ch.fl.shape == fl.shape and np.all(np.isfinite(ch.fl)) and err <= TOL_CYCLE["chunk"], (err, TOL_CYCLE["chunk"])


def test_optimize_GP_f_matches_oracle_driven_fit(oracle):
    """Same Nelder-Mead driver (covariance.py:405-422) on the device likelihood and on the oracle likelihood."""
    from scipy.optimize import minimize
    from psoap_amd import covariance as cov
    ch = syn.make_chunk(1, 3, 80, seed=321)               # N = 240
    got = cov.optimize_GP_f(ch.lwls[0], ch.fl, ch.sigma, 0.3, 8.0)
    want = minimize(lambda x: -oracle.lnlike(ch.lwls, ch.fl, ch.sigma, [x[0], x[1]]), np.array([0.3, 8.0]),
                    method="Nelder-Mead")["x"]
    assert np.allclose(got, want, rtol=1e-5)
    assert cov.lnlike_f(None, ch.lwls[0], ch.fl, ch.sigma, *got) >= cov.lnlike_f(None, ch.lwls[0], ch.fl, ch.sigma, 0.3, 8.0)
