"""CPU: the long-double calibration reference (tests/calibration_reference.py) is right, and the bound derived from it bites.

The reference against the vectors the reference program recorded; the float64 evaluation against it within the bound of
tests/test_gpu_calibration.py on every case; and eight seeded defects, each applied to the float64 evaluation, each of which
has to leave the bound on a case it applies to -- by the measure and the bound the device is held to, not by any digit.
"""
import os

import numpy as np
import pytest

import calibration_reference as cr
from test_calibration_oracle import CAL_RTOL, cal_cases, close
from test_gpu_calibration import F64, F64_CYCLE, MARGIN, TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ghost():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "golden_host_v1.npz")))


def _within(err, tol):
    return all(err[k] <= tol[k] for k in cr.OUTPUTS)


def test_reference_matches_recorded_vectors(ghost):
    seen = 0
    for name, c, order, case in cal_cases():
        ref = cr.calibrate_ext(case, order)
        assert ref.fl_cor.dtype == np.longdouble and ref.X.shape == (order + 1,)
        assert close(ref.fl_cor, ghost[f"cal_{name}_fl"], CAL_RTOL) and close(ref.X, ghost[f"cal_{name}_X"], CAL_RTOL), name
        # from the float64 blocks the explicit form is handed: the same solve
        blk = cr.calibrate_ext(case, order, blocks=cr.blocks_f64(case))
        assert close(blk.fl_cor, ghost[f"cal_{name}_fl"], CAL_RTOL) and close(blk.X, ghost[f"cal_{name}_X"], CAL_RTOL), name
        if c == 1:
            st = cr.calibrate_ext(cr.static_inputs(case), order)
            assert close(st.fl_cor, ghost[f"cal_{name}_static_fl"], CAL_RTOL), name
            assert close(st.X, ghost[f"cal_{name}_static_X"], CAL_RTOL), name
        seen += 1
    assert seen == 4


def test_case_table_reaches_what_it_names():
    by = {c.name: c for c in cr.CASES}
    assert [c.name for c in cr.CASES] == list("abcdefghi")
    for case in cr.CASES:
        inp = cr.case_inputs(case)
        assert inp["lwls_cal"].shape == (case.c, case.M) and inp["lwls_fixed"].shape == (case.c, case.N)
        assert inp["lwl0"] <= inp["lwl_cal"].min() and inp["lwl_cal"].max() <= inp["lwl1"]
    pad = lambda n, to: -(-n // to) * to                                          # noqa: E731
    assert (by["b"].M, by["b"].N, by["b"].order) == (128, 128, 15)
    assert by["d"].M == 127 and by["d"].mu != 1.0
    assert pad(by["e"].M, cr.NB) // cr.NB == 3 and pad(by["e"].N, cr.NB) == 384 and by["e"].order == 15
    assert by["g"].M > by["g"].N and pad(by["g"].M, cr.NB) // cr.NB > pad(by["g"].N, cr.NB) // cr.NB and by["g"].mu != 1.0
    assert pad(by["i"].N, cr.NB) == 640 and by["i"].order == 15
    assert by["h"].M % cr.NB and by["h"].N % cr.NB and by["h"].masked_fraction > 0
    assert {c.c for c in cr.CASES} == {1, 2, 3}


@pytest.mark.parametrize("case", cr.CASES, ids=cr.case_id)
def test_float64_evaluation_within_the_derived_bound(case):
    """by construction (F64 is the largest of these figures); it keeps the recorded table honest when a case is edited"""
    inp = cr.case_inputs(case)
    f = cr.calibrate_f64(inp, case.order, case.mu)
    route = cr.calibrate_f64_route(inp, case.order, case.mu)
    for level in cr.LEVELS:
        ref = cr.case_ext(case, level)
        err = cr.errors(f, ref)
        assert _within(err, TOL[level]), (level, err)
        assert _within(cr.errors(route, ref), TOL[level]), (level, cr.errors(route, ref), cr.stage_errors(route, ref))
    assert err["fl_cor"] < 1e-9                                                   # a case worse than this is badly conditioned
    if case.c == 1:
        st = cr.static_inputs(inp)
        assert _within(cr.errors(cr.calibrate_f64(st, case.order, case.mu), cr.static_ext(case)), TOL["static"])
        assert _within(cr.errors(cr.calibrate_f64_route(st, case.order, case.mu), cr.static_ext(case)), TOL["static"])


def test_recorded_maxima_are_current():
    rows = cr.measure_f64()
    for level in cr.LEVELS + ("static",):
        for k in cr.OUTPUTS:
            top = cr.max_row(rows, level)[k]
            # another BLAS rounds otherwise, so not to the digit: the recorded row is neither stale nor generous
            assert F64[level][k] / MARGIN <= top <= MARGIN * F64[level][k], (level, k, top, F64[level][k])
    assert MARGIN == 8


def test_cycle_twins_within_their_bound():
    cyc = cr.measure_cycles()
    for k in ("cycle", "chunk"):
        assert F64_CYCLE[k] / MARGIN <= cyc[k] <= MARGIN * F64_CYCLE[k], (k, cyc[k], F64_CYCLE[k])
    # the polynomial on the solve's mapped abscissa instead of the host's u: inside the chunk cycle's bound
    assert cyc["chunk_map"] <= MARGIN * F64_CYCLE["chunk"]
    lwl, fl, sigma, mask, truth = cr.cycle_case()
    ref, ref_chunk = cr.cycle_refs()
    before = np.std(fl / truth, axis=0).mean()
    assert np.std(np.asarray(ref, dtype=np.float64) / truth, axis=0).mean() < 0.25 * before
    assert np.std(np.asarray(ref_chunk, dtype=np.float64) / truth, axis=0).mean() < 0.25 * before
    assert 0.05 < 1.0 - mask.mean() < 0.15


# ---- seeded defects ----------------------------------------------------------------------------------------------------
def _with(inp, **kw):
    out = dict(inp)
    out.update(kw)
    return out


def _no_sigma_cal(case, inp):
    A, B, C = cr.blocks_f64(inp)
    A = A.copy()
    A[np.diag_indices_from(A)] -= inp["sigma_cal"] ** 2
    return cr.calibrate_f64_route(inp, case.order, case.mu, blocks=(A, B, C))


def _mu_one(case, inp):
    return cr.calibrate_f64_route(inp, case.order, 1.0)


def _domain_of_the_epoch(case, inp):
    return cr.calibrate_f64_route(_with(inp, lwl0=float(inp["lwl_cal"].min()), lwl1=float(inp["lwl_cal"].max())), case.order,
                                  case.mu)


def _last_column_without_2(case, inp):
    D = cr.design_f64(inp["lwl0"], inp["lwl1"], inp["lwl_cal"], inp["fl_cal"], case.order, last_factor=1.0)
    return cr.calibrate_f64_route(inp, case.order, case.mu, D=D)


def _last_block_row_of_B(case, inp):
    return cr.calibrate_f64_route(inp, case.order, case.mu, cbc_rows=cr.NB * (case.N // cr.NB))


def _last_gemv_slab(case, inp):
    return cr.calibrate_f64_route(inp, case.order, case.mu, flp_rows=cr.SLAB * ((case.N - 1) // cr.SLAB))


def _last_pixel_not_in_D(case, inp):
    D = cr.design_f64(inp["lwl0"], inp["lwl1"], inp["lwl_cal"], inp["fl_cal"], case.order)
    D[case.M - 1] = 0.0
    return cr.calibrate_f64_route(inp, case.order, case.mu, D=D)


def _C_untransposed(case, inp):
    A, B, C = cr.blocks_f64(inp)
    return cr.calibrate_f64_route(inp, case.order, case.mu, blocks=(A, B, np.ascontiguousarray(C.T)))


# name -> (the defect, the cases it applies to and why the others do not)
DEFECTS = {
    "sigma_cal^2 left off A's diagonal": (_no_sigma_cal, "abcdefghi"),
    "mu = 1 where the case has another": (_mu_one, "dg"),                        # the cases with mu != 1
    "Chebyshev domain from lwl_cal itself": (_domain_of_the_epoch, "bcdefghi"),  # order 0 has no abscissa
    "highest column without the factor 2": (_last_column_without_2, "bcdefghi"),     # the factor enters from order 2 on
    "last, ragged block row of B dropped from C B^-1 C^T": (_last_block_row_of_B, "acdefghi"),   # N = 128: none is ragged
    "last GEMV slab dropped from fl'": (_last_gemv_slab, "abcdefghi"),
    "last pixel left out of the design matrix": (_last_pixel_not_in_D, "abcdefghi"),
    "C untransposed": (_C_untransposed, "abe"),                                  # the shapes allow it only where M == N
}


def test_defect_table_is_consistent():
    for name, (_, applies) in DEFECTS.items():
        for case in cr.CASES:
            if name.startswith("mu = 1"):
                assert (case.name in applies) == (case.mu != 1.0)
            if name.startswith("C untransposed"):
                assert (case.name in applies) == (case.M == case.N)
            if name.startswith("highest column") or name.startswith("Chebyshev domain"):
                assert (case.name in applies) == (case.order >= (2 if name.startswith("highest") else 1))
            if name.startswith("last, ragged"):
                assert (case.name in applies) == (case.N % cr.NB != 0)
    assert len(DEFECTS) == 8


@pytest.mark.parametrize("name", list(DEFECTS), ids=[f"defect{i}" for i in range(len(DEFECTS))])
def test_seeded_defect_leaves_the_bound(name):
    defect, applies = DEFECTS[name]
    caught = []
    for case in cr.CASES:
        if case.name not in applies:
            continue
        inp = cr.case_inputs(case)
        ref = cr.case_ext(case, "grids")
        assert _within(cr.errors(cr.calibrate_f64_route(inp, case.order, case.mu), ref), TOL["grids"])   # sound without it
        err = cr.errors(defect(case, inp), ref)
        print(f"{name} / {cr.case_id(case)}: " + ", ".join(f"{k} {v:.2e} ({TOL['grids'][k]:.2e})" for k, v in err.items()))
        if not _within(err, TOL["grids"]):
            caught.append(case.name)
    assert caught, name                                       # the condition: caught on a case it applies to
    assert caught == [n for n in applies], (name, caught)     # as the table stands, on every one of them
