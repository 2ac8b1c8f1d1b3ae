"""GPU tests of the analytic gradient of the likelihood (psoap_chunk_lnlike_grad, psoap_amd/csrc/grad_kernels.hpp).

Shapes at the edges of the 128-row tiles (tests/grad_reference.py: CASES), masked chunks with unequal epochs, the
benchmark hyper-parameters, mu_GP = 0.9.  ``lnp`` against the oracle at the project's 1e-10 max(1, |lnp|); the gradient
against the long-double reference, every entry, relative to the cancellation scale S = 1/2 sum_ij |Q_ij| |dK_ij/dtheta|
of its sum (sum_i |alpha_i| for mu_GP).

The tolerance is derived, not fitted: the float64 SciPy evaluation of the same formulas (cho_factor / cho_solve,
grad_reference.grad_f64) measured against the long-double one on these very cases (python tests/grad_reference.py),
max over the entries of |f64 - long double| / S:

    case        grad_gp    grad_mu   grad_lwl
    N100-c2    2.94e-17   1.31e-17   5.28e-15
    N128-c2    3.09e-17   1.21e-17   1.20e-14
    N129-c2    2.41e-17   2.32e-17   3.55e-15
    N300-c1    2.92e-17   2.68e-18   2.23e-14
    N300-c2    2.21e-17   3.35e-18   1.24e-14
    N300-c3    1.46e-16   1.15e-18   3.82e-14
    N520-c2    1.17e-17   2.73e-17   6.48e-14
    max        1.46e-16   2.73e-17   6.48e-14

The device sums in another order and fuses multiply-adds but is fp64 throughout: it gets the largest measured value of
each output times a margin of 8:

    grad_gp  8 x 1.46e-16 = 1.17e-15      grad_mu  8 x 2.73e-17 = 2.18e-16      grad_lwl  8 x 6.48e-14 = 5.18e-13
"""
import json
import os

import numpy as np
import pytest

import grad_reference as gr
from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu

LNP_RTOL = 1e-10
MARGIN = 8
F64_REL_TO_S = {"gp": 1.46e-16, "mu": 2.73e-17, "lwl": 6.48e-14}        # the table above, last row
TOL = {k: MARGIN * v for k, v in F64_REL_TO_S.items()}


def _handle(ch, **kw):
    from psoap_amd.chunk import ChunkHandle
    return ChunkHandle(ch.fl, ch.sigma, **kw)


def _bits(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float64).view(np.int64).copy() for a in arrays]


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(*a), _bits(*b)))


@pytest.mark.parametrize("case", gr.CASES, ids=gr.case_id)
def test_gradient_against_long_double(oracle, case):
    ch, gp, ref = gr.case_chunk(case), gr.case_gp(case), gr.case_ext(case)
    with _handle(ch) as h:
        lnp, g_gp, g_lwl, g_mu = h.lnlike_grad(ch.lwls, gp, gr.MU_GP)
        same = h.lnlike(ch.lwls, gp, gr.MU_GP)
    want = oracle.lnlike(ch.lwls, ch.fl, ch.sigma, gp, gr.MU_GP)
    err = {"gp": gr.rel_to_scale(g_gp, ref.gp, ref.s_gp), "mu": gr.rel_to_scale(g_mu, ref.mu, ref.s_mu),
           "lwl": gr.rel_to_scale(g_lwl, ref.lwl, ref.s_lwl)}
    print(f"{gr.case_id(case)}: lnp {lnp!r} oracle {want!r} psoap_lnlike {same!r}; error / S: " +
          ", ".join(f"{k} {v:.2e} (bound {TOL[k]:.2e})" for k, v in err.items()))
    assert abs(lnp - want) <= LNP_RTOL * max(1.0, abs(want))
    assert abs(lnp - same) <= 1e-14 * max(1.0, abs(same))          # another summation order (a few ulp)
    assert g_lwl.shape == ch.lwls.shape and np.all(np.isfinite(g_lwl))
    for k in ("gp", "mu", "lwl"):
        assert err[k] <= TOL[k], (k, err[k], TOL[k])


def _proposals(ch, B, seed):
    gps = syn.make_walkers(ch.n_components, B, seed=seed)
    lw = syn.walker_lwls(ch, syn.make_walker_velocities(ch, B, seed=seed + 1))
    return lw, gps


def test_batches_are_bit_reproducible_and_independent_of_the_grouping():
    """B = 3 different proposals = three B = 1 calls, bit for bit; the same call twice; and B = 10 -- above the cap of 8
    matrices per group (include/psoap_gp.h) -- equals its proposals one by one."""
    ch = gr.case_chunk(gr.CASES[2])           # N = 129: two tile rows
    lw, gps = _proposals(ch, 10, 7300)
    with _handle(ch) as h:
        three = h.lnlike_grad(lw[:3], gps[:3], gr.MU_GP)
        again = h.lnlike_grad(lw[:3], gps[:3], gr.MU_GP)
        ten = h.lnlike_grad(lw, gps, gr.MU_GP)
        singles = [h.lnlike_grad(lw[b], gps[b], gr.MU_GP) for b in range(10)]
    assert three[0].shape == (3,) and three[1].shape == (3, 4) and three[2].shape == (3, 2, ch.N) and three[3].shape == (3,)
    assert _same_bits(three, again)
    assert len({float(v) for v in ten[0]}) == 10
    for b in range(10):
        one = [np.atleast_1d(v) for v in singles[b]]
        assert _same_bits([ten[k][b] for k in range(4)], one), b
        if b < 3:
            assert _same_bits([three[k][b] for k in range(4)], one), b


def test_conventions_negative_amplitude_not_positive_definite_null_outputs_release():
    import ctypes
    from psoap_amd._lib import check, dptr
    ch = gr.case_chunk(gr.CASES[0])
    lw, gps = _proposals(ch, 3, 7400)
    gps[1, 0] = -0.5
    with _handle(ch) as h:
        lnp, g_gp, g_lwl, g_mu = h.lnlike_grad(lw, gps, gr.MU_GP)
        assert np.isneginf(lnp[1]) and np.all(np.isnan(g_gp[1])) and np.all(np.isnan(g_lwl[1])) and np.isnan(g_mu[1])
        keep = [0, 2]
        assert np.all(np.isfinite(lnp[keep])) and np.all(np.isfinite(g_gp[keep])) and np.all(np.isfinite(g_lwl[keep]))
        # NULL for the optional outputs: the same bits in the others
        lnp2, g2 = np.empty(3), np.empty((3, 4))
        check(h._L.psoap_chunk_lnlike_grad(h._h, 3, 2, dptr(np.ascontiguousarray(lw)), dptr(np.ascontiguousarray(gps)),
                                           gr.MU_GP, dptr(lnp2), dptr(g2), None, None), "psoap_chunk_lnlike_grad")
        assert _same_bits([lnp2[keep], g2[keep]], [lnp[keep], g_gp[keep]]) and np.isneginf(lnp2[1])
        # release, then another call: the workspace comes back, and so do the bits
        h.grad_release()
        h.grad_release()
        assert _same_bits(h.lnlike_grad(lw[0], gps[0], gr.MU_GP), [v[0] for v in (lnp, g_gp, g_lwl, g_mu)])
    # not positive definite: zero noise and two identical pixels (the device's convention: -inf, no exception)
    lw2 = lw.copy()
    lw2[:, :, 1] = lw2[:, :, 0]
    from psoap_amd.chunk import ChunkHandle
    with ChunkHandle(ch.fl, np.zeros_like(ch.sigma)) as h:
        lnp, g_gp, g_lwl, g_mu = h.lnlike_grad(lw2[0], np.abs(gps[0]), gr.MU_GP)
    assert np.isneginf(lnp) and np.all(np.isnan(g_gp)) and np.all(np.isnan(g_lwl)) and np.isnan(g_mu)


def test_recorded_conventions_hold_for_lnlike_grad():
    """covariance.lnlike_grad on the inputs of golden_conventions_v1.json (what the REFERENCE's lnlike does with them):
    the same exception, -inf with NaN gradients, or the recorded value."""
    from psoap_amd import _convention_cases as cc, covariance
    with open(os.path.join(os.path.dirname(__file__), "golden", "golden_conventions_v1.json")) as fh:
        want = json.load(fh)
    n_comp = {"lnlike_f": 1, "lnlike_f_g": 2, "lnlike_f_g_h": 3}
    kinds = set()
    try:
        for name, fname, args, kwargs in cc.cases():
            c = n_comp[fname]
            call = lambda: covariance.lnlike_grad(args[:c], args[c], args[c + 1], args[c + 2:], **kwargs)    # noqa: E731
            kind = want[name]["kind"]
            kinds.add(kind)
            if kind in ("ValueError", "ZeroDivisionError"):
                with pytest.raises(ValueError if kind == "ValueError" else ZeroDivisionError):
                    call()
                continue
            lnp, g_gp, g_lwl, g_mu = call()
            if kind == "-inf":
                assert np.isneginf(lnp) and np.all(np.isnan(g_gp)) and np.all(np.isnan(g_lwl)) and np.isnan(g_mu), name
            else:
                assert abs(lnp - want[name]["value"]) <= LNP_RTOL * max(1.0, abs(want[name]["value"])), name
                assert g_gp.shape == (2 * c,) and g_lwl.shape == (c, len(args[0]))
    finally:
        covariance.release_handles()
    assert kinds == {"ValueError", "ZeroDivisionError", "-inf", "finite"}


def test_gradient_leaves_the_handle_as_it_was():
    """a persistent-kernel evaluation before and after a gradient call on the same handle: identical bits, and an
    uploaded batch survives the call"""
    ch = gr.case_chunk(gr.CASES[4])
    lw, gps = _proposals(ch, 4, 7500)
    with _handle(ch, max_batch=4) as h:
        before = h.lnlike_batch(lw, gps, gr.MU_GP)
        h.upload(lw[::-1].copy(), gps[::-1].copy(), gr.MU_GP)
        h.lnlike_grad(lw[:2], gps[:2], 1.1)
        h.eval()
        pending = h.fetch()
        after = h.lnlike_batch(lw, gps, gr.MU_GP)
    assert _same_bits([before], [after]) and _same_bits([pending], [before[::-1]])


def test_optimize_GP_reaches_at_least_the_simplex_fit():
    """c = 1, N = 200: L-BFGS-B with the analytic gradient ends at a likelihood no lower than Nelder-Mead's from the same
    start, minus the optimiser's own ftol (relative to the value, SciPy's definition)"""
    from psoap_amd import covariance
    ch = syn.make_chunk(1, 4, 50, seed=7600)
    assert ch.N == 200
    start, ftol = np.array([0.3, 8.0]), 1e-10
    try:
        res = covariance.optimize_GP(ch.lwls, ch.fl, ch.sigma, start, 1.0, ftol=ftol, full_output=True)
        simplex = covariance.optimize_GP_f(ch.lwls[0], ch.fl, ch.sigma, start[0], start[1], 1.0)
        l_grad = covariance.lnlike_f(None, ch.lwls[0], ch.fl, ch.sigma, *res.x)
        l_simplex = covariance.lnlike_f(None, ch.lwls[0], ch.fl, ch.sigma, *simplex)
        l_start = covariance.lnlike_f(None, ch.lwls[0], ch.fl, ch.sigma, *start)
    finally:
        covariance.release_handles()
    print(f"L-BFGS-B {res.x} lnL {l_grad!r} in {res.nfev} evaluations, |grad| {np.linalg.norm(res.jac):.3e}; "
          f"Nelder-Mead {simplex} lnL {l_simplex!r}; start lnL {l_start!r}")
    assert np.all(res.x > 0) and l_grad > l_start
    assert l_grad >= l_simplex - ftol * max(1.0, abs(l_simplex))
