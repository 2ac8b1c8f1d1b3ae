"""CPU checks that pin the gradient formulas of the continuum-marginalised likelihood (tests/marg_grad_reference.py): the
long-double analytic gradient against long-double central differences of ``marg_reference.marg_ext(...).lnp``, the limit of a
vanishing prior, and four seeded defects that the tolerance of tests/test_gpu_marg_grad.py must reject."""
import numpy as np
import pytest

import grad_reference as gr
import marg_grad_reference as mg
import marg_reference as mr
import test_gpu_marg_grad as tg

_LD = np.longdouble


def _central(f, h):
    return (f(+h) - f(-h)) / (2 * h)


@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_id)
def test_long_double_gradient_matches_finite_differences_of_marg_ext(case):
    """Central differences D(h) = (f(+h) - f(-h)) / 2h of the long-double marginal likelihood, at two steps.  The bound is
    stated, not fitted, as in tests/test_grad_reference.py: D(h) - g = h^2 f'''/6 + O(h^4), so the truncation of D(h) is
    |D(2h) - D(h)| / 3, taken twice over for the O(h^4) term; it must itself stay below 1e-6 of the derivative's scale (the
    steps are 1e-3 relative for amplitudes, length scales and mu_GP as in that test, and 5e-9 for ln-wavelengths -- 1/3300 of
    l/c_kms, a relative truncation of 1e-7; long double has the digits for it).  The rounding of a long-double likelihood
    (2^-64 of ~1e3, times the condition of Kt, over 2h: 1e-4 beside scales of 1e4 and more) is allowed 1e-8 of the scale.
    The weights alternate over the cases; every hyper-parameter, mu_GP and four grid points (first and last pixel, one on
    either side of the first tile edge or mid-chunk) of the first and the last component."""
    kind = mr.WEIGHTS[mr.CASES.index(case) % 2]
    lwls, fl, sigma, gp, x, ep, ne, order, sd, weight, mu = mr._case_args(case, kind)
    ref = mg.case_ext(case, kind)
    c, N = lwls.shape
    assert abs(ref.lnp - mr.case_ext(case, kind).lnp) <= 1e-15 * abs(ref.lnp)

    def check(name, g, scale, h, at):
        f = lambda d: mr.marg_ext(*at(d)[:1], fl, sigma, at(d)[1], x, ep, ne, order, sd, weight, at(d)[2]).lnp      # noqa: E731
        d1, d2 = _central(f, h), _central(f, 2 * h)
        trunc = 2 * abs(d2 - d1) / 3
        assert trunc <= 1e-6 * scale, (name, float(trunc), float(scale))
        bound = trunc + 1e-8 * scale
        print(f"{name:10s} analytic {float(g):+.9e} difference {float(d1):+.9e} bound {float(bound):.2e}")
        assert abs(d1 - _LD(g)) <= bound, (name, float(g), float(d1), float(bound))

    for k in range(2 * c):
        def at(d, k=k):
            p = gp.copy()
            p[k] += d
            return lwls, p, mu
        check(f"gp[{k}]", ref.gp[k], ref.s_gp[k], 1e-3 * gp[k], at)
    check("mu_GP", ref.mu, ref.s_mu, 1e-3, lambda d: (lwls, gp, mu + d))
    edge = 127 if N > 128 else N // 2
    for k in sorted({0, c - 1}):
        for i in sorted({0, edge, edge + 1, N - 1}):
            def at(d, k=k, i=i):
                xs = np.asarray(lwls, dtype=_LD).copy()          # (a float64 grid would round the step by 2e-7 of itself)
                xs[k, i] += d
                return xs, gp, mu
            check(f"x[{k},{i}]", ref.lwl[k, i], ref.s_lwl[k, i], 5e-9, at)


@pytest.mark.parametrize("case", [mr.case_named("a"), mr.case_named("e")], ids=mr.case_id)
def test_vanishing_prior_is_the_plain_gradient(case):
    """prior_sd = 1e-12: H Lambda H^T is 1e-24 |H|^2 beside a K of 1e-4 and more, twenty digits down; the marginal gradient
    is the plain one of tests/grad_reference.py to 1e-12 of its scale"""
    for kind in mr.WEIGHTS:
        args = list(mr._case_args(case, kind))
        args[8] = np.full(case[5] + 1, 1e-12)
        got = mg.marg_grad_ext(*args)
        ref = gr.grad_ext(args[0], args[1], args[2], args[3], args[10])
        assert abs(got.lnp - _LD(ref.lnp)) <= 1e-12 * abs(ref.lnp)
        for k, v in mg.errors(got, ref).items():
            assert v <= 1e-12, (kind, k, v)


def test_float64_route_is_within_the_device_tolerance():
    """the Woodbury route in float64 against the long-double dense one, on the smallest and the largest Q: what the device's
    tolerance is derived from stays below it (the whole table: python tests/marg_grad_reference.py)"""
    for name, kind in (("a", "flux"), ("f", "one")):
        case = mr.case_named(name)
        err = mg.errors(mg.marg_grad_f64(*mr._case_args(case, kind)), mg.case_ext(case, kind))
        for k, v in err.items():
            assert v <= tg.TOL[k], (name, k, v)


@pytest.mark.parametrize("defect", mg.DEFECTS)
def test_seeded_defect_is_rejected_at_the_device_tolerance(defect):
    """every case and weight: some output of the defective route misses the bound the GPU test applies"""
    for case in mr.CASES:
        for kind in mr.WEIGHTS:
            err = mg.errors(mg.marg_grad_f64(*mr._case_args(case, kind), defect=defect), mg.case_ext(case, kind))
            worst = max(err[k] / tg.TOL[k] for k in err)
            assert worst > 100.0, (defect, mr.case_id(case), kind, err)
