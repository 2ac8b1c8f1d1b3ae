"""CPU checks that pin the gradient formulas (tests/grad_reference.py) to the golden-pinned oracle: the long-double
analytic gradient against central finite differences of ``oracle.lnlike``, and ``covariance.velocity_gradient`` against a
finite difference through ``replicate_wls``."""
import numpy as np
import pytest

import grad_reference as gr
from psoap_amd import synthetic as syn

_LD = np.longdouble
N_PIX = (0, 1, 17, 31, 59)          # the handful of pixels whose wavelength derivative is checked, per component


def _chunk(c):
    ch = syn.make_chunk(c, 3, 20, seed=6100 + c)
    assert ch.N == 60
    return ch


def _central(f, h):
    return (f(+h) - f(-h)) / (2 * h)


@pytest.mark.parametrize("c", [1, 2, 3])
def test_long_double_gradient_matches_finite_differences_of_the_oracle(oracle, c):
    """Central differences D(h) = (f(+h) - f(-h)) / 2h of ``oracle.lnlike`` (float64, LAPACK) around the benchmark
    hyper-parameters and mu_GP = 0.9.  The bound on |g - D(h)| is stated, not fitted:

    * truncation: D(h) - g = h^2 f'''/6 + O(h^4), so D(2h) - D(h) = 3 (D(h) - g) + O(h^4): the truncation of D(h) is
      |D(2h) - D(h)| / 3, taken twice over for the O(h^4) term.  It is formed from the long-double likelihood (free of
      rounding at these steps) and must itself stay below 1e-6 of the derivative's scale: the steps (1e-3 relative for
      amplitudes, length scales and mu_GP, 2e-8 for ln-wavelengths -- 1/800 of l/c_kms) are chosen for that;
    * rounding of the oracle: D_oracle(h) - D_ext(h) = (d+ - d-) / 2h exactly, with d+- the oracle's own error at the two
      points, measured there against the long-double likelihood: (|d+| + |d-|) / 2h."""
    ch, gp, mu = _chunk(c), np.array(syn.GP_BASE[c]), gr.MU_GP
    ref = gr.grad_ext(ch.lwls, ch.fl, ch.sigma, gp, mu)
    assert abs(ref.lnp - oracle.lnlike(ch.lwls, ch.fl, ch.sigma, gp, mu)) <= 1e-10 * max(1.0, abs(ref.lnp))

    def check(name, g, scale, h, at):
        """``at(d)`` -> (lwls, gp, mu) with the parameter moved by d"""
        f_or = lambda d: _LD(oracle.lnlike(*at(d)[:1], ch.fl, ch.sigma, *at(d)[1:]))              # noqa: E731
        f_ext = lambda d: oracle.lnlike_ext(*at(d)[:1], ch.fl, ch.sigma, *at(d)[1:])              # noqa: E731
        d1, d2 = _central(f_ext, h), _central(f_ext, 2 * h)
        trunc = 2 * abs(d2 - d1) / 3
        assert trunc <= 1e-6 * scale, (name, float(trunc), float(scale))
        noise = (abs(f_or(+h) - f_ext(+h)) + abs(f_or(-h) - f_ext(-h))) / (2 * h)
        got = _central(f_or, h)
        bound = trunc + noise + 1e-12 * scale
        print(f"{name:10s} analytic {float(g):+.9e} difference {float(got):+.9e} bound {float(bound):.2e}")
        assert abs(got - _LD(g)) <= bound, (name, float(g), float(got), float(bound))

    for k in range(2 * c):
        def at(d, k=k):
            p = gp.copy()
            p[k] += d
            return ch.lwls, p, mu
        check(f"gp[{k}]", ref.gp[k], ref.s_gp[k], 1e-3 * gp[k], at)
    check("mu_GP", ref.mu, ref.s_mu, 1e-3, lambda d: (ch.lwls, gp, mu + d))
    for k in range(c):
        for i in N_PIX:
            def at(d, k=k, i=i):
                x = ch.lwls.copy()
                x[k, i] += d
                return x, gp, mu
            check(f"x[{k},{i}]", ref.lwl[k, i], ref.s_lwl[k, i], 2e-8, at)


def test_float64_reference_agrees_with_long_double():
    """the SciPy evaluation of the same formulas: what the device's tolerance is derived from (tests/test_gpu_grad.py)"""
    ch, gp = _chunk(2), np.array(syn.GP_BASE[2])
    a, b = gr.grad_ext(ch.lwls, ch.fl, ch.sigma, gp, gr.MU_GP), gr.grad_f64(ch.lwls, ch.fl, ch.sigma, gp, gr.MU_GP)
    assert gr.rel_to_scale(b.gp, a.gp, a.s_gp) < 1e-14 and gr.rel_to_scale(b.lwl, a.lwl, a.s_lwl) < 1e-12
    assert gr.rel_to_scale(b.mu, a.mu, a.s_mu) < 1e-14 and abs(a.lnp - b.lnp) <= 1e-11 * abs(a.lnp)


def test_gpu_cases_have_the_sizes_the_tiles_need():
    sizes = sorted({c[0] for c in gr.CASES})
    assert sizes == [100, 128, 129, 300, 520] and sorted(c[1] for c in gr.CASES if c[0] == 300) == [1, 2, 3]
    for case in gr.CASES:
        ch = gr.case_chunk(case)
        assert ch.N == case[0] and len(set(ch.mask.sum(axis=1))) > 1          # unequal epochs


def test_velocity_gradient_is_the_chain_rule_through_replicate_wls():
    """f(v) = sum_ci w_ci x_ci(v) with x = replicate_wls(lwl, v, mask) is linear in v, so its central difference has no
    truncation error; with the two grids subtracted pixel by pixel before the sum, each difference (2 / c_kms = 6.7e-6 at a
    step of 1 km/s) carries the rounding of ln-wavelengths near 8.6, 1e-15, i.e. 1.4e-10 of itself: the bound is 1e-9 of
    sum_i |w_i| / c_kms over the epoch's pixels."""
    from psoap_amd import covariance, data
    rng = np.random.default_rng(11)
    mask = rng.uniform(size=(5, 40)) > 0.3
    mask[2, :] = False                                      # an epoch with no pixel left
    mask[2, 7] = True
    lwl = np.log(5200.0) + 9e-6 * np.arange(int(mask.sum()))
    v = rng.uniform(-50, 50, size=(2, 5))
    w = rng.standard_normal((2, lwl.shape[0]))
    ep = data.epoch_index_of(mask)
    got = covariance.velocity_gradient(w, ep, 5)
    assert got.shape == (2, 5)
    for c in range(2):
        for e in range(5):
            dv = np.zeros_like(v)
            dv[c, e] = 1.0
            fd = np.sum(w * (data.replicate_wls(lwl, v + dv, mask) - data.replicate_wls(lwl, v - dv, mask))) / 2.0
            assert abs(fd - got[c, e]) <= 1e-9 * np.sum(np.abs(w[c][ep == e])) / data.c_kms
    # a leading batch axis, and the checks on the index
    assert np.array_equal(covariance.velocity_gradient(np.stack([w, 2 * w]), ep, 5)[1], 2 * got)
    with pytest.raises(ValueError):
        covariance.velocity_gradient(w, ep, 4)
    with pytest.raises(ValueError):
        covariance.velocity_gradient(w[:, :-1], ep, 5)
