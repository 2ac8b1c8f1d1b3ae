"""GPU tests of the Fisher information and the leave-one-out under the time-variable kernel (psoap_chunk_fisher_tv,
psoap_chunk_loo_tv; psoap_amd/csrc/fisher_kernels.hpp).

Shapes at the edges of the 128-row tiles (tests/timevar_fisher_reference.py: CASES, each with its own tau, one with the pixels
in no time order); per case T = 3c + 3 tangents: the 2c unit tangents of gp, the c of tau, two velocity tangents and one random
grid tangent.  The device's F against the long-double reference, every entry, relative to sqrt(F_ss F_tt); F_mu relative to
itself; the leave-one-out in the units of tests/test_gpu_loo.py.

The tolerances are derived, not fitted: the float64 twin (``fisher_tv_f64``, ``loo_tv_f64``: SciPy on a matrix whose exp()
arguments are formed in the device's order) measured against the long-double evaluation on these very cases
(python tests/timevar_fisher_reference.py):

    case                   F       F_mu
    N100-c2         4.88e-15   3.33e-16
    N128-c2         3.39e-14   2.87e-18
    N129-c2         4.17e-15   1.43e-16
    N300-c1         6.74e-15   9.96e-17
    N300-c2         9.65e-15   8.83e-18
    N300-c3         9.23e-15   9.48e-17
    N300-c2-perm    3.02e-14   1.82e-15
    max             3.39e-14   1.82e-15

    case            pix_mean    pix_var   pix_logp   loo_logp   ep_resid    ep_chi2    ep_logp
    N129-c2         3.35e-15   4.42e-14   6.37e-14   2.26e-16   2.33e-15   1.55e-14   1.81e-15
    N300-c2-perm    8.96e-15   1.37e-13   6.89e-13   2.61e-16   6.54e-15   4.92e-14   6.78e-15
    max             8.96e-15   1.37e-13   6.89e-13   2.61e-16   6.54e-15   4.92e-14   6.78e-15

The device sums in another order and fuses multiply-adds but is fp64 throughout: it gets the largest measured value of each
output times the project's margin of 8:

    F  8 x 3.39e-14 = 2.71e-13      F_mu  8 x 1.82e-15 = 1.46e-14
    pix_mean 7.17e-14  pix_var 1.10e-12  pix_logp 5.51e-12  loo_logp 2.09e-15  ep_resid 5.23e-14  ep_chi2 3.94e-13  ep_logp 5.42e-14

Planted variability (``timevar_fisher_reference.planted``: N300-c2 with its flux redrawn from the time-variable K, both
tau = 0.25 span, seed 4).  The epoch farthest in time from the others is epoch 0 (50 pixels); the float64 reference gives
chi2 / npix = 1.1538 for it under the time-variable K and 68.3609 under the static K: |1.1538 - 1| = 0.15 against 67.4.
"""
import numpy as np
import pytest

import loo_reference as lr
import timevar_fisher_reference as tf

pytestmark = pytest.mark.gpu

MARGIN = 8
F64_REL = {"F": 3.39e-14, "mu": 1.82e-15}        # the first table above, last row
TOL = {k: MARGIN * v for k, v in F64_REL.items()}
LOO_F64 = {"pix_mean": 8.96e-15, "pix_var": 1.37e-13, "pix_logp": 6.89e-13, "loo_logp": 2.61e-16, "ep_resid": 6.54e-15,
           "ep_chi2": 4.92e-14, "ep_logp": 6.78e-15}        # the second table, last row
LOO_TOL = {k: MARGIN * v for k, v in LOO_F64.items()}
PLANT_CPU = {"epoch": 0, "tv": 1.1538, "static": 68.3609}
_LD = np.longdouble
LOO_FIELDS = ("lnp", "loo_logp", "pix_mean", "pix_var", "pix_logp", "ep_resid", "ep_chi2", "ep_logp", "ep_npix")


def _handle(d, **kw):
    from psoap_amd.chunk import ChunkHandle
    h = ChunkHandle(d.fl, d.sigma, **kw)
    h.set_times(d.times)
    return h


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).copy()


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _same_loo(a, b):
    return all(_same_bits(getattr(a, k), getattr(b, k)) for k in LOO_FIELDS)


@pytest.mark.parametrize("case", tf.CASES, ids=tf.case_id)
def test_fisher_tv_against_long_double(case):
    d = tf.case_data(case)
    tan_lwl, tan_gp, tan_tau = tf.case_tangents(case)
    F_ref, mu_ref = tf.case_ext(case)
    with _handle(d) as h:
        F, F_mu = h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp, tan_tau, tan_lwl, want_mu=True)
    err = {"F": tf.rel_to_scale(F, F_ref), "mu": float(abs(_LD(F_mu) - mu_ref) / mu_ref)}
    print(f"{tf.case_id(case)}: " + ", ".join(f"{k} {v:.2e} (bound {TOL[k]:.2e})" for k, v in err.items()))
    assert F.shape == (tan_gp.shape[0],) * 2 and np.all(np.isfinite(F))
    assert _same_bits(F, F.T)                                                   # rule 2
    for k in ("F", "mu"):
        assert err[k] <= TOL[k], (k, err[k], TOL[k])


@pytest.mark.parametrize("case", tf.CASES, ids=tf.case_id)
def test_tau_inf_is_the_static_call_bit_for_bit(case):
    """rule 1: with every tau = inf, the bits of ``fisher`` in every entry whose two tangents have no time-scale part, and of
    F_mu; exact zeros in the rows and columns of the pure time-scale tangents; and a time-scale part added to the OTHER
    tangents changes no bit.  ``loo_tv`` at tau = inf: the bits of ``loo`` in every field."""
    d = tf.case_data(case)
    c = d.lwls.shape[0]
    tan_lwl, tan_gp, tan_tau = tf.case_tangents(case)
    ep, ne = tf.case_epochs(case)
    inf = np.full(c, np.inf)
    shared = [t for t in range(3 * c + 3) if not np.any(tan_tau[t])]
    pure = [t for t in range(3 * c + 3) if t not in shared]
    loud = np.where(np.any(tan_tau, axis=1)[:, None], tan_tau, 3.0 + np.arange(c)[None, :])       # tan_tau != 0 everywhere
    with _handle(d) as h:
        S, S_mu = h.fisher(d.lwls, d.gp, tan_gp[shared], tan_lwl[shared], want_mu=True)
        F, F_mu = h.fisher_tv(d.lwls, d.gp, inf, tan_gp, tan_tau, tan_lwl, want_mu=True)
        L, L_mu = h.fisher_tv(d.lwls, d.gp, inf, tan_gp, loud, tan_lwl, want_mu=True)
        N_ = h.fisher_tv(d.lwls, d.gp, inf, tan_gp[shared], None, tan_lwl[shared])
        loo_static = h.loo(d.lwls, d.gp, tf.MU_GP, ep, ne)
        loo_inf = h.loo_tv(d.lwls, d.gp, inf, tf.MU_GP, ep, ne)
        pix_static = h.loo(d.lwls, d.gp, tf.MU_GP)
        pix_inf = h.loo_tv(d.lwls, d.gp, inf, tf.MU_GP)
    assert np.all(np.isfinite(S))
    assert _same_bits(F[np.ix_(shared, shared)], S) and _same_bits(F_mu, S_mu)
    assert np.all(F[pure] == 0.0) and np.all(F[:, pure] == 0.0)
    assert _same_bits(L, F) and _same_bits(L_mu, F_mu)
    assert _same_bits(N_, S)
    assert np.isfinite(loo_static.lnp) and _same_loo(loo_inf, loo_static)
    assert pix_inf.ep_chi2 is None and all(_same_bits(getattr(pix_inf, k), getattr(pix_static, k)) for k in LOO_FIELDS[:5])


def test_bits_repeat_and_a_subsequence_of_the_tangents_shares_them():
    """rules 2 and 3 on N300-c3 (three tile rows, T = 12, tau = (0.25 span, inf, 2 span))"""
    case = next(c for c in tf.CASES if tf.case_id(c) == "N300-c3")
    d = tf.case_data(case)
    tan_lwl, tan_gp, tan_tau = tf.case_tangents(case)
    pick = [1, 6, 8, 10]                    # a length scale, two time scales, a velocity tangent
    with _handle(d) as h:
        full, mu = h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp, tan_tau, tan_lwl, want_mu=True)
        again, mu2 = h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp, tan_tau, tan_lwl, want_mu=True)
        few = h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp[pick], tan_tau[pick], tan_lwl[pick])
        one = h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp[6:7], tan_tau[6:7])
    assert _same_bits(full, again) and _same_bits(mu, mu2)
    assert _same_bits(full, full.T) and _same_bits(few, few.T)
    assert _same_bits(few, full[np.ix_(pick, pick)])
    assert _same_bits(one[0, 0], full[6, 6]) and full[6, 6] > 0
    assert np.all(full[7] == 0.0)           # tau_1 = inf


@pytest.mark.parametrize("name", ["N129-c2", "N300-c2-perm"])
def test_loo_tv_against_long_double_and_lnp_has_the_bits_of_lnlike_tv(name):
    """rule 4, and every output of the leave-one-out within the derived bounds, with an epoch index"""
    case = next(c for c in tf.CASES if tf.case_id(c) == name)
    d = tf.case_data(case)
    ep, ne = tf.case_epochs(case)
    ref = tf.case_loo_ext(case)
    with _handle(d) as h:
        got = h.loo_tv(d.lwls, d.gp, d.tau, tf.MU_GP, ep, ne)
        lnp = h.lnlike_tv(d.lwls, d.gp, d.tau, tf.MU_GP)
        lnp_grad = h.lnlike_tv_grad(d.lwls, d.gp, d.tau, tf.MU_GP)[0]
        static = h.loo(d.lwls, d.gp, tf.MU_GP, ep, ne)
    err = lr.errors(got, ref)
    print(f"{name}: " + ", ".join(f"{k} {err[k]:.2e} (bound {LOO_TOL[k]:.2e})" for k in lr.OUTPUTS))
    assert _same_bits(got.lnp, lnp) and _same_bits(got.lnp, lnp_grad)
    assert abs(_LD(got.lnp) - ref.lnp) <= 1e-10 * abs(ref.lnp)
    assert np.array_equal(got.ep_npix, ref.ep_npix)
    for k in lr.OUTPUTS:
        assert err[k] <= LOO_TOL[k], (k, err[k], LOO_TOL[k])
    assert not _same_bits(got.pix_mean, static.pix_mean)          # a finite tau is another model


def test_planted_variability_fits_the_time_variable_model_only():
    d, fl, tau, ep, ne, far = tf.planted()
    assert far == PLANT_CPU["epoch"]
    from psoap_amd.chunk import ChunkHandle
    with ChunkHandle(fl, d.sigma) as h:
        h.set_times(d.times)
        tv = h.loo_tv(d.lwls, d.gp, tau, tf.MU_GP, ep, ne)
        st = h.loo(d.lwls, d.gp, tf.MU_GP, ep, ne)
    a, b = tv.ep_chi2[far] / tv.ep_npix[far], st.ep_chi2[far] / st.ep_npix[far]
    print(f"epoch {far}: chi2 / npix {a:.4f} under the time-variable K (CPU {PLANT_CPU['tv']}), {b:.4f} under the static K "
          f"(CPU {PLANT_CPU['static']})")
    assert abs(a - 1) < abs(b - 1)


def test_conventions_nan_everywhere_and_the_next_call_keeps_its_bits():
    from psoap_amd.chunk import ChunkHandle
    case = tf.CASES[0]
    d = tf.case_data(case)
    c = d.lwls.shape[0]
    tan_lwl, tan_gp, tan_tau = tf.case_tangents(case)
    ep, ne = tf.case_epochs(case)
    T = tan_gp.shape[0]

    def refused(h, gp, tau, lwls=d.lwls):
        F, mu = h.fisher_tv(lwls, gp, tau, tan_gp, tan_tau, tan_lwl, want_mu=True)       # status 0: no exception
        assert F.shape == (T, T) and np.all(np.isnan(F)) and np.isnan(mu)
        r = h.loo_tv(lwls, gp, tau, tf.MU_GP, ep, ne)
        assert r.lnp == -np.inf and np.isnan(r.loo_logp)
        assert all(np.all(np.isnan(getattr(r, k))) for k in ("pix_mean", "pix_var", "pix_logp", "ep_resid", "ep_chi2", "ep_logp"))

    with _handle(d) as h:
        good = h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp, tan_tau, tan_lwl, want_mu=True)
        good_loo = h.loo_tv(d.lwls, d.gp, d.tau, tf.MU_GP, ep, ne)
        neg = d.gp.copy()
        neg[0] = -neg[0]
        for gp, tau in ((neg, d.tau), (d.gp, np.array([0.0, d.tau[1]])), (d.gp, np.array([d.tau[0], np.nan])),
                        (d.gp, np.array([-1.0, 1.0]))):
            refused(h, gp, tau)
            after = h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp, tan_tau, tan_lwl, want_mu=True)
            assert _same_bits(after[0], good[0]) and _same_bits(after[1], good[1])
            assert _same_loo(h.loo_tv(d.lwls, d.gp, d.tau, tf.MU_GP, ep, ne), good_loo)
        # release, twice, then another call: the workspaces come back, and so do the bits
        h.fisher_release(), h.fisher_release(), h.loo_release(), h.grad_release()
        assert _same_bits(h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp, tan_tau, tan_lwl), good[0])
        assert _same_loo(h.loo_tv(d.lwls, d.gp, d.tau, tf.MU_GP, ep, ne), good_loo)
        assert h.fisher_tv(d.lwls, d.gp, d.tau, np.tile(tan_gp[:1], (32, 1))).shape == (32, 32)
    # not positive definite: zero noise and two identical pixels observed at the same time
    lw, t = d.lwls.copy(), d.times.copy()
    lw[:, 1], t[1] = lw[:, 0], t[0]
    with ChunkHandle(d.fl, np.zeros_like(d.sigma)) as h:
        h.set_times(t)
        refused(h, d.gp, d.tau, lw)
    assert c == 2


def test_refusals_raise_with_their_messages():
    from psoap_amd._lib import PsoapError
    from psoap_amd.chunk import ChunkHandle
    import grad_reference as gr
    case = tf.CASES[0]
    d = tf.case_data(case)
    c = d.lwls.shape[0]
    _tan_lwl, tan_gp, tan_tau = tf.case_tangents(case)
    with ChunkHandle(d.fl, d.sigma) as h:
        with pytest.raises(PsoapError, match="psoap_chunk_fisher_tv: call psoap_chunk_set_times first"):
            h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp, tan_tau)
        with pytest.raises(PsoapError, match="psoap_chunk_loo_tv: call psoap_chunk_set_times first"):
            h.loo_tv(d.lwls, d.gp, d.tau)
        h.set_times(d.times)
        with pytest.raises(PsoapError, match="tangents must be between 1 and 32"):
            h.fisher_tv(d.lwls, d.gp, d.tau, np.zeros((0, 2 * c)))
        with pytest.raises(PsoapError, match="tangents must be between 1 and 32"):
            h.fisher_tv(d.lwls, d.gp, d.tau, np.zeros((33, 2 * c)))
        with pytest.raises(PsoapError, match="psoap_chunk_loo_tv: .*contiguous"):
            h.loo_tv(d.lwls, d.gp, d.tau, tf.MU_GP, np.arange(d.lwls.shape[1]) % 2, 2)
        h.stream_open(c, 1)
        try:
            with pytest.raises(PsoapError, match="psoap_chunk_fisher_tv: the handle has an open stream"):
                h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp, tan_tau)
            with pytest.raises(PsoapError, match="psoap_chunk_loo_tv: the handle has an open stream"):
                h.loo_tv(d.lwls, d.gp, d.tau)
        finally:
            h.stream_close()
        assert np.all(np.isfinite(h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp, tan_tau)))
        ch = gr.case_chunk(case[1])
        h.set_baseline(1, ch.lwl, ch.epoch_index, ch.n_epochs, [0.1, 0.1])
        with pytest.raises(PsoapError, match="psoap_chunk_fisher_tv: the handle has a baseline"):
            h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp, tan_tau)
        with pytest.raises(PsoapError, match="psoap_chunk_loo_tv: the handle has a baseline"):
            h.loo_tv(d.lwls, d.gp, d.tau)
        # the static entries stay what they were on such a handle
        assert np.all(np.isfinite(h.fisher(d.lwls, d.gp, tan_gp[:2 * c])))


def test_covariance_entries_give_the_bits_of_the_handle_calls():
    from psoap_amd import covariance
    case = next(c for c in tf.CASES if tf.case_id(c) == "N300-c3")
    d = tf.case_data(case)
    c = 3
    ep, ne = tf.case_epochs(case)
    t_abs = d.times + 2450000.5                         # the entry takes the minimum off
    eye = np.eye(3 * c)
    try:
        F = covariance.fisher_information_timevar(d.lwls, d.fl, d.sigma, d.gp, d.tau, t_abs)
        res = covariance.loo_timevar(d.lwls, d.fl, d.sigma, d.gp, d.tau, t_abs, tf.MU_GP, ep)
        cov, sd_gp, sd_tau = covariance.timevar_laplace(d.lwls, d.fl, d.sigma, d.gp, d.tau, t_abs)
        bad = covariance.fisher_information_timevar(d.lwls, d.fl, d.sigma, d.gp, [1.0, 0.0, 1.0], t_abs)
        bad_loo = covariance.loo_timevar(d.lwls, d.fl, d.sigma, -d.gp, d.tau, t_abs, tf.MU_GP, ep)
    finally:
        covariance.release_handles()
    t0 = t_abs - t_abs.min()
    from psoap_amd.chunk import ChunkHandle
    with ChunkHandle(d.fl, d.sigma) as h:
        h.set_times(t0)
        F_h = h.fisher_tv(d.lwls, d.gp, d.tau, eye[:, :2 * c], eye[:, 2 * c:])
        res_h = h.loo_tv(d.lwls, d.gp, d.tau, tf.MU_GP, ep, ne)
    assert F.shape == (9, 9) and _same_bits(F, F_h) and _same_loo(res, res_h)
    assert np.all(F[7] == 0.0) and np.all(F[:, 7] == 0.0) and F[6, 6] > 0 and F[8, 8] > 0       # tau_1 = inf
    ref = covariance._laplace_from_fisher(F_h, d.gp, d.tau, np.isfinite(d.tau))
    assert all(_same_bits(a, b) for a, b in zip((cov, sd_gp, sd_tau), ref))
    assert cov.shape == (8, 8) and np.isnan(sd_tau[1]) and np.all(sd_gp > 0)
    assert np.all(np.isnan(bad)) and bad.shape == (9, 9)
    assert bad_loo.lnp == -np.inf and np.all(np.isnan(bad_loo.pix_mean)) and np.array_equal(bad_loo.ep_npix, res.ep_npix)
