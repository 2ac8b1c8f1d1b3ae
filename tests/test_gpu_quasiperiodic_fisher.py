"""GPU tests of the Fisher information and the leave-one-out under the quasi-periodic kernel (psoap_chunk_fisher_qp,
psoap_chunk_loo_qp; k_qp_fisher_tangent_fill, k_qp_fisher_contract and k_qp_fisher_dot of psoap_amd/csrc/fisher_kernels.hpp).

Shapes at the edges of the 128-row tiles (tests/quasiperiodic_fisher_reference.py: CASES, each with its own tau, Gamma and P);
per case T = 8 tangents: two unit tangents, one mixed, pure dtau, pure dGamma, two pure dP, one grid tangent.  The device's F
against the long-double reference, every entry, relative to sqrt(F_ss F_tt); F_mu relative to itself; the leave-one-out in the
units of tests/test_gpu_loo.py.

The tolerances are derived, not fitted: the float64 twin (``fisher_qp_f64``, ``loo_qp_f64``) measured against the long-double
evaluation on these very cases on the CPU (python tests/quasiperiodic_fisher_reference.py; profiles/quasiperiodic_fisher.md):

    case                   F       F_mu
    N100-c2         6.72e-15   2.78e-16
    N128-c2         2.54e-15   1.67e-16
    N129-c2         4.62e-15   7.96e-17
    N300-c1         4.68e-15   9.85e-17
    N300-c2         4.47e-15   5.06e-17
    N300-c3         7.52e-15   2.87e-17
    N300-c2-perm    2.80e-15   3.50e-16
    max             7.52e-15   3.50e-16

    case            pix_mean    pix_var   pix_logp   loo_logp   ep_resid    ep_chi2    ep_logp
    N129-c2         1.84e-15   2.50e-14   3.54e-14   1.17e-15   4.14e-15   1.07e-14   1.04e-15
    N300-c2-perm    7.22e-15   1.38e-13   3.04e-13   3.00e-15   5.38e-15   2.54e-14   4.41e-15
    max             7.22e-15   1.38e-13   3.04e-13   3.00e-15   5.38e-15   2.54e-14   4.41e-15

The device gets the largest measured value of each output times the project's margin of 8:

    F  8 x 7.52e-15 = 6.02e-14      F_mu  8 x 3.50e-16 = 2.80e-15
    pix_mean 5.78e-14  pix_var 1.10e-12  pix_logp 2.43e-12  loo_logp 2.40e-14  ep_resid 4.30e-14  ep_chi2 2.03e-13  ep_logp 3.53e-14

The fit (``quasiperiodic_reference.fit_case``), on the twin: P_0 = 84.694616 +- 0.382697 days, 0.27 sd from the planted 84.5907;
Gamma_0 = 1.836551 +- 0.427367, tau_0 = 773.58 +- 164.51 days.  The periodicity score at the planted period, at Gamma = 0 on the
fit's own (gp, tau): z = +1488.15 (S = +1.381e+06, I = 8.614e+05) on the planted draw, z = -1.8246 (S = -1.714e+03, I = 8.820e+05)
on the Gamma = 0 draw, whose quasi-periodic fit IS the time-variable fit (Gamma_0 -> 1e-9).  On the planted draw the
time-variable model RE-fitted drives tau_0 to 13.9 days, below the spacing of the epochs: no two epochs are correlated any
more, Gamma has nothing to act on (I = 0.060) and z there is +0.33 -- the score test at that point has no power, which is why
the test below takes the fit's own (gp, tau).
"""
import numpy as np
import pytest

import loo_reference as lr
import quasiperiodic_fisher_reference as qf
import quasiperiodic_reference as qr

pytestmark = pytest.mark.gpu

MARGIN = 8
F64_REL = {"F": 7.52e-15, "mu": 3.50e-16}        # the first table above, last row
TOL = {k: MARGIN * v for k, v in F64_REL.items()}
LOO_F64 = {"pix_mean": 7.22e-15, "pix_var": 1.38e-13, "pix_logp": 3.04e-13, "loo_logp": 3.00e-15, "ep_resid": 5.38e-15,
           "ep_chi2": 2.54e-14, "ep_logp": 4.41e-15}        # the second table, last row
LOO_TOL = {k: MARGIN * v for k, v in LOO_F64.items()}
# the twin's figures of the fit and of the score (the docstring's last lines)
TWIN_Z = {True: 1488.1490, False: -1.8246}
P_TRUE = 84.5907
_LD = np.longdouble
LOO_FIELDS = ("lnp", "loo_logp", "pix_mean", "pix_var", "pix_logp", "ep_resid", "ep_chi2", "ep_logp", "ep_npix")


def _handle(d, **kw):
    from psoap_amd.chunk import ChunkHandle
    h = ChunkHandle(d.fl, d.sigma, **kw)
    h.set_times(d.times)
    return h


def _eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _same_loo(a, b):
    return all(_eq(getattr(a, k), getattr(b, k)) for k in LOO_FIELDS)


def _case(name):
    return next(c for c in qf.CASES if qf.case_id(c) == name)


def _fisher(h, d, tans, want_mu=False, pick=None, gamma=None, period=None):
    tan_lwl, tan_gp, tan_tau, tan_gamma, tan_period = tans if pick is None else [a[pick] for a in tans]
    return h.fisher_qp(d.lwls, d.gp, d.tau, d.gamma if gamma is None else gamma, d.period if period is None else period, tan_gp,
                       tan_tau, tan_gamma, tan_period, tan_lwl, want_mu)


@pytest.mark.parametrize("case", qf.CASES, ids=qf.case_id)
def test_fisher_qp_against_long_double(case):
    d = qf.case_data(case)
    tans = qf.case_tangents(case)
    F_ref, mu_ref = qf.case_ext(case)
    with _handle(d) as h:
        F, F_mu = _fisher(h, d, tans, True)
    err = {"F": qf.rel_to_scale(F, F_ref), "mu": float(abs(_LD(F_mu) - mu_ref) / mu_ref)}
    print(f"{qf.case_id(case)}: " + ", ".join(f"{k} {v:.2e} (bound {TOL[k]:.2e})" for k, v in err.items()))
    assert F.shape == (8, 8) and np.all(np.isfinite(F))
    assert _eq(F, F.T)                                                          # rule 4
    if d.gamma[-1] == 0.0:                                                      # rule 3: dP of a component with Gamma = 0
        assert np.all(F[6] == 0.0) and np.all(F[:, 6] == 0.0)
    for k in ("F", "mu"):
        assert err[k] <= TOL[k], (k, err[k], TOL[k])


@pytest.mark.parametrize("case", qf.CASES, ids=qf.case_id)
def test_gamma_zero_is_the_time_variable_call(case):
    """rules 1, 2 and 5: with every Gamma = 0 and tan_gamma = 0, ``fisher_tv``'s F and F_mu whatever period and tan_period hold;
    a tangent with nothing but dP has an exactly-zero row and column; ``loo_qp`` is ``loo_tv`` field by field"""
    d = qf.case_data(case)
    c = d.lwls.shape[0]
    tan_lwl, tan_gp, tan_tau, _tan_gamma, tan_period = qf.case_tangents(case)
    T = tan_gp.shape[0]
    ep, ne = qf.case_epochs(case)
    zero = np.zeros(c)
    no_gamma = np.zeros((T, c))
    loud = tan_period + 3.0 + np.arange(c)[None, :]       # tan_period != 0 everywhere
    loud[5], loud[6] = tan_period[5], tan_period[6]       # ... but the pure dP tangents stay pure
    pure = [t for t in (5, 6) if not (np.any(tan_gp[t]) or np.any(tan_tau[t]) or np.any(tan_lwl[t]))]
    with _handle(d) as h:
        V, V_mu = h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp, tan_tau, tan_lwl, want_mu=True)
        F, F_mu = h.fisher_qp(d.lwls, d.gp, d.tau, zero, d.period, tan_gp, tan_tau, no_gamma, tan_period, tan_lwl, True)
        L, L_mu = h.fisher_qp(d.lwls, d.gp, d.tau, zero, 7.0 * d.period[::-1].copy(), tan_gp, tan_tau, None, loud, tan_lwl, True)
        loo_tv = h.loo_tv(d.lwls, d.gp, d.tau, qf.MU_GP, ep, ne)
        loo_qp = h.loo_qp(d.lwls, d.gp, d.tau, zero, d.period, qf.MU_GP, ep, ne)
        pix_tv = h.loo_tv(d.lwls, d.gp, d.tau, qf.MU_GP)
        pix_qp = h.loo_qp(d.lwls, d.gp, d.tau, zero, 2.0 * d.period, qf.MU_GP)
    assert np.all(np.isfinite(V)) and pure == [5, 6]
    assert _eq(F, V) and _eq(F_mu, V_mu)
    assert _eq(L, V) and _eq(L_mu, V_mu)
    assert np.all(F[pure] == 0.0) and np.all(F[:, pure] == 0.0)
    assert np.isfinite(loo_tv.lnp) and _same_loo(loo_qp, loo_tv)
    assert pix_qp.ep_chi2 is None and all(_eq(getattr(pix_qp, k), getattr(pix_tv, k)) for k in LOO_FIELDS[:5])


def test_bits_repeat_a_subsequence_shares_them_and_the_workspace_leaves_no_trace():
    """rule 4 on N300-c3 (three tile rows, c = 3), with a call at another T and c on the same handle in between"""
    case, other = _case("N300-c3"), _case("N300-c1")
    d, o = qf.case_data(case), qf.case_data(other)
    tans, otans = qf.case_tangents(case), qf.case_tangents(other)
    pick = [1, 2, 4, 5, 7]
    with _handle(d) as h:
        full, mu = _fisher(h, d, tans, True)
        between = _fisher(h, o, otans, pick=[0, 2, 4])       # c = 1, T = 3: shorter records in the same workspace
        again, mu2 = _fisher(h, d, tans, True)
        few = _fisher(h, d, tans, pick=pick)
        one = _fisher(h, d, tans, pick=[4])
    assert np.all(np.isfinite(between))
    assert _eq(full, again) and _eq(mu, mu2)
    assert _eq(full, full.T) and _eq(few, few.T)
    assert _eq(few, full[np.ix_(pick, pick)])
    assert _eq(one[0, 0], full[4, 4]) and full[4, 4] > 0
    assert np.all(full[6] == 0.0) and full[5, 5] > 0       # Gamma_2 = 0; the period of the component with the largest Gamma


@pytest.mark.parametrize("name", ["N129-c2", "N300-c2-perm"])
def test_loo_qp_against_long_double_and_lnp_has_the_bits_of_lnlike_qp(name):
    """rule 5, and every output of the leave-one-out within the derived bounds, with an epoch index"""
    case = _case(name)
    d = qf.case_data(case)
    ep, ne = qf.case_epochs(case)
    ref = qf.case_loo_ext(case)
    with _handle(d) as h:
        got = h.loo_qp(d.lwls, d.gp, d.tau, d.gamma, d.period, qf.MU_GP, ep, ne)
        lnp = h.lnlike_qp(d.lwls, d.gp, d.tau, d.gamma, d.period, qf.MU_GP)
        lnp_grad = h.lnlike_qp_grad(d.lwls, d.gp, d.tau, d.gamma, d.period, qf.MU_GP)[0]
        tv = h.loo_tv(d.lwls, d.gp, d.tau, qf.MU_GP, ep, ne)
    err = lr.errors(got, ref)
    print(f"{name}: " + ", ".join(f"{k} {err[k]:.2e} (bound {LOO_TOL[k]:.2e})" for k in lr.OUTPUTS))
    assert _eq(got.lnp, lnp) and _eq(got.lnp, lnp_grad)
    assert abs(_LD(got.lnp) - ref.lnp) <= 1e-10 * abs(ref.lnp)
    assert np.array_equal(got.ep_npix, ref.ep_npix)
    for k in lr.OUTPUTS:
        assert err[k] <= LOO_TOL[k], (k, err[k], LOO_TOL[k])
    assert not _eq(got.pix_mean, tv.pix_mean)          # a positive Gamma is another model


def test_the_older_entries_return_what_they_returned():
    """rule 6: the static and time-variable Fisher, the time-variable leave-one-out and the quasi-periodic gradient before and
    after the new calls on one handle"""
    case = _case("N129-c2")
    d = qf.case_data(case)
    tans = qf.case_tangents(case)
    tan_lwl, tan_gp, tan_tau = tans[:3]
    ep, ne = qf.case_epochs(case)

    def older(h):
        return (h.fisher(d.lwls, d.gp, tan_gp, tan_lwl, want_mu=True), h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp, tan_tau, tan_lwl, True),
                h.loo_tv(d.lwls, d.gp, d.tau, qf.MU_GP, ep, ne), h.lnlike_qp_grad(d.lwls, d.gp, d.tau, d.gamma, d.period, qf.MU_GP))

    with _handle(d) as h:
        before = older(h)
        _fisher(h, d, tans, True)
        h.loo_qp(d.lwls, d.gp, d.tau, d.gamma, d.period, qf.MU_GP, ep, ne)
        after = older(h)
    for b, a in zip(before[:2], after[:2]):
        assert _eq(b[0], a[0]) and _eq(b[1], a[1]) and np.all(np.isfinite(b[0]))
    assert _same_loo(before[2], after[2])
    assert all(_eq(x, y) for x, y in zip(before[3], after[3]))


def test_conventions_nan_everywhere_and_the_next_call_keeps_its_bits():
    from psoap_amd.chunk import ChunkHandle
    case = qf.CASES[0]
    d = qf.case_data(case)
    tans = qf.case_tangents(case)
    ep, ne = qf.case_epochs(case)
    nan, inf = np.nan, np.inf

    def refused(h, gp=d.gp, tau=d.tau, gamma=d.gamma, period=d.period, lwls=d.lwls):
        tan_lwl, tan_gp, tan_tau, tan_gamma, tan_period = tans
        F, mu = h.fisher_qp(lwls, gp, tau, gamma, period, tan_gp, tan_tau, tan_gamma, tan_period, tan_lwl, True)   # status 0
        assert F.shape == (8, 8) and np.all(np.isnan(F)) and np.isnan(mu)
        r = h.loo_qp(lwls, gp, tau, gamma, period, qf.MU_GP, ep, ne)
        assert r.lnp == -np.inf and np.isnan(r.loo_logp)
        assert all(np.all(np.isnan(getattr(r, k))) for k in ("pix_mean", "pix_var", "pix_logp", "ep_resid", "ep_chi2", "ep_logp"))

    with _handle(d) as h:
        good = _fisher(h, d, tans, True)
        good_loo = h.loo_qp(d.lwls, d.gp, d.tau, d.gamma, d.period, qf.MU_GP, ep, ne)
        neg = d.gp.copy()
        neg[0] = -neg[0]
        g0, g1, p0, p1 = d.gamma[0], d.gamma[1], d.period[0], d.period[1]
        for kw in (dict(gp=neg), dict(tau=np.array([0.0, d.tau[1]])), dict(tau=np.array([d.tau[0], nan])),
                   dict(gamma=np.array([-1.0, g1])), dict(gamma=np.array([g0, nan])), dict(gamma=np.array([inf, g1])),
                   dict(period=np.array([0.0, p1])), dict(period=np.array([p0, -2.0])), dict(period=np.array([nan, p1])),
                   dict(period=np.array([p0, inf]))):
            refused(h, **kw)
        after = _fisher(h, d, tans, True)
        assert _eq(after[0], good[0]) and _eq(after[1], good[1])
        assert _same_loo(h.loo_qp(d.lwls, d.gp, d.tau, d.gamma, d.period, qf.MU_GP, ep, ne), good_loo)
        # release, twice, then another call: the workspaces come back, and so do the bits
        h.fisher_release(), h.fisher_release(), h.loo_release(), h.grad_release()
        assert _eq(_fisher(h, d, tans), good[0])
        assert _same_loo(h.loo_qp(d.lwls, d.gp, d.tau, d.gamma, d.period, qf.MU_GP, ep, ne), good_loo)
        assert h.fisher_qp(d.lwls, d.gp, d.tau, d.gamma, d.period, np.tile(tans[1][:1], (32, 1))).shape == (32, 32)
    # not positive definite: zero noise and two identical pixels observed at the same time
    lw, t = d.lwls.copy(), d.times.copy()
    lw[:, 1], t[1] = lw[:, 0], t[0]
    with ChunkHandle(d.fl, np.zeros_like(d.sigma)) as h:
        h.set_times(t)
        refused(h, lwls=lw)


def test_refusals_raise_with_their_messages():
    from psoap_amd._lib import PsoapError
    from psoap_amd.chunk import ChunkHandle
    import grad_reference as gr
    case = qf.CASES[0]
    d = qf.case_data(case)
    c = d.lwls.shape[0]
    tan_gp = qf.case_tangents(case)[1]
    hyper = (d.gp, d.tau, d.gamma, d.period)
    with ChunkHandle(d.fl, d.sigma) as h:
        with pytest.raises(PsoapError, match="psoap_chunk_fisher_qp: call psoap_chunk_set_times first"):
            h.fisher_qp(d.lwls, *hyper, tan_gp)
        with pytest.raises(PsoapError, match="psoap_chunk_loo_qp: call psoap_chunk_set_times first"):
            h.loo_qp(d.lwls, *hyper)
        h.set_times(d.times)
        with pytest.raises(PsoapError, match="psoap_chunk_fisher_qp: the number of tangents must be between 1 and 32"):
            h.fisher_qp(d.lwls, *hyper, np.zeros((0, 2 * c)))
        with pytest.raises(PsoapError, match="psoap_chunk_fisher_qp: the number of tangents must be between 1 and 32"):
            h.fisher_qp(d.lwls, *hyper, np.zeros((33, 2 * c)))
        with pytest.raises(PsoapError, match="psoap_chunk_loo_qp: .*contiguous"):
            h.loo_qp(d.lwls, *hyper, qf.MU_GP, np.arange(d.lwls.shape[1]) % 2, 2)
        h.stream_open(c, 1)
        try:
            with pytest.raises(PsoapError, match="psoap_chunk_fisher_qp: the handle has an open stream"):
                h.fisher_qp(d.lwls, *hyper, tan_gp)
            with pytest.raises(PsoapError, match="psoap_chunk_loo_qp: the handle has an open stream"):
                h.loo_qp(d.lwls, *hyper)
        finally:
            h.stream_close()
        assert np.all(np.isfinite(h.fisher_qp(d.lwls, *hyper, tan_gp)))
        ch = gr.case_chunk(case[1])
        h.set_baseline(1, ch.lwl, ch.epoch_index, ch.n_epochs, [0.1, 0.1])
        with pytest.raises(PsoapError, match="psoap_chunk_fisher_qp: the handle has a baseline"):
            h.fisher_qp(d.lwls, *hyper, tan_gp)
        with pytest.raises(PsoapError, match="psoap_chunk_loo_qp: the handle has a baseline"):
            h.loo_qp(d.lwls, *hyper)
        assert np.all(np.isfinite(h.fisher(d.lwls, d.gp, tan_gp[:2 * c])))


def test_covariance_entries_against_the_twin():
    """``fisher_information_quasiperiodic``, ``quasiperiodic_laplace`` and ``loo_quasiperiodic`` on N300-c3: the handle's bits,
    and the twin's figures within the derived bounds"""
    from psoap_amd import covariance
    case = _case("N300-c3")
    d = qf.case_data(case)
    c = 3
    ep, ne = qf.case_epochs(case)
    t_abs = d.times + 2450000.5                         # the entry takes the minimum off
    eye = np.eye(5 * c)
    free = {"period": np.array([True, True, False])}
    try:
        F = covariance.fisher_information_quasiperiodic(d.lwls, d.fl, d.sigma, d.gp, d.tau, d.gamma, d.period, t_abs)
        res = covariance.loo_quasiperiodic(d.lwls, d.fl, d.sigma, d.gp, d.tau, d.gamma, d.period, t_abs, qf.MU_GP, ep)
        lap = covariance.quasiperiodic_laplace(d.lwls, d.fl, d.sigma, d.gp, d.tau, d.gamma, d.period, t_abs)
        with pytest.raises(np.linalg.LinAlgError):       # the period of component 2, whose Gamma is 0, set free
            covariance.quasiperiodic_laplace(d.lwls, d.fl, d.sigma, d.gp, d.tau, d.gamma, d.period, t_abs,
                                             {"period": np.array([True, True, True])})
        lap_free = covariance.quasiperiodic_laplace(d.lwls, d.fl, d.sigma, d.gp, d.tau, d.gamma, d.period, t_abs, free)
        bad = covariance.fisher_information_quasiperiodic(d.lwls, d.fl, d.sigma, d.gp, d.tau, [1.0, -1.0, 0.0], d.period, t_abs)
        bad_loo = covariance.loo_quasiperiodic(d.lwls, d.fl, d.sigma, d.gp, d.tau, d.gamma, [1.0, 0.0, 1.0], t_abs, qf.MU_GP, ep)
    finally:
        covariance.release_handles()
    t0 = t_abs - t_abs.min()
    from psoap_amd.chunk import ChunkHandle
    with ChunkHandle(d.fl, d.sigma) as h:
        h.set_times(t0)
        F_h = h.fisher_qp(d.lwls, d.gp, d.tau, d.gamma, d.period, eye[:, :2 * c], eye[:, 2 * c:3 * c], eye[:, 3 * c:4 * c], eye[:, 4 * c:])
        res_h = h.loo_qp(d.lwls, d.gp, d.tau, d.gamma, d.period, qf.MU_GP, ep, ne)
    assert F.shape == (15, 15) and _eq(F, F_h) and _same_loo(res, res_h)
    assert np.all(F[7] == 0.0) and np.all(F[14] == 0.0) and F[12, 12] > 0 and F[13, 13] > 0      # tau_1 = inf, Gamma_2 = 0
    zeros = np.zeros((15, c, d.lwls.shape[1]))
    F_twin = qf.fisher_qp_f64(d.lwls, t0, d.sigma, d.gp, d.tau, d.gamma, d.period, zeros, eye[:, :2 * c], eye[:, 2 * c:3 * c],
                              eye[:, 3 * c:4 * c], eye[:, 4 * c:])[0]
    err = qf.rel_to_scale(F, F_twin)
    print(f"fisher_information_quasiperiodic against the twin: {err:.2e} (bound {2 * TOL['F']:.2e})")
    assert err <= 2 * TOL["F"]      # (both sides carry the twin's error against long double)
    ref = covariance._qp_laplace_from_fisher(F_h, d.gp, d.tau, d.gamma, d.period, None)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(lap, ref))       # (nan where a parameter is not free)
    cov, sd_gp, sd_tau, sd_gamma, sd_period = lap
    assert cov.shape == (12, 12) and np.isnan(sd_tau[1]) and np.isnan(sd_gamma[2]) and np.isnan(sd_period[2]) and np.all(sd_gp > 0)
    assert _eq(lap_free[0], cov)
    twin = covariance._qp_laplace_from_fisher(F_twin, d.gp, d.tau, d.gamma, d.period, None)
    np.testing.assert_allclose(sd_period[:2], twin[4][:2], rtol=1e-8)
    np.testing.assert_allclose(sd_gamma[:2], twin[3][:2], rtol=1e-8)
    assert np.all(np.isnan(bad)) and bad.shape == (15, 15)
    assert bad_loo.lnp == -np.inf and np.all(np.isnan(bad_loo.pix_mean)) and np.array_equal(bad_loo.ep_npix, res.ep_npix)


def test_the_planted_period_has_an_error_bar_that_holds_it():
    """the device's fit of ``fit_case(True)``: sd_period from ``quasiperiodic_laplace`` agrees with the twin's F at the same
    point, and the planted period lies within 5 sd of the fitted one"""
    from psoap_amd import covariance
    fc = qr.fit_case(True)
    try:
        gp, tau, gamma, period = covariance.optimize_GP_quasiperiodic(fc.lwls, fc.fl, fc.sigma, *fc.start, fc.times)
        lap = covariance.quasiperiodic_laplace(fc.lwls, fc.fl, fc.sigma, gp, tau, gamma, period, fc.times)
    finally:
        covariance.release_handles()
    twin = covariance._qp_laplace_from_fisher(qf.fit_fisher_twin(True, gp, tau, gamma, period), gp, tau, gamma, period, None)
    print(f"P_0 {period[0]:.6f} +- {lap[4][0]:.6f} (twin {twin[4][0]:.6f})  Gamma_0 {gamma[0]:.6f} +- {lap[3][0]:.6f}  "
          f"tau_0 {tau[0]:.4f} +- {lap[2][0]:.4f}")
    np.testing.assert_allclose(lap[4][0], twin[4][0], rtol=1e-6)
    np.testing.assert_allclose(lap[3][0], twin[3][0], rtol=1e-6)
    assert np.isnan(lap[4][1]) and np.isnan(lap[3][1]) and np.isnan(lap[2][1])
    assert abs(period[0] - P_TRUE) < 5 * lap[4][0]


@pytest.mark.parametrize("planted", [True, False], ids=["planted", "gamma0-draw"])
def test_periodicity_score_agrees_with_the_twin(planted):
    """z at the planted period, at Gamma = 0 on (gp, tau) of the quasi-periodic fit of the draw (the twin's fit: both sides at
    one point; on the Gamma = 0 draw that fit is the time-variable fit): the device's z is the twin's; large and positive on
    the planted draw, below 3 on the Gamma = 0 draw"""
    from psoap_amd import covariance
    fc = qr.fit_case(planted)
    gp, tau = qr.fit_on_twin(planted)[:2]
    try:
        z, S, I = covariance.periodicity_score(fc.lwls, fc.fl, fc.sigma, gp, tau, fc.times, fc.P0)
    finally:
        covariance.release_handles()
    zt, St, It = qf.score_twin(planted, gp, tau, fc.P0)
    print(f"{'planted' if planted else 'Gamma = 0 draw'}: z {z:+.6f} (twin {zt:+.6f}, recorded {TWIN_Z[planted]:+.4f})  "
          f"S {S:+.6e} (twin {St:+.6e})  I {I:.6e} (twin {It:.6e})")
    np.testing.assert_allclose(I, It, rtol=1e-6)
    assert abs(z - zt) <= 1e-6 * max(1.0, abs(zt))
    if planted:
        assert z > 5.0
    else:
        assert z < 3.0
