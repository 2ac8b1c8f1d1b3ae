"""GPU tests of the quasi-periodic kernel (psoap_chunk_lnlike_qp_grad, psoap_fill_sym_qp; k_fill_sym_qp in
psoap_amd/csrc/fill_kernels.hpp, k_qp_grad_contract and k_qp_grad_finish in grad_kernels.hpp).

The cases are those of tests/quasiperiodic_reference.py: the data of timevar_reference.CASES (N = 100 .. 520 at the edges of the
128-row tiles, c = 1, 2, 3, masked chunks with unequal epochs, mu_GP = 0.9, the permuted case) with a (tau, Gamma, P) triple per
component -- among them P shorter than the span by a factor of more than 20, P longer than the span, components with
Gamma = 0 and purely periodic ones (tau = inf, Gamma > 0).  ``lnp`` against the long-double reference at the project's 1e-10
max(1, |lnp|); the gradient against it, every entry, relative to the cancellation scale S = 1/2 sum_ij |Q_ij| |dK_ij/dtheta| of
its sum (sum_i |alpha_i| for mu_GP); the fill against the long-double matrix of the same float64 inputs, element by element,
relative.

The tolerances are derived, not fitted: the float64 twin (quasiperiodic_reference.qp_f64, matrix_f64: the device's operation
order) measured against long double on these very cases (python tests/quasiperiodic_reference.py), max over the entries:

    case              grad_gp    grad_tau  grad_gamma grad_period     grad_mu    grad_lwl         lnp        fill
    N100-c2          4.69e-17    5.85e-17    6.08e-17    4.83e-17    1.21e-17    3.59e-15    1.30e-16    7.62e-14
    N128-c2          1.63e-17    2.09e-17    2.60e-17    2.15e-17    5.14e-17    6.28e-15    3.84e-16    4.22e-14
    N129-c2          2.22e-17    2.89e-17    2.24e-17    9.19e-17    1.91e-17    2.68e-15    0.00e+00    5.14e-14
    N300-c1          4.78e-18    9.18e-18    1.12e-17    1.20e-17    6.80e-18    1.32e-15    1.61e-16    2.65e-13
    N300-c2          6.79e-17    9.27e-18    6.86e-17    1.08e-17    1.48e-17    1.60e-14    8.71e-16    1.68e-13
    N300-c3          1.26e-17    2.63e-17    8.80e-18    3.58e-17    5.98e-18    1.61e-15    3.34e-16    1.41e-13
    N520-c2          1.61e-17    3.90e-18    4.19e-18    1.41e-17    1.11e-17    5.10e-15    1.79e-16    2.15e-13
    N300-c2-perm     2.84e-17    2.16e-17    1.67e-17    1.84e-17    2.94e-17    1.62e-14    7.56e-16    1.42e-13
    max              6.79e-17    5.85e-17    6.86e-17    9.19e-17    5.14e-17    1.62e-14    8.71e-16    2.65e-13

Every output gets 8 x its largest measured value (the margin of tests/test_gpu_grad.py); ``lnp`` keeps the siblings' 1e-10.
(The fill's error is that of the ARGUMENT, rounded three times and up to 746 in size, through exp: the device and the twin
share it.)  tests/test_quasiperiodic_reference.py (CPU) holds the twin to this table and the six seeded defects out of it.
What the device measures is in profiles/quasiperiodic.md.
"""
import numpy as np
import pytest

import grad_reference as gr
import quasiperiodic_reference as qp
import timevar_reference as tv
from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu

LNP_RTOL = qp.LNP_RTOL
MARGIN = qp.MARGIN
F64_MAX = {"gp": 6.79e-17, "tau": 5.85e-17, "gamma": 6.86e-17, "period": 9.19e-17, "mu": 5.14e-17, "lwl": 1.62e-14,
           "fill": 2.65e-13}                                                                   # the table above, last row
LNP_F64_MAX = 8.71e-16
TOL = {k: MARGIN * v for k, v in F64_MAX.items()}
INF = float("inf")


def _handle(d, **kw):
    from psoap_amd.chunk import ChunkHandle
    h = ChunkHandle(d.fl, d.sigma, **kw)
    h.set_times(d.times)
    return h


def _bits(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float64).view(np.int64).copy() for a in arrays]


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(*a), _bits(*b)))


def _got(res):
    lnp, g_gp, g_tau, g_gam, g_per, g_lwl, g_mu = res
    return qp.QpGrad(lnp, g_gp, g_tau, g_gam, g_per, g_lwl, g_mu, None, None, None, None, None, None)


# ---- the fill --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_sigma", (False, True), ids=("plain", "sigma"))
@pytest.mark.parametrize("N", (129, 300))
@pytest.mark.parametrize("c", (1, 2, 3))
def test_fill_at_zero_gamma_is_the_time_variable_fill_bit_for_bit_whatever_the_period(c, N, with_sigma):
    """rule 1, the fill: finite and infinite tau, periods from a thousandth of the span to a thousand spans"""
    from psoap_amd import matrix_functions as mf
    ch = syn.make_chunk(c, 5, 60, seed=9300 + c)
    lw = np.ascontiguousarray(ch.lwls[:, :N])
    t = np.ascontiguousarray((ch.dates[ch.epoch_index] - ch.dates.min())[:N])
    span = float(t.max())
    gp = np.array(syn.GP_BASE[c], dtype=np.float64)
    tau = np.array([0.3 * span, INF, 2.0 * span][:c])
    sig = np.ascontiguousarray(ch.sigma[:N]) if with_sigma else None
    want = np.empty((N, N))
    mf.fill_V11_timevar(want, lw, t, gp, tau, sigma=sig)
    for period in (np.array([1e-3, 0.37, 1e3][:c]) * span, np.full(c, 1.0)):
        got = np.empty((N, N))
        mf.fill_V11_quasiperiodic(got, lw, t, gp, tau, np.zeros(c), period, sigma=sig)
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
    assert np.any(want[0, 1:] != 0.0) and len(np.unique(t)) > 1


@pytest.mark.parametrize("case", (qp.CASES[0], qp.CASES[5], qp.CASES[7]), ids=qp.case_id)
def test_within_an_epoch_the_blocks_are_those_of_the_static_fill(case):
    """rule 2: the chunk's times are constant per epoch, so dt = 0 and s = +0 exactly between two pixels of one epoch: there
    the matrix has the bits of psoap_fill_sym, with every Gamma > 0 and every tau finite; elsewhere it does not"""
    from psoap_amd import matrix_functions as mf
    d = qp.case_data(case)
    c, N = d.lwls.shape
    gamma, tau = np.full(c, 1.7), np.full(c, 0.4 * d.span)
    got, static = np.empty((N, N)), np.empty((N, N))
    mf.fill_V11_quasiperiodic(got, d.lwls, d.times, d.gp, tau, gamma, d.period, sigma=d.sigma)
    from psoap_amd import _lib
    from psoap_amd._lib import check, dptr
    check(_lib.load().psoap_fill_sym(_lib.default_device(), c, N, dptr(d.lwls), dptr(d.gp), dptr(d.sigma), dptr(static)),
          "psoap_fill_sym")
    same_epoch = d.times[:, None] == d.times[None, :]
    assert same_epoch.sum() > N and not np.all(same_epoch)
    assert np.array_equal(got[same_epoch].view(np.int64), static[same_epoch].view(np.int64))
    live = ~same_epoch & (static > 1e-300)
    assert live.any() and np.all(got[live] < static[live])


@pytest.mark.parametrize("case", qp.CASES, ids=qp.case_id)
def test_fill_against_the_long_double_matrix(case):
    from psoap_amd import matrix_functions as mf
    d = qp.case_data(case)
    N = d.lwls.shape[1]
    got = np.empty((N, N))
    mf.fill_V11_quasiperiodic(got, d.lwls, d.times, d.gp, d.tau, d.gamma, d.period, sigma=d.sigma)
    ext = qp.matrix_ext(d.lwls, d.times, d.gp, d.tau, d.gamma, d.period) + np.diag(np.asarray(d.sigma, dtype=np.longdouble) ** 2)
    twin = qp.matrix_f64(d.lwls, d.times, d.gp, d.tau, d.gamma, d.period, d.sigma)
    err = qp.fill_error(got, ext)
    ulp = np.abs(got.view(np.int64) - twin.view(np.int64))
    print(f"{qp.case_id(case)}: fill error {err:.2e} (bound {TOL['fill']:.2e}); against the twin max {int(ulp.max())} ulp, "
          f"{float(np.mean(ulp == 0)):.3f} of the elements equal")
    assert err <= TOL["fill"]
    assert np.array_equal(got, got.T) and not np.any(np.signbit(got))


# ---- value and gradient ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", qp.CASES, ids=qp.case_id)
def test_value_and_gradient_against_long_double(case):
    d, ref = qp.case_data(case), qp.case_ext(case)
    with _handle(d) as h:
        res = h.lnlike_qp_grad(d.lwls, d.gp, d.tau, d.gamma, d.period, qp.MU_GP)
        value_only = h.lnlike_qp(d.lwls, d.gp, d.tau, d.gamma, d.period, qp.MU_GP)
    got = _got(res)
    err = qp.errors(got, ref)
    print(f"{qp.case_id(case)}: lnp {got.lnp!r} long double {ref.lnp!r} ({qp.lnp_error(got.lnp, ref):.2e}); grad_gamma {got.gamma} "
          f"long double {np.asarray(ref.gamma, dtype=np.float64)}; grad_period {got.period} long double "
          f"{np.asarray(ref.period, dtype=np.float64)}; error / S: " + ", ".join(f"{k} {v:.2e} (bound {TOL[k]:.2e})" for k, v in err.items()))
    assert qp.lnp_error(got.lnp, ref) <= LNP_RTOL
    assert _same_bits([value_only], [got.lnp])
    assert got.lwl.shape == d.lwls.shape and np.all(np.isfinite(got.lwl))
    assert np.all(got.tau[np.isinf(d.tau)] == 0.0) and np.all(got.tau[np.isfinite(d.tau)] != 0.0)
    assert np.all(got.period[d.gamma == 0.0] == 0.0) and np.all(got.period[d.gamma > 0.0] != 0.0)
    assert np.all(np.isfinite(got.gamma)) and np.all(got.gamma != 0.0)
    for k in qp.OUTPUTS:
        assert err[k] <= TOL[k], (k, err[k], TOL[k])


@pytest.mark.parametrize("case", tv.CASES, ids=tv.case_id)
def test_zero_gamma_has_the_bits_of_lnlike_tv_grad(case):
    """rule 1: lnp, grad_gp, grad_tau, grad_lwl and grad_mu are the time-variable call's, grad_period is exactly 0 and
    grad_gamma, the score, is finite and not 0 -- at two sets of periods, which move the score alone"""
    d = tv.case_data(case)
    c = d.lwls.shape[0]
    with _handle(d) as h:
        want = h.lnlike_tv_grad(d.lwls, d.gp, d.tau, tv.MU_GP)
        scores = []
        for period in (np.array([0.031, 0.77, 4.0][:c]) * d.span, np.array([0.5, 0.11, 0.2][:c]) * d.span):
            lnp, g_gp, g_tau, g_gam, g_per, g_lwl, g_mu = h.lnlike_qp_grad(d.lwls, d.gp, d.tau, np.zeros(c), period, tv.MU_GP)
            assert _same_bits([lnp, g_gp, g_tau, g_lwl, g_mu], want)
            assert np.all(g_per == 0.0) and not np.any(np.signbit(g_per))
            assert np.all(np.isfinite(g_gam)) and np.all(g_gam != 0.0)
            assert _same_bits([h.lnlike_qp(d.lwls, d.gp, d.tau, np.zeros(c), period, tv.MU_GP)], [want[0]])
            scores.append(g_gam)
        assert not np.array_equal(scores[0], scores[1])
        again = h.lnlike_tv_grad(d.lwls, d.gp, d.tau, tv.MU_GP)
    assert _same_bits(again, want)


@pytest.mark.parametrize("shape", (gr.CASES[2], gr.CASES[3], gr.CASES[5]), ids=gr.case_id)
def test_zero_gamma_and_infinite_tau_have_the_bits_of_lnlike_grad(shape):
    ch, gp = gr.case_chunk(shape), gr.case_gp(shape)
    c = shape[1]
    from psoap_amd.chunk import ChunkHandle
    with ChunkHandle(ch.fl, ch.sigma) as h:
        h.set_times(ch.dates[ch.epoch_index] - ch.dates.min())
        static = h.lnlike_grad(ch.lwls, gp, gr.MU_GP)
        lnp, g_gp, g_tau, g_gam, g_per, g_lwl, g_mu = h.lnlike_qp_grad(ch.lwls, gp, np.full(c, INF), np.zeros(c), np.full(c, 3.3),
                                                                     gr.MU_GP)
    assert _same_bits([lnp, g_gp, g_lwl, g_mu], static)
    assert np.all(g_tau == 0.0) and np.all(g_per == 0.0) and np.all(np.isfinite(g_gam))


def _proposals(d, B, seed):
    """B different proposals on the case's chunk: perturbed grids, hyper-parameters, time scales (an inf stays inf), Gammas (a 0
    stays 0) and periods"""
    rng = np.random.default_rng(seed)
    c, N = d.lwls.shape
    lw = d.lwls[None] + rng.normal(0.0, 2.0 / syn.C_KMS, size=(B, c, 1))
    gps = d.gp[None] * rng.uniform(0.8, 1.25, size=(B, 2 * c))
    taus = np.where(np.isfinite(d.tau), 1.0, INF)[None] * np.where(np.isfinite(d.tau), d.tau, 1.0)[None] * rng.uniform(0.5, 2.0, size=(B, c))
    gams = d.gamma[None] * rng.uniform(0.5, 2.0, size=(B, c))
    pers = d.period[None] * rng.uniform(0.7, 1.4, size=(B, c))
    return tuple(np.ascontiguousarray(v) for v in (lw, gps, taus, gams, pers))


def test_batches_are_bit_reproducible_and_independent_of_the_grouping():
    """rule 3: B = 3 different proposals = three B = 1 calls, bit for bit; the same call twice; B = 10 -- above the cap of 8
    matrices per group -- equals its proposals one by one, and reversed it returns the reversed bits; the value-only call
    returns the bits of lnp of the full call"""
    d = qp.case_data(qp.CASES[2])           # N = 129: two tile rows
    lw, gps, taus, gams, pers = _proposals(d, 10, 9400)
    rev = slice(None, None, -1)
    with _handle(d) as h:
        three = h.lnlike_qp_grad(lw[:3], gps[:3], taus[:3], gams[:3], pers[:3], qp.MU_GP)
        again = h.lnlike_qp_grad(lw[:3], gps[:3], taus[:3], gams[:3], pers[:3], qp.MU_GP)
        ten = h.lnlike_qp_grad(lw, gps, taus, gams, pers, qp.MU_GP)
        back = h.lnlike_qp_grad(lw[rev], gps[rev], taus[rev], gams[rev], pers[rev], qp.MU_GP)
        values = h.lnlike_qp(lw, gps, taus, gams, pers, qp.MU_GP)
        singles = [h.lnlike_qp_grad(lw[b], gps[b], taus[b], gams[b], pers[b], qp.MU_GP) for b in range(10)]
    N = d.lwls.shape[1]
    assert [v.shape for v in three] == [(3,), (3, 4), (3, 2), (3, 2), (3, 2), (3, 2, N), (3,)]
    assert _same_bits(three, again)
    assert _same_bits([v[rev] for v in back], ten)
    assert len({float(v) for v in ten[0]}) == 10 and np.all(np.isfinite(ten[0]))
    assert values.shape == (10,) and _same_bits([values], [ten[0]])
    for b in range(10):
        one = [np.atleast_1d(v) for v in singles[b]]
        assert _same_bits([ten[k][b] for k in range(7)], one), b
        if b < 3:
            assert _same_bits([three[k][b] for k in range(7)], one), b


BAD = {"gamma-negative": ("gamma", -0.5), "gamma-nan": ("gamma", float("nan")), "gamma-inf": ("gamma", INF),
       "period-zero": ("period", 0.0), "period-negative": ("period", -3.0), "period-nan": ("period", float("nan")),
       "period-inf": ("period", INF), "tau-zero": ("tau", 0.0), "tau-nan": ("tau", float("nan")), "gp-negative": ("gp", -0.1)}


@pytest.mark.parametrize("bad", list(BAD))
def test_a_value_that_is_no_proposal_gives_minus_inf_there_and_leaves_the_others(bad):
    """rule 4 and the conventions"""
    d = qp.case_data(qp.CASES[0])
    lw, gps, taus, gams, pers = _proposals(d, 3, 9500)
    with _handle(d) as h:
        good = h.lnlike_qp_grad(lw, gps, taus, gams, pers, qp.MU_GP)
        arrays = {"gp": gps.copy(), "tau": taus.copy(), "gamma": gams.copy(), "period": pers.copy()}
        which, value = BAD[bad]
        arrays[which][1, 0] = value
        res = h.lnlike_qp_grad(lw, arrays["gp"], arrays["tau"], arrays["gamma"], arrays["period"], qp.MU_GP)
        value_only = h.lnlike_qp(lw, arrays["gp"], arrays["tau"], arrays["gamma"], arrays["period"], qp.MU_GP)
    assert np.isneginf(res[0][1]) and np.isneginf(value_only[1])
    assert all(np.all(np.isnan(v[1])) for v in res[1:])
    keep = [0, 2]
    assert np.all(np.isfinite(good[0]))
    assert _same_bits([v[keep] for v in res], [v[keep] for v in good])
    assert _same_bits([value_only[keep]], [good[0][keep]])


def test_a_matrix_that_does_not_factor_gives_minus_inf_there_and_leaves_the_others():
    """zero noise and two identical pixels at one time (the degenerate input of tests/test_gpu_marg_grad.py) between two
    proposals whose pixels lie far apart, so that K is nearly diagonal and factors without noise"""
    d = qp.case_data(qp.CASES[0])
    from psoap_amd.chunk import ChunkHandle
    N = d.lwls.shape[1]
    far = d.lwls + 1e-3 * np.arange(N)[None, :]
    lw = d.lwls.copy()
    lw[:, 1] = lw[:, 0]
    times = d.times.copy()
    times[1] = times[0]
    gamma = np.array([1.5, 0.4])
    rep = lambda v: np.stack([v, v, v])      # noqa: E731
    with ChunkHandle(d.fl, np.zeros_like(d.sigma)) as h:
        h.set_times(times)
        solo = h.lnlike_qp_grad(far, d.gp, d.tau, gamma, d.period, qp.MU_GP)
        out = h.lnlike_qp_grad(np.stack([far, lw, far]), rep(d.gp), rep(d.tau), rep(gamma), rep(d.period), qp.MU_GP)
    assert np.isfinite(solo[0]) and out[0][1] == -np.inf and all(np.all(np.isnan(v[1])) for v in out[1:])
    assert _same_bits([v[0] for v in out], solo) and _same_bits([v[2] for v in out], solo)


def test_conventions_null_outputs_missing_times_stream_baseline_release():
    from psoap_amd._lib import PsoapError, check, dptr
    from psoap_amd.chunk import ChunkHandle
    d = qp.case_data(qp.CASES[0])
    lw, gps, taus, gams, pers = _proposals(d, 3, 9700)
    N = d.lwls.shape[1]
    with ChunkHandle(d.fl, d.sigma) as h:
        with pytest.raises(PsoapError, match="psoap_chunk_set_times"):
            h.lnlike_qp_grad(lw, gps, taus, gams, pers, qp.MU_GP)
        with pytest.raises(PsoapError, match="psoap_chunk_set_times"):
            h.lnlike_qp(lw, gps, taus, gams, pers, qp.MU_GP)
        h.set_times(d.times)
        full = h.lnlike_qp_grad(lw, gps, taus, gams, pers, qp.MU_GP)
        # NULL for the optional outputs: the same bits in the others
        lnp2, g2 = np.empty(3), np.empty((3, 4))
        t2, m2, p2 = np.empty((3, 2)), np.empty((3, 2)), np.empty((3, 2))
        call = h._L.psoap_chunk_lnlike_qp_grad
        head = (h._h, 3, 2, dptr(lw), dptr(gps), dptr(taus), dptr(gams), dptr(pers), qp.MU_GP, dptr(lnp2))
        check(call(*head, dptr(g2), dptr(t2), dptr(m2), dptr(p2), None, None), "psoap_chunk_lnlike_qp_grad")
        assert _same_bits([lnp2, g2, t2, m2, p2], full[:5])
        # value only: the other gradients must be NULL too; with grad_gp the three temporal gradients are required
        assert call(*head, None, None, None, dptr(p2), None, None) != 0 and b"grad_gp == NULL" in h._L.psoap_last_error()
        assert call(*head, dptr(g2), dptr(t2), None, dptr(p2), None, None) != 0 and b"go with grad_gp" in h._L.psoap_last_error()
        assert call(h._h, 0, 2, *head[3:], None, None, None, None, None, None) != 0 and b"B must be" in h._L.psoap_last_error()
        # an open stream refuses the call
        h.stream_open(2, 1)
        try:
            with pytest.raises(PsoapError, match="open stream"):
                h.lnlike_qp_grad(lw, gps, taus, gams, pers, qp.MU_GP)
        finally:
            h.stream_close()
        # release twice, then another call: the workspace comes back, the times stayed, and so do the bits
        h.grad_release()
        h.grad_release()
        assert _same_bits(h.lnlike_qp_grad(lw[0], gps[0], taus[0], gams[0], pers[0], qp.MU_GP), [v[0] for v in full])
        # the time-variable call after the quasi-periodic one on the same workspace, and back
        tv_first = h.lnlike_tv_grad(lw, gps, taus, qp.MU_GP)
        assert _same_bits(h.lnlike_qp_grad(lw, gps, taus, gams, pers, qp.MU_GP), full)
        assert _same_bits(h.lnlike_tv_grad(lw, gps, taus, qp.MU_GP), tv_first)
        # a handle with a baseline is refused
        ch = gr.case_chunk(qp.CASES[0][1])
        h.set_baseline(1, ch.lwl, ch.epoch_index, ch.n_epochs, [0.1, 0.1])
        with pytest.raises(PsoapError, match="baseline"):
            h.lnlike_qp_grad(lw, gps, taus, gams, pers, qp.MU_GP)
    assert full[5].shape == (3, 2, N)


def test_times_need_not_be_sorted_a_permuted_chunk_gives_the_permuted_gradient():
    """rule 5, as test_gpu_timevar.py asks it of the time-variable kernel: the permuted case against the same chunk in epoch
    order (another summation order: the value to 1e-10 relative, the gradients to twice the bound of the table)"""
    case = qp.CASES[7]
    d = qp.case_data(case)
    perm = np.random.default_rng(7200 + 300 + 2).permutation(d.lwls.shape[1])
    inv = np.argsort(perm)
    with _handle(d) as h:
        p = _got(h.lnlike_qp_grad(d.lwls, d.gp, d.tau, d.gamma, d.period, qp.MU_GP))
    from psoap_amd.chunk import ChunkHandle
    with ChunkHandle(d.fl[inv], d.sigma[inv]) as h:
        h.set_times(d.times[inv])
        s = _got(h.lnlike_qp_grad(d.lwls[:, inv], d.gp, d.tau, d.gamma, d.period, qp.MU_GP))
    assert np.all(np.diff(d.times[inv]) >= 0)
    ref = qp.case_ext(case)
    assert abs(p.lnp - s.lnp) <= LNP_RTOL * max(1.0, abs(s.lnp))
    assert gr.rel_to_scale(p.gp, s.gp, ref.s_gp) <= 2 * TOL["gp"] and tv.rel_tau(p.tau, s.tau, ref.s_tau) <= 2 * TOL["tau"]
    assert tv.rel_tau(p.gamma, s.gamma, ref.s_gamma) <= 2 * TOL["gamma"]
    assert tv.rel_tau(p.period, s.period, ref.s_period) <= 2 * TOL["period"]
    assert gr.rel_to_scale(p.lwl[:, inv], s.lwl, ref.s_lwl[:, inv]) <= 2 * TOL["lwl"]


# ---- the gradient is the gradient of the value ---------------------------------------------------------------------------------
def test_grad_gamma_and_grad_period_are_central_differences_of_the_value():
    """N128-c2 (both Gammas > 0, one P longer than the span): D(h) = (f(x + h e_k) - f(x - h e_k)) / 2h of ``lnlike_qp`` in
    x = (log Gamma, log P) against theta_k dlnL/dtheta_k of ``lnlike_qp_grad``.

    The step and the bound come from the float64 twin alone, as profiles/marg_timevar.md derives them.  D(h) has the
    truncation error |f'''| h^2 / 6 and carries the value's rounding noise eps / h; eps is the measured noise of a float64
    lnp -- LNP_F64_MAX max(1, |f|), the lnp column of the table above -- not its last bit.  f''' per parameter is the second
    central difference (step 1e-3) of the twin's ANALYTIC gradient, h = (3 eps / |f'''|)^(1/3) minimises the sum, and the
    device gets MARGIN times the twin's own |D(h) - analytic|."""
    d = qp.case_data(qp.CASES[1])
    x0 = np.concatenate([np.log(d.gamma), np.log(d.period)])

    def unpack(x):
        return np.exp(x[:2]), np.exp(x[2:])

    def twin(x):
        g, p = unpack(x)
        r = qp.qp_f64(d.lwls, d.times, d.fl, d.sigma, d.gp, d.tau, g, p, qp.MU_GP)
        return r.lnp, np.concatenate([r.gamma * g, r.period * p])

    f0, g0 = twin(x0)
    eps = LNP_F64_MAX * max(1.0, abs(f0))
    with _handle(d) as h:
        res = _got(h.lnlike_qp_grad(d.lwls, d.gp, d.tau, d.gamma, d.period, qp.MU_GP))
        analytic = np.concatenate([res.gamma * d.gamma, res.period * d.period])
        for k in range(x0.size):
            e = np.zeros(x0.size)
            e[k] = 1.0
            d3 = abs(twin(x0 + 1e-3 * e)[1][k] - 2 * g0[k] + twin(x0 - 1e-3 * e)[1][k]) / 1e-6
            step = (3 * eps / d3) ** (1.0 / 3.0)
            e_twin = abs((twin(x0 + step * e)[0] - twin(x0 - step * e)[0]) / (2 * step) - g0[k])
            bound = MARGIN * e_twin
            up, dn = unpack(x0 + step * e), unpack(x0 - step * e)
            D = (h.lnlike_qp(d.lwls, d.gp, d.tau, up[0], up[1], qp.MU_GP) - h.lnlike_qp(d.lwls, d.gp, d.tau, dn[0], dn[1], qp.MU_GP)) / (2 * step)
            print(f"x[{k}]: analytic {analytic[k]:+.9e} difference {D:+.9e} step {step:.2e} |f'''| {d3:.2e} twin's own error "
                  f"{e_twin:.2e} device |analytic - difference| {abs(analytic[k] - D):.2e} bound {bound:.2e}")
            assert abs(analytic[k] - D) <= bound, (k, analytic[k], D, bound)


# ---- the fit, the scan, the statistic ------------------------------------------------------------------------------------------
def test_optimize_GP_quasiperiodic_agrees_with_the_same_driver_on_the_float64_twin_and_the_scan_peaks_at_the_planted_period():
    """``quasiperiodic_reference.fit_case(True)``: N = 300 over 12 epochs, P_0 = span / 4.3 planted in component 0.
    ``optimize_GP_quasiperiodic`` on the device and the same driver on the twin (``fit_on_twin``) start from the same point,
    10 % off in P.  Asserted: agreement with the twin, to the bounds of test_gpu_timevar.py's fit -- the optimum's lnp 1e-8
    relative; the parameters: both runs end within delta = 1e-8 |lnp| of the maximum, and near a maximum with Hessian H (of
    -lnL in the log parameters) a deficit delta confines a point to |x - x*| <= sqrt(2 delta / lambda_min(H)), two such points
    to twice that; H from central differences (step 1e-4) of the twin's own analytic gradient at the twin's optimum.
    The periodicity statistic lnp - lnp_timevar is positive (the twin's is, by tens); ``period_scan`` over 31 trial periods
    peaks at the grid point nearest P_0 (the twin's scan does), and the score at Gamma = 0 is positive there."""
    from psoap_amd import covariance
    fc = qp.fit_case(True)
    gp_t, tau_t, gam_t, per_t, lnp_t, lnp0_t, lnptv_t, res_t = qp.fit_on_twin(True)
    try:
        gp_d, tau_d, gam_d, per_d, lnp_d, lnp0_d, lnptv_d, res_d = covariance.optimize_GP_quasiperiodic(
            fc.lwls, fc.fl, fc.sigma, *fc.start, fc.times, full_output=True)
        grid = fc.P0 * np.linspace(0.5, 2.0, 31)
        truth = fc.truth
        scan, score = covariance.period_scan(fc.lwls, fc.fl, fc.sigma, truth[0], truth[1], truth[2], fc.times, grid)
    finally:
        covariance.release_handles()
    x_t = np.concatenate([np.log(gp_t), np.log([tau_t[0], gam_t[0], per_t[0]])])
    x_d = np.concatenate([np.log(gp_d), np.log([tau_d[0], gam_d[0], per_d[0]])])
    vg = qp.fit_twin(fc)

    def grad_log(x):
        gp = np.exp(x[:4])
        tau, gam, per = np.array([np.exp(x[4]), INF]), np.array([np.exp(x[5]), 0.0]), np.array([np.exp(x[6]), 1.0])
        _, g_gp, g_tau, g_gam, g_per = vg(gp, tau, gam, per)
        return -np.concatenate([g_gp * gp, [g_tau[0] * tau[0], g_gam[0] * gam[0], g_per[0] * per[0]]])

    step = 1e-4
    H = np.empty((7, 7))
    for k in range(7):
        e = np.zeros(7)
        e[k] = step
        H[k] = (grad_log(x_t + e) - grad_log(x_t - e)) / (2 * step)
    lam = float(np.linalg.eigvalsh(0.5 * (H + H.T)).min())
    delta = 1e-8 * abs(lnp_t)
    bound = 2.0 * np.sqrt(2.0 * delta / lam) if lam > 0 else float("nan")
    twin_scan = np.array([vg(truth[0], truth[1], truth[2], np.array([p, 1.0]))[0] for p in grid])
    nearest = int(np.argmin(np.abs(grid - fc.P0)))
    print(f"device: gp {gp_d} tau {tau_d} gamma {gam_d} period {per_d} lnp {lnp_d!r} in {res_d.nfev} evaluations; twin: gp {gp_t} "
          f"tau {tau_t} gamma {gam_t} period {per_t} lnp {lnp_t!r} in {res_t.nfev}; planted P_0 {fc.P0:.4f}; lambda_min {lam:.3e}, "
          f"|dx| {np.linalg.norm(x_d - x_t):.3e} (bound {bound:.3e}); statistic device {lnp_d - lnptv_d:.4f} twin "
          f"{lnp_t - lnptv_t:.4f}; lnp at gamma = 0 device {lnp0_d:.4f} twin {lnp0_t:.4f}; scan peak {grid[int(np.argmax(scan))]:.4f} "
          f"(twin {grid[int(np.argmax(twin_scan))]:.4f}), score at the peak {score[nearest]:.4e}")
    assert tau_d[1] == INF and gam_d[1] == 0.0 and per_d[1] == 1.0 and np.all(gp_d > 0)
    assert abs(lnp_d - lnp_t) <= 1e-8 * abs(lnp_t)
    assert lam > 0, "the twin's optimum is no maximum in the free parameters"
    assert np.linalg.norm(x_d - x_t) <= bound
    assert lnp_t - lnptv_t > 0 and lnp_d - lnptv_d > 0
    assert abs(lnptv_d - lnptv_t) <= 1e-8 * abs(lnptv_t) and abs(lnp0_d - lnp0_t) <= 1e-8 * abs(lnp0_t)
    assert int(np.argmax(twin_scan)) == nearest and int(np.argmax(scan)) == nearest
    assert np.max(np.abs(scan - twin_scan) / np.maximum(1.0, np.abs(twin_scan))) <= LNP_RTOL
    assert score.shape == (31,) and score[nearest] > 0


def test_on_a_chunk_drawn_with_zero_gamma_the_periodicity_statistic_is_not_positive():
    """``fit_case(False)``: the same draw with Gamma = 0.  What the twin shows (tests/test_quasiperiodic_reference.py holds it
    on the CPU): the fit drives Gamma towards 0, where the model is the time-variable one, the score d lnp / d Gamma at
    Gamma = 0 at the planted period is negative -- a periodic factor loses to first order -- and the statistic is not positive
    beyond what the two fits' convergence leaves open, delta = 1e-8 |lnp| each way (the bound the fit test above puts on a
    converged lnp).  The device is asked for the same three things."""
    from psoap_amd import covariance
    fc = qp.fit_case(False)
    gp_t, tau_t, gam_t, per_t, lnp_t, lnp0_t, lnptv_t, res_t = qp.fit_on_twin(False)
    try:
        gp_d, tau_d, gam_d, per_d, lnp_d, lnp0_d, lnptv_d, res_d = covariance.optimize_GP_quasiperiodic(
            fc.lwls, fc.fl, fc.sigma, *fc.start, fc.times, full_output=True)
        _scan, score = covariance.period_scan(fc.lwls, fc.fl, fc.sigma, fc.truth[0], fc.truth[1], fc.truth[2], fc.times,
                                              np.array([fc.P0]))
    finally:
        covariance.release_handles()
    delta = 1e-8 * abs(lnp_t)
    print(f"device: gamma {gam_d} period {per_d} lnp {lnp_d!r} lnp_timevar {lnptv_d!r} statistic {lnp_d - lnptv_d:.3e}; twin: gamma "
          f"{gam_t} period {per_t} lnp {lnp_t!r} lnp_timevar {lnptv_t!r} statistic {lnp_t - lnptv_t:.3e}; delta {delta:.3e}; score "
          f"at P_0 {score[0]:.4e}")
    assert lnp_t - lnptv_t <= delta and gam_t[0] < 1e-3
    assert lnp_d - lnptv_d <= delta and gam_d[0] < 1e-3
    assert score[0] < 0
