"""GPU tests of the time-variable kernel under the marginalised continuum (psoap_chunk_lnlike_marg_tv,
psoap_chunk_lnlike_marg_tv_grad, psoap_chunk_fisher_marg_tv; k_marg_tv_grad_contract in psoap_amd/csrc/marg_grad_kernels.hpp,
the runs of analysis_host.hpp with ``marg && tv``).

The cases are those of tests/marg_reference.py (N = 100, 128, 129, 384, 300 with an empty epoch, 312 with Q = 2), each with
weight = None and weight = fl, the times the dates of the chunk each case is cut from, tau per component a finite fraction of
the span (0.25 or 2) mixed with inf where c > 1 (tests/marg_tv_reference.py).  The reference is the long-double evaluation on
the dense K_tv + H Lambda H^T (marg_tv_reference.marg_tv_ext): ``lnp`` at the relative 1e-10 of the sibling tests, the value
side in the measures of tests/test_gpu_marg.py, the gradients relative to the cancellation scale
S = 1/2 sum_ij |Q_m,ij| |dK_ij/dtheta| (sum_i |alpha_m,i| for mu_GP), F relative to sqrt(F_ss F_tt).

The tolerance is derived, not fitted: the float64 SciPy evaluation of the device's own route (marg_tv_reference.marg_tv_f64)
measured against the long-double one on these very cases (python tests/marg_tv_reference.py), the largest over the twelve
case-weight pairs -- the table's last row, ``marg_tv_reference.F64_MAX``, restated in ``F64`` below (the whole table:
profiles/marg_timevar.md).  The device sums in another order and fuses multiply-adds but is fp64 throughout: it gets each figure
times the project's margin of 8 (tests/test_gpu_grad.py).  The four seeded defects of tests/test_marg_tv_reference.py miss the
bound on grad_tau by factors of 1e9 and more.

Measured on the device (MI355X), the largest over the twelve case-weight pairs: lnp 1.18e-14, quad 2.69e-14, logdet_K 1.70e-15,
gain 5.18e-13, logdet_M 2.25e-13, beta 8.61e-13, beta_cov 3.78e-12, fl_cor 1.24e-12, grad_gp 1.03e-15, grad_tau 1.37e-15,
grad_mu 1.22e-15, grad_lwl 2.65e-12, F 8.54e-13, F_mu 1.63e-14 (profiles/marg_timevar.md has them beside the bounds).
"""
import ctypes

import numpy as np
import pytest

import marg_reference as mr
import marg_tv_reference as mt
import timevar_reference as tr
from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu

LNP_RTOL = 1e-10
MARGIN = 8
# python tests/marg_tv_reference.py, last row (max over the cases and weights of |f64 - long double| in each output's measure)
F64 = {"quad": 1.20e-14, "logdet_K": 1.27e-15, "gain": 5.59e-12, "logdet_M": 5.18e-13, "beta": 1.07e-12, "beta_cov": 3.71e-12,
       "fl_cor": 1.62e-12, "grad_gp": 8.23e-16, "grad_tau": 4.71e-15, "grad_mu": 6.18e-15, "grad_lwl": 3.17e-12, "F": 5.94e-13,
       "F_mu": 3.60e-14}
TOL = {k: MARGIN * v for k, v in F64.items()}
INF = float("inf")
dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))      # noqa: E731


def test_the_bounds_are_the_reference_modules():
    assert F64 == mt.F64_MAX and MARGIN == mt.MARGIN and LNP_RTOL == mt.LNP_RTOL


def _handle(case, kind, times=True, baseline=True, **kw):
    from psoap_amd.chunk import ChunkHandle
    ch = mr.case_chunk(case)
    h = ChunkHandle(ch.fl, ch.sigma, **kw)
    if times:
        h.set_times(mt.case_times(case)[0])
    if baseline:
        h.set_baseline(ch.order, ch.x, ch.epoch_index, ch.n_epochs, mr.prior_sd(ch.order), mr.case_weight(case, kind))
    return h


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).copy()


def _same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _marg_fields(r):
    return [r.lnp, r.parts, r.beta, r.beta_cov, r.fl_cor]


class _Got:
    def __init__(self, value, grad, F=None, F_mu=None):
        self.lnp, self.parts, self.beta, self.beta_cov, self.fl_cor = _marg_fields(value)
        _, self.gp, self.tau, self.lwl, self.mu = grad
        self.F, self.F_mu = F, F_mu


# ---- 1: value and gradient against long double ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", mr.WEIGHTS)
@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_id)
def test_value_and_gradient_against_long_double_and_value_bits(case, kind):
    ch, gp, c, tau = mr.case_chunk(case), mr.case_gp(case), case[2], mt.case_tau(case)
    ref = mt.case_ext(case, kind)
    with _handle(case, kind) as h:
        value = h.lnlike_marg_tv(ch.lwls, gp, tau, mt.MU_GP, want_beta=True, want_cov=True, want_flux=True)
        bare = h.lnlike_marg_tv(ch.lwls, gp, tau, mt.MU_GP)
        grad = h.lnlike_marg_tv_grad(ch.lwls, gp, tau, mt.MU_GP)
        lw, lnp, parts, g_gp, g_tau = np.ascontiguousarray(ch.lwls), np.empty(1), np.empty(4), np.empty(2 * c), np.empty(c)
        assert h._L.psoap_chunk_lnlike_marg_tv_grad(h._h, 1, c, dp(lw), dp(gp), dp(tau), mt.MU_GP, dp(lnp), dp(parts), dp(g_gp),
                                                    dp(g_tau), None, None) == 0
        lnp0, parts0 = np.empty(1), np.empty(4)
        assert h._L.psoap_chunk_lnlike_marg_tv_grad(h._h, 1, c, dp(lw), dp(gp), dp(tau), mt.MU_GP, dp(lnp0), dp(parts0), None, None,
                                                    None, None) == 0
    assert grad[1].shape == (2 * c,) and grad[2].shape == (c,) and grad[3].shape == ch.lwls.shape
    # lnp and the parts of the gradient entry, with or without the optional outputs, and of the value-only call: the bits of
    # the value entry, which does not depend on the outputs asked for either
    assert _same_bits([grad[0], lnp[0], parts, lnp0[0], parts0, bare], [value.lnp, value.lnp, value.parts, value.lnp, value.parts,
                                                                        value.lnp])
    assert _same_bits([g_gp, g_tau], [grad[1], grad[2]])
    assert np.all(grad[2][np.isinf(tau)] == 0.0) and np.all(grad[2][np.isfinite(tau)] != 0.0)
    err = mt.errors(_Got(value, grad), ref, mr.prior_sd(case[5]), want_fisher=False)
    print(f"{mr.case_id(case)}-{kind}: lnp {value.lnp!r} long double {ref.lnp!r}; " +
          ", ".join(f"{k} {v:.2e} ({TOL[k]:.2e})" for k, v in err.items() if k != "lnp") + f", lnp {err['lnp']:.2e}")
    assert abs(value.lnp - ref.lnp) <= LNP_RTOL * max(1.0, abs(ref.lnp))
    for k, v in err.items():
        if k != "lnp":
            assert v <= TOL[k], (k, v, TOL[k])


# ---- 2: tau = inf is the static marginal model, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_id)
def test_all_infinite_tau_has_the_bits_of_the_static_marginal_entries(case):
    ch, gp, c = mr.case_chunk(case), mr.case_gp(case), case[2]
    inf = np.full(c, INF)
    for kind in mr.WEIGHTS:
        with _handle(case, kind) as h:
            static = h.lnlike_marg(ch.lwls, gp, mt.MU_GP, want_beta=True, want_cov=True, want_flux=True)
            static_grad = h.lnlike_marg_grad(ch.lwls, gp, mt.MU_GP)
            value = h.lnlike_marg_tv(ch.lwls, gp, inf, mt.MU_GP, want_beta=True, want_cov=True, want_flux=True)
            lnp, g_gp, g_tau, g_lwl, g_mu = h.lnlike_marg_tv_grad(ch.lwls, gp, inf, mt.MU_GP)
            again = h.lnlike_marg_grad(ch.lwls, gp, mt.MU_GP)
        assert _same_bits(_marg_fields(value), _marg_fields(static)), kind
        assert _same_bits([lnp, g_gp, g_lwl, g_mu], static_grad) and _same_bits(again, static_grad), kind
        assert g_tau.shape == (c,) and np.all(g_tau == 0.0) and not np.any(np.signbit(g_tau))


# ---- 3: batches ---------------------------------------------------------------------------------------------------------------
def _proposals(case, B, seed):
    """B different proposals on the case's chunk: perturbed grids and hyper-parameters; tau rows that mix finite and inf --
    row b keeps the case's pattern, every third row swaps it, one row is all inf"""
    rng = np.random.default_rng(seed)
    ch, c = mr.case_chunk(case), case[2]
    span = mt.case_times(case)[1]
    lw = ch.lwls[None] + rng.normal(0.0, 2.0 / syn.C_KMS, size=(B, c, 1))
    gps = mr.case_gp(case)[None] * rng.uniform(0.8, 1.25, size=(B, 2 * c))
    taus = span * rng.uniform(0.2, 3.0, size=(B, c))
    mask = np.isinf(mt.case_tau(case))[None].repeat(B, axis=0)
    mask[::3] = ~mask[::3]
    taus[mask] = INF
    if B > 4:
        taus[4] = INF
    return np.ascontiguousarray(lw), np.ascontiguousarray(gps), np.ascontiguousarray(taus)


def test_batches_groups_repeats_and_the_entries_around_them_keep_the_bits():
    """case c (N = 129, c = 2), B = 10 (more than the 8 matrices of a group: 8 + 2) against B = 3 and single calls, a call
    repeated, the value entry; and a plain entry, a ``_tv`` entry on a second handle without a baseline and a ``_marg`` entry in
    between keep their own bits"""
    case = mr.case_named("c")
    ch, c = mr.case_chunk(case), case[2]
    lw, gps, taus = _proposals(case, 10, 9901)
    assert np.any(np.isinf(taus)) and np.any(np.isfinite(taus)) and np.all(np.isinf(taus[4]))
    with _handle(case, "flux", max_batch=10) as h, _handle(case, "flux", baseline=False) as h2:
        plain0 = h.lnlike_grad(lw[1], gps[1], mt.MU_GP)
        marg0 = h.lnlike_marg_grad(lw[1], gps[1], mt.MU_GP)
        tv0 = h2.lnlike_tv_grad(lw[1], gps[1], taus[1], mt.MU_GP)
        ten = h.lnlike_marg_tv_grad(lw, gps, taus, mt.MU_GP)
        plain1 = h.lnlike_grad(lw[1], gps[1], mt.MU_GP)
        again = h.lnlike_marg_tv_grad(lw, gps, taus, mt.MU_GP)
        tv1 = h2.lnlike_tv_grad(lw[1], gps[1], taus[1], mt.MU_GP)
        three = h.lnlike_marg_tv_grad(lw[:3], gps[:3], taus[:3], mt.MU_GP)
        marg1 = h.lnlike_marg_grad(lw[1], gps[1], mt.MU_GP)
        values = h.lnlike_marg_tv(lw, gps, taus, mt.MU_GP, want_beta=True)
        singles = [h.lnlike_marg_tv_grad(lw[b], gps[b], taus[b], mt.MU_GP) for b in range(10)]
        single_values = [h.lnlike_marg_tv(lw[b], gps[b], taus[b], mt.MU_GP, want_beta=True) for b in range(10)]
        static4 = h.lnlike_marg_grad(lw[4], gps[4], mt.MU_GP)
    N = ch.fl.shape[0]
    assert [v.shape for v in ten] == [(10,), (10, 2 * c), (10, c), (10, c, N), (10,)]
    assert len({float(v) for v in ten[0]}) == 10 and np.all(np.isfinite(ten[0]))
    assert _same_bits(ten, again) and _same_bits([values.lnp], [ten[0]])
    for b in range(10):
        one = [np.atleast_1d(v) for v in singles[b]]
        assert _same_bits([ten[k][b] for k in range(5)], one), b
        assert _same_bits([values.lnp[b], values.parts[b], values.beta[b]], [single_values[b].lnp, single_values[b].parts,
                                                                             single_values[b].beta]), b
        if b < 3:
            assert _same_bits([three[k][b] for k in range(5)], one), b
    # the all-inf row inside the batch: the static marginal gradient's bits, an exactly-zero grad_tau
    assert _same_bits([ten[0][4], ten[1][4], ten[3][4], ten[4][4]], static4) and np.all(ten[2][4] == 0.0)
    assert _same_bits(plain1, plain0) and _same_bits(marg1, marg0) and _same_bits(tv1, tv0)
    assert not _same_bits([marg0[1]], [plain0[1]])


# ---- 4: degenerate proposals inside a batch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ("tau_zero", "tau_negative", "tau_nan", "amplitude_negative"))
def test_a_degenerate_proposal_gives_minus_inf_there_and_leaves_its_neighbours(bad):
    case = mr.case_named("a")
    lw, gps, taus = _proposals(case, 3, 9902)
    gps2, taus2 = gps.copy(), taus.copy()
    if bad == "amplitude_negative":
        gps2[1, 0] = -gps2[1, 0]
    else:
        taus2[1, 1] = {"tau_zero": 0.0, "tau_negative": -3.0, "tau_nan": float("nan")}[bad]
    with _handle(case, "one", max_batch=3) as h:
        good = h.lnlike_marg_tv_grad(lw, gps, taus, mt.MU_GP)
        good_value = h.lnlike_marg_tv(lw, gps, taus, mt.MU_GP, want_beta=True, want_cov=True, want_flux=True)
        out = h.lnlike_marg_tv_grad(lw, gps2, taus2, mt.MU_GP)
        value = h.lnlike_marg_tv(lw, gps2, taus2, mt.MU_GP, want_beta=True, want_cov=True, want_flux=True)
        lnp, parts = np.empty(3), np.empty((3, 4))
        assert h._L.psoap_chunk_lnlike_marg_tv_grad(h._h, 3, 2, dp(lw), dp(gps2), dp(taus2), mt.MU_GP, dp(lnp), dp(parts), None, None,
                                                    None, None) == 0
        F = h.fisher_marg_tv(lw[1], gps2[1], taus2[1], np.eye(4), want_mu=True)
    assert np.all(np.isfinite(good[0]))
    assert np.isneginf(out[0][1]) and np.isneginf(value.lnp[1]) and np.isneginf(lnp[1]) and np.all(np.isnan(parts[1]))
    assert all(np.all(np.isnan(v[1])) for v in out[1:])
    assert all(np.all(np.isnan(v[1])) for v in _marg_fields(value)[1:])
    assert np.all(np.isnan(F[0])) and np.isnan(F[1])
    keep = [0, 2]
    assert _same_bits([v[keep] for v in out], [v[keep] for v in good])
    assert _same_bits([v[keep] for v in _marg_fields(value)], [v[keep] for v in _marg_fields(good_value)])
    assert _same_bits([lnp[keep], parts[keep]], [good[0][keep], good_value.parts[keep]])


def test_a_matrix_that_does_not_factor_inside_a_batch():
    """zero noise and two identical pixels (the degenerate input of tests/test_gpu_marg_grad.py), between two proposals whose
    pixels lie far apart"""
    from psoap_amd.chunk import ChunkHandle
    case = mr.case_named("a")
    ch, gp = mr.case_chunk(case), mr.case_gp(case)
    tau = mt.case_tau(case)
    lw = ch.lwls.copy()
    lw[:, 1] = lw[:, 0]
    t = mt.case_times(case)[0].copy()
    amp = gp.copy()
    amp[0] *= 1.5
    with ChunkHandle(ch.fl, np.zeros_like(ch.sigma)) as h:
        h.set_times(t)
        h.set_baseline(ch.order, ch.x, ch.epoch_index, ch.n_epochs, mr.prior_sd(ch.order), None)
        far = ch.lwls + 1e-3 * np.arange(ch.lwls.shape[1])[None, :]
        solo = h.lnlike_marg_tv_grad(far, amp, tau, mt.MU_GP)
        out = h.lnlike_marg_tv_grad(np.stack([far, lw, far]), np.stack([amp, gp, amp]), np.stack([tau] * 3), mt.MU_GP)
    assert np.isfinite(solo[0]) and out[0][1] == -np.inf and all(np.all(np.isnan(v[1])) for v in out[1:])
    assert _same_bits([v[0] for v in out], solo) and _same_bits([v[2] for v in out], solo)


# ---- 5: refusals and release ------------------------------------------------------------------------------------------------------
def test_refusals_and_release():
    from psoap_amd._lib import PsoapError, load
    case = mr.case_named("c")
    ch, gp, c, tau = mr.case_chunk(case), mr.case_gp(case), case[2], mt.case_tau(case)
    last = lambda: load().psoap_last_error()      # noqa: E731
    lw, lnp, g, gt, F = np.ascontiguousarray(ch.lwls), np.empty(1), np.empty(2 * c), np.empty(c), np.empty((1, 1))
    tan = np.zeros((1, 2 * c))
    tan[0, 0] = 1.0

    def raw_value(h, B=1):
        return h._L.psoap_chunk_lnlike_marg_tv(h._h, B, c, dp(lw), dp(gp), dp(tau), mt.MU_GP, dp(lnp), None, None, None, None)

    def raw_grad(h, B=1, g_gp=g, g_tau=gt):
        opt = lambda a: None if a is None else dp(a)      # noqa: E731
        return h._L.psoap_chunk_lnlike_marg_tv_grad(h._h, B, c, dp(lw), dp(gp), dp(tau), mt.MU_GP, dp(lnp), None, opt(g_gp),
                                                    opt(g_tau), None, None)

    def raw_fisher(h, T=1):
        return h._L.psoap_chunk_fisher_marg_tv(h._h, c, dp(lw), dp(gp), dp(tau), T, None, dp(tan), None, dp(F), None)

    names = {raw_value: b"psoap_chunk_lnlike_marg_tv: ", raw_grad: b"psoap_chunk_lnlike_marg_tv_grad: ",
             raw_fisher: b"psoap_chunk_fisher_marg_tv: "}
    with _handle(case, "flux", times=False, baseline=False) as h:
        # before set_times (and before a baseline: the times are asked for first)
        for call, name in names.items():
            assert call(h) != 0 and last() == name + b"call psoap_chunk_set_times first"
        h.set_times(mt.case_times(case)[0])
        # without a baseline: the message of psoap_chunk_lnlike_marg
        for call, name in names.items():
            assert call(h) != 0 and last() == name + b"call psoap_chunk_set_baseline first"
        for method in (h.lnlike_marg_tv, h.lnlike_marg_tv_grad):
            with pytest.raises(PsoapError, match="set_baseline"):
                method(ch.lwls, gp, tau, mt.MU_GP)
        with pytest.raises(PsoapError, match="set_baseline"):
            h.fisher_marg_tv(ch.lwls, gp, tau, tan)
        h.set_baseline(ch.order, ch.x, ch.epoch_index, ch.n_epochs, mr.prior_sd(ch.order), ch.fl)
        good = h.lnlike_marg_tv_grad(ch.lwls, gp, tau, mt.MU_GP)
        good_F = h.fisher_marg_tv(ch.lwls, gp, tau, tan, want_mu=True)
        # B, c, T out of range; the NULL rules
        assert raw_value(h, 0) != 0 and last() == names[raw_value] + b"batch size outside [1, max_batch]"
        assert raw_value(h, 2) != 0 and last() == names[raw_value] + b"batch size outside [1, max_batch]"
        assert raw_grad(h, 0) != 0 and last() == names[raw_grad] + b"B must be at least 1"
        assert raw_fisher(h, 0) != 0 and last() == names[raw_fisher] + b"the number of tangents must be between 1 and 32"
        assert raw_fisher(h, 33) != 0 and last() == names[raw_fisher] + b"the number of tangents must be between 1 and 32"
        assert h._L.psoap_chunk_lnlike_marg_tv(h._h, 1, 4, dp(lw), dp(gp), dp(tau), mt.MU_GP, dp(lnp), None, None, None, None) != 0
        assert last() == names[raw_value] + b"number of components must be 1, 2 or 3"
        assert raw_grad(h, 1, None, gt) != 0 and b"grad_gp == NULL asks for the value only" in last()
        assert raw_grad(h, 1, g, None) != 0 and last() == names[raw_grad] + b"grad_tau goes with grad_gp"
        assert h._L.psoap_chunk_lnlike_marg_tv(h._h, 1, c, dp(lw), dp(gp), None, mt.MU_GP, dp(lnp), None, None, None, None) != 0
        assert last() == names[raw_value] + b"bad arguments"
        # an open stream
        h.stream_open(c, 1)
        try:
            for call, name in names.items():
                assert call(h) != 0 and last() == name + b"the handle has an open stream (psoap_stream_close first)"
        finally:
            h.stream_close()
        # the existing time-variable entries still refuse this handle, in their own words
        for call in (lambda: h.lnlike_tv_grad(ch.lwls, gp, tau, mt.MU_GP), lambda: h.lnlike_tv(ch.lwls, gp, tau, mt.MU_GP),
                     lambda: h.fisher_tv(ch.lwls, gp, tau, tan), lambda: h.loo_tv(ch.lwls, gp, tau, mt.MU_GP)):
            with pytest.raises(PsoapError, match="the time-variable kernel under the marginalised continuum is not built yet"):
                call()
        # releases, in any combination, then a call: the same bits; the times and the baseline stayed
        h.marg_release()
        assert _same_bits(h.lnlike_marg_tv_grad(ch.lwls, gp, tau, mt.MU_GP), good)
        h.grad_release()
        h.marg_release()
        h.fisher_release()
        assert _same_bits(h.fisher_marg_tv(ch.lwls, gp, tau, tan, want_mu=True), good_F)
        h.grad_release()
        assert _same_bits(h.lnlike_marg_tv_grad(ch.lwls, gp, tau, mt.MU_GP), good)
        # a set_data after a weighted baseline: refused, with the message of lnlike_marg
        h.set_data(ch.fl, ch.sigma)
        for call, name in names.items():
            assert call(h) != 0 and last().startswith(name + b"psoap_chunk_set_data changed the data") and b"set_baseline again" in last()


# ---- 6: the Fisher information -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", mr.WEIGHTS)
@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_id)
def test_fisher_against_long_double(case, kind):
    """the unit tangents of (gp, tau) and one grid tangent against the long-double F: relative to sqrt(F_ss F_tt), exact zeros
    in the rows and columns of a tau = inf; F == F^T bit for bit; a subsequence of the tangents gives the shared entries' bits"""
    ch, gp, c, tau = mr.case_chunk(case), mr.case_gp(case), case[2], mt.case_tau(case)
    tan_lwl, tan_gp, tan_tau = mt.case_tangents(case)
    ref = mt.case_ext(case, kind)
    sub = list(range(1, 3 * c + 1, 2))
    with _handle(case, kind) as h:
        F, F_mu = h.fisher_marg_tv(ch.lwls, gp, tau, tan_gp, tan_tau, tan_lwl, want_mu=True)
        Fs = h.fisher_marg_tv(ch.lwls, gp, tau, tan_gp[sub], tan_tau[sub], tan_lwl[sub])
    assert F.shape == (3 * c + 1,) * 2 and np.array_equal(_bits(F), _bits(F.T))
    assert np.array_equal(_bits(Fs), _bits(F[np.ix_(sub, sub)]))
    dead = 2 * c + np.flatnonzero(np.isinf(tau))
    assert np.all(F[dead, :] == 0.0) and np.all(F[:, dead] == 0.0)
    err = {"F": mt.tfr.rel_to_scale(F, ref.F), "F_mu": float(abs(np.longdouble(F_mu) - ref.F_mu) / ref.F_mu)}
    print(f"{mr.case_id(case)}-{kind}: " + ", ".join(f"{k} {v:.2e} ({TOL[k]:.2e})" for k, v in err.items()))
    for k, v in err.items():
        assert v <= TOL[k], (k, v, TOL[k])


@pytest.mark.parametrize("kind", mr.WEIGHTS)
@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_id)
def test_fisher_at_infinite_tau_has_the_bits_of_fisher_marg(case, kind):
    ch, gp, c = mr.case_chunk(case), mr.case_gp(case), case[2]
    tan_lwl, tan_gp, tan_tau = mt.case_tangents(case)
    shared = [k for k in range(3 * c + 1) if not 2 * c <= k < 3 * c]
    with _handle(case, kind) as h:
        static, static_mu = h.fisher_marg(ch.lwls, gp, tan_gp[shared], tan_lwl[shared], want_mu=True)
        F, F_mu = h.fisher_marg_tv(ch.lwls, gp, np.full(c, INF), tan_gp, tan_tau, tan_lwl, want_mu=True)
        # ... whatever tan_tau holds: its coefficient is 0
        G = h.fisher_marg_tv(ch.lwls, gp, np.full(c, INF), tan_gp[shared], np.ones((len(shared), c)), tan_lwl[shared])
    assert np.array_equal(_bits(F[np.ix_(shared, shared)]), _bits(static)) and np.array_equal(_bits(G), _bits(static))
    assert _same_bits([F_mu], [static_mu])
    assert np.all(F[2 * c:3 * c, :] == 0.0) and np.all(F[:, 2 * c:3 * c] == 0.0)


# ---- 7: the gradient is the gradient of the value --------------------------------------------------------------------------------------
def test_gradient_is_the_central_difference_of_the_value_in_log_parameters():
    """Case a, weight = fl: D(h) = (f(x + h e_k) - f(x - h e_k)) / 2h of ``lnlike_marg_tv`` in x = (log gp, log tau[finite])
    against theta_k dlnL/dtheta_k of ``lnlike_marg_tv_grad``.

    The step and the bound come from the float64 twin alone.  D(h) has the truncation error |f'''| h^2 / 6 and carries the
    value's rounding noise eps / h.  eps is what a float64 evaluation of lnp is measured to be away from long double,
    marg_tv_reference.LNP_F64_MAX max(1, |f|) (8.16e-14 relative: the lnp column of the table the tolerances come from) -- not
    the last bit of lnp: a step sized for half an ulp of noise (1e-5 .. 4e-5) leaves D(h) all noise, two evaluations with
    different summation orders then differ by whatever their noise happens to be, and MARGIN times the twin's draw does not
    bound the device's (measured so: log l_0 1.02e-8 against 8 x 1.20e-9).  f''' per parameter is the second central difference (step 1e-3) of the twin's ANALYTIC gradient, and
    h = (3 eps / |f'''|)^(1/3) minimises the sum.  The twin's own D(h) misses the twin's analytic gradient by e_twin; the
    device, whose value has another but equally fixed summation order, gets MARGIN times e_twin."""
    case, kind = mr.case_named("a"), "flux"
    ch, gp, tau = mr.case_chunk(case), mr.case_gp(case), mt.case_tau(case)
    finite = np.flatnonzero(np.isfinite(tau))
    x0 = np.concatenate([np.log(gp), np.log(tau[finite])])
    args = mt.case_args(case, kind)

    def unpack(x):
        t = tau.copy()
        t[finite] = np.exp(x[4:])
        return np.exp(x[:4]), t

    def twin(x):
        g, t = unpack(x)
        r = mt.marg_tv_f64(*args[:4], g, t, *args[6:], tangents=([], [], []))
        return r.lnp, np.concatenate([r.gp * g, r.tau[finite] * t[finite]])

    f0, g0 = twin(x0)
    eps = mt.LNP_F64_MAX * max(1.0, abs(f0))
    with _handle(case, kind) as h:
        lnp, g_gp, g_tau, _, _ = h.lnlike_marg_tv_grad(ch.lwls, gp, tau, mt.MU_GP)
        analytic = np.concatenate([g_gp * gp, g_tau[finite] * tau[finite]])
        for k in range(x0.size):
            e = np.zeros(x0.size)
            e[k] = 1.0
            d3 = abs(twin(x0 + 1e-3 * e)[1][k] - 2 * g0[k] + twin(x0 - 1e-3 * e)[1][k]) / 1e-6
            step = (3 * eps / d3) ** (1.0 / 3.0)
            e_twin = abs((twin(x0 + step * e)[0] - twin(x0 - step * e)[0]) / (2 * step) - g0[k])
            bound = MARGIN * e_twin
            up, dn = unpack(x0 + step * e), unpack(x0 - step * e)
            D = (h.lnlike_marg_tv(ch.lwls, up[0], up[1], mt.MU_GP) - h.lnlike_marg_tv(ch.lwls, dn[0], dn[1], mt.MU_GP)) / (2 * step)
            print(f"x[{k}]: analytic {analytic[k]:+.9e} difference {D:+.9e} step {step:.2e} |f'''| {d3:.2e} twin's own error "
                  f"{e_twin:.2e} device |analytic - difference| {abs(analytic[k] - D):.2e} bound {bound:.2e}")
            assert abs(analytic[k] - D) <= bound, (k, analytic[k], D, bound)
    assert lnp == h_value_bits(case, kind, gp, tau)


def h_value_bits(case, kind, gp, tau):
    with _handle(case, kind) as h:
        return h.lnlike_marg_tv(mr.case_chunk(case).lwls, gp, tau, mt.MU_GP)


# ---- 8: the fit -------------------------------------------------------------------------------------------------------------------
def test_optimize_GP_timevar_marginal_agrees_with_the_same_driver_on_the_float64_twin():
    """``marg_reference.planted()``: a static SB2 model plus a per-epoch linear continuum drawn from the prior (N = 240, six
    epochs).  ``optimize_GP_timevar_marginal`` on the device and the same L-BFGS-B driver (covariance._fit_timevar) on
    ``marg_tv_f64`` start from the same point; the first component's tau is free, the second held at inf.

    The bounds are those of tests/test_gpu_timevar.py's fit: the optimum's lnp to 1e-8 relative; both runs end within
    delta = 1e-8 |lnp| of the maximum, and near a maximum with Hessian H of -lnL in the log-parameters a deficit delta confines a
    point to |x - x*| <= sqrt(2 delta / lambda_min(H)), two such points to twice that; H from central differences (step 1e-4)
    of the twin's analytic gradient at the twin's optimum.  The truth is static, so under the baseline the fit walks tau out
    towards infinity until the gradient is below L-BFGS-B's threshold: the twin ends at 1e5 spans with lambda_min 1.2e-7 -- the
    tau direction is flat there and the bound on |dx| is wide in it (about 20 in log tau); the other four eigenvalues are 30
    and more.

    ``timevar_laplace(..., baseline=...)`` against the twin's Fisher matrix through the same algebra, at the START of the fit
    (gp0, tau0 = half the span): at the optimum F_tau,tau is 1e-30 of the other entries, no measure relative to
    sqrt(F_ss F_tt) means anything and the Laplace covariance is singular to rounding.  F to the Fisher tolerance, twice over:
    the twin is that far from long double itself.

    The variability statistic lnp - lnp(tau = inf) with and without the baseline.  The twin on the CPU: 226.75 without the
    baseline -- a finite tau absorbs the planted per-epoch continuum -- and -3e-8 with it (profiles/marg_timevar.md): the
    baseline removes the spurious gain by nine orders of magnitude, so the device is asked for the same direction, the twin's
    values the reference: without the baseline at least half the twin's gain, with it less than a thousandth of that."""
    from psoap_amd import covariance
    ch, gp_true, _beta = mr.planted()
    times, span = mt.planted_times()
    t0 = times - times.min()
    base = dict(x=ch.x, epoch_index=ch.epoch_index, order=1, prior_sd=mr.PLANT_SD)
    margs = (ch.x, ch.epoch_index, ch.n_epochs, 1, mr.PLANT_SD, None, mr.MU_GP)
    gp0, tau0, free = gp_true * np.array([1.3, 0.8, 0.8, 1.25]), np.array([0.5 * span, INF]), [True, False]

    def twin(gp, tau):
        r = mt.marg_tv_f64(ch.lwls, t0, ch.fl, ch.sigma, gp, tau, *margs, tangents=([], [], []))
        return r.lnp, r.gp, r.tau

    def twin_plain(gp, tau):
        r = tr.tv_f64(ch.lwls, t0, ch.fl, ch.sigma, gp, tau, mr.MU_GP)
        return r.lnp, r.gp, r.tau

    gp_t, tau_t, res_t = covariance._fit_timevar(twin, 2, gp0, tau0, free, 1e-10)
    lnp_t = -float(res_t["fun"])
    stat_t = lnp_t - twin(gp_t, np.full(2, INF))[0]
    gp_p, tau_p, res_p = covariance._fit_timevar(twin_plain, 2, gp0, tau0, free, 1e-10)
    stat_t_plain = -float(res_p["fun"]) - twin_plain(gp_p, np.full(2, INF))[0]
    try:
        gp_d, tau_d, lnp_d, lnp_static, res_d = covariance.optimize_GP_timevar_marginal(ch.lwls, ch.fl, ch.sigma, gp0, tau0, times,
                                                                                        base, free_tau=free, mu_GP=mr.MU_GP,
                                                                                        full_output=True)
        value_d = covariance.lnlike_timevar_marginal(ch.lwls, ch.fl, ch.sigma, gp_d, tau_d, times, base, mr.MU_GP)
        # (the baseline off on the same chunk, then on again: the statistic both ways from one session)
        _, tau_dp, lnp_dp, static_dp, _ = covariance.optimize_GP_timevar(ch.lwls, ch.fl, ch.sigma, gp0, tau0, times, free_tau=free,
                                                                         mu_GP=mr.MU_GP, full_output=True)
        value_again = covariance.lnlike_timevar_marginal(ch.lwls, ch.fl, ch.sigma, gp_d, tau_d, times, base, mr.MU_GP)
        static_marg = covariance.lnlike_marginal(ch.lwls, ch.fl, ch.sigma, gp_d, ch.x, ch.epoch_index, 1, mr.PLANT_SD, None, mr.MU_GP)
        cov_d, sd_gp_d, sd_tau_d = covariance.timevar_laplace(ch.lwls, ch.fl, ch.sigma, gp0, tau0, times, free_tau=free,
                                                              baseline=base)
        F_d = covariance.fisher_information_timevar(ch.lwls, ch.fl, ch.sigma, gp0, tau0, times, baseline=base)
    finally:
        covariance.release_handles()
    x_t = np.concatenate([np.log(gp_t), np.log(tau_t[:1])])
    x_d = np.concatenate([np.log(gp_d), np.log(tau_d[:1])])

    def grad_log(x):
        gp, tau = np.exp(x[:4]), np.array([np.exp(x[4]), INF])
        _, g_gp, g_tau = twin(gp, tau)
        return -np.concatenate([g_gp * gp, g_tau[:1] * tau[:1]])

    step = 1e-4
    H = np.empty((5, 5))
    for k in range(5):
        e = np.zeros(5)
        e[k] = step
        H[k] = (grad_log(x_t + e) - grad_log(x_t - e)) / (2 * step)
    lam = float(np.linalg.eigvalsh(0.5 * (H + H.T)).min())
    delta = 1e-8 * abs(lnp_t)
    bound = 2.0 * np.sqrt(2.0 * delta / lam) if lam > 0 else float("nan")
    F_t = mt.marg_tv_f64(ch.lwls, t0, ch.fl, ch.sigma, gp0, tau0, *margs).F
    cov_t, sd_gp_t, sd_tau_t = covariance._laplace_from_fisher(F_t, gp0, tau0, free)
    err_F = mt.tfr.rel_to_scale(F_d, F_t)
    print(f"device: gp {gp_d} tau {tau_d} lnp {lnp_d!r} in {res_d.nfev} evaluations; twin: gp {gp_t} tau {tau_t} lnp {lnp_t!r} in "
          f"{res_t.nfev}; truth gp {gp_true}, static; lambda_min {lam:.3e}, |dx| {np.linalg.norm(x_d - x_t):.3e} (bound {bound:.3e}); "
          f"F against the twin's {err_F:.2e}; sd_tau device {sd_tau_d} twin {sd_tau_t}")
    print(f"variability statistic lnp - lnp(tau = inf): with the baseline device {lnp_d - lnp_static:.6f} twin {stat_t:.6f}; "
          f"without it device {lnp_dp - static_dp:.6f} (tau {tau_dp}) twin {stat_t_plain:.6f} (tau {tau_p})")
    assert tau_d[1] == INF and tau_t[1] == INF and np.isfinite(tau_d[0]) and np.all(gp_d > 0)
    assert abs(lnp_d - lnp_t) <= 1e-8 * abs(lnp_t)
    # lnp_static is the MARGINAL likelihood at tau = inf: the bits of lnlike_marginal at the fitted gp
    assert _same_bits([lnp_static], [static_marg]) and value_d == lnp_d and value_again == value_d
    assert lam > 0, "the twin's optimum is no maximum in the free parameters"
    assert np.linalg.norm(x_d - x_t) <= bound
    # ... and in the four log gp alone, where that bound says nothing: minimised over the flat tau coordinate the quadratic form
    # is the Schur complement S = H_gg - H_gt H_tt^-1 H_tg, so the same deficit confines log gp to sqrt(2 delta / lambda_min(S))
    # (on the twin: lambda_min(S) = 30.2, the bound 1.3e-3)
    Hs = 0.5 * (H + H.T)
    assert Hs[4, 4] > 0
    lam_gp = float(np.linalg.eigvalsh(Hs[:4, :4] - np.outer(Hs[:4, 4], Hs[4, :4]) / Hs[4, 4]).min())
    bound_gp = 2.0 * np.sqrt(2.0 * delta / lam_gp) if lam_gp > 0 else float("nan")
    print(f"log gp alone: lambda_min of the Schur complement {lam_gp:.3e}, |dx_gp| {np.linalg.norm((x_d - x_t)[:4]):.3e} "
          f"(bound {bound_gp:.3e})")
    assert lam_gp > 0 and np.linalg.norm((x_d - x_t)[:4]) <= bound_gp
    # the Fisher matrix and the Laplace algebra on it: twice the float64 table's figure (two float64 evaluations, each that far
    # from long double) times the margin; the inverse loses the condition number of the scaled F_log on top
    assert err_F <= 2 * TOL["F"]
    d_t = np.sqrt(np.diag(cov_t))
    cond = np.linalg.cond(np.linalg.inv(cov_t) * np.outer(d_t, d_t))
    assert np.max(np.abs(cov_d - cov_t) / np.outer(d_t, d_t)) <= 2 * TOL["F"] * cond
    assert np.isnan(sd_tau_d[1]) and sd_tau_d[0] > 0 and np.all(sd_gp_d > 0)
    # the direction the twin shows: the baseline takes the spurious gain away
    assert stat_t_plain > 100 and abs(stat_t) < 1e-3 * stat_t_plain
    assert lnp_dp - static_dp >= 0.5 * stat_t_plain and abs(lnp_d - lnp_static) <= 1e-3 * stat_t_plain
