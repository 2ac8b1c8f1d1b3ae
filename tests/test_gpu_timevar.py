"""GPU tests of the time-variable kernel (psoap_chunk_set_times, psoap_chunk_lnlike_tv_grad, psoap_fill_sym_tv;
k_fill_sym_tv in psoap_amd/csrc/fill_kernels.hpp and the TV branches of grad_kernels.hpp).

The cases are those of tests/timevar_reference.py: the seven shapes of grad_reference.CASES (N = 100 .. 520 at the edges of
the 128-row tiles, c = 1, 2, 3, masked chunks with unequal epochs, mu_GP = 0.9), times = dates[epoch] of the chunk's own
dates, tau per component from (0.25 x span, inf, 2 x span), and N = 300, c = 2 with the pixels permuted.  ``lnp`` against the
long-double reference at the project's 1e-10 max(1, |lnp|); the gradient against it, every entry, relative to the cancellation
scale S = 1/2 sum_ij |Q_ij| |dK_ij/dtheta| of its sum (sum_i |alpha_i| for mu_GP).

The tolerance is derived, not fitted: the float64 SciPy evaluation of the same formulas (timevar_reference.tv_f64) measured
against the long-double one on these very cases (python tests/timevar_reference.py), max over the entries of
|f64 - long double| / S:

    case             grad_gp   grad_tau    grad_mu   grad_lwl
    N100-c2         1.77e-17   1.06e-16   1.09e-17   1.66e-15
    N128-c2         3.01e-17   4.67e-17   2.57e-18   1.23e-14
    N129-c2         1.91e-17   5.37e-17   5.34e-18   5.00e-15
    N300-c1         8.63e-18   2.07e-17   9.73e-18   2.70e-15
    N300-c2         6.64e-17   8.19e-18   9.13e-18   1.63e-14
    N300-c3         6.40e-17   1.62e-17   1.99e-18   8.77e-15
    N520-c2         1.70e-17   5.90e-19   1.53e-17   4.21e-15
    N300-c2-perm    1.85e-17   9.02e-17   2.71e-17   2.13e-14
    max             6.64e-17   1.06e-16   2.71e-17   2.13e-14

The device sums in another order and fuses multiply-adds but is fp64 throughout: it gets the largest measured value of each
output times the margin of 8 of tests/test_gpu_grad.py:

    grad_gp 8 x 6.64e-17 = 5.31e-16    grad_tau 8 x 1.06e-16 = 8.48e-16    grad_mu 8 x 2.71e-17 = 2.17e-16
    grad_lwl 8 x 2.13e-14 = 1.70e-13

Measured on one MI355X, the largest over the cases: grad_gp 1.14e-16, grad_tau 1.24e-16, grad_mu 6.27e-17, grad_lwl
2.34e-14; the fill 2 ulp.

Registers of the build these figures come from (profiles/timevar.md; VGPRs / spilled VGPRs / scratch bytes per lane):
k_tv_grad_contract<1> 216 / 0 / 0, <2> 256 / 32 / 132, <3> 256 / 38 / 156, beside k_grad_contract<1> 212 / 0 / 0,
<2> 256 / 15 / 64, <3> 256 / 13 / 56; k_fill_sym_tv<1,2,3> 88 / 124 / 148 VGPRs, no spill.
"""
import numpy as np
import pytest

import grad_reference as gr
import timevar_reference as tv
from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu

LNP_RTOL = 1e-10
MARGIN = 8
F64_REL_TO_S = {"gp": 6.64e-17, "tau": 1.06e-16, "mu": 2.71e-17, "lwl": 2.13e-14}        # the table above, last row
TOL = {k: MARGIN * v for k, v in F64_REL_TO_S.items()}
FILL_ULP = 4
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


def _ulp_diff(a, b):
    return np.abs(np.ascontiguousarray(a, dtype=np.float64).view(np.int64) - np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


# ---- the fill ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_sigma", (False, True), ids=("plain", "sigma"))
@pytest.mark.parametrize("N", (129, 300))
@pytest.mark.parametrize("c", (1, 2, 3))
def test_fill_at_infinite_tau_is_the_static_fill_bit_for_bit(c, N, with_sigma):
    from psoap_amd import _lib
    from psoap_amd._lib import check, dptr
    ch = syn.make_chunk(c, 5, 60, seed=7700 + c)
    lw = np.ascontiguousarray(ch.lwls[:, :N])
    t = np.ascontiguousarray((ch.dates[ch.epoch_index] - ch.dates.min())[:N])
    gp = np.array(syn.GP_BASE[c], dtype=np.float64)
    sig = np.ascontiguousarray(ch.sigma[:N]) if with_sigma else None
    L, dev = _lib.load(), _lib.default_device()
    static, tvm = np.empty((N, N)), np.empty((N, N))
    check(L.psoap_fill_sym(dev, c, N, dptr(lw), dptr(gp), None if sig is None else dptr(sig), dptr(static)), "psoap_fill_sym")
    check(L.psoap_fill_sym_tv(dev, c, N, dptr(lw), dptr(t), dptr(gp), dptr(np.full(c, INF)), None if sig is None else dptr(sig),
                              dptr(tvm)), "psoap_fill_sym_tv")
    assert np.array_equal(static.view(np.int64), tvm.view(np.int64))
    assert np.any(static[0, 1:] != 0.0)


@pytest.mark.parametrize("narrow", (False, True), ids=("base", "narrow"))
@pytest.mark.parametrize("case", (tv.CASES[2], tv.CASES[5], tv.CASES[7]), ids=tv.case_id)
def test_fill_at_finite_tau_against_the_float64_twin(case, narrow):
    """The twin forms the same argument bits, so only exp() differs: 4 ulp, the project's fill contract, and exact zeros
    exactly where every component's argument is at or below -746.  ``narrow``: length scales a tenth of the benchmark's and
    every tau finite and short, so that most of the matrix underflows and the shortcut is taken."""
    from psoap_amd import matrix_functions as mf
    d = tv.case_data(case)
    gp, tau = d.gp.copy(), d.tau.copy()
    if narrow:
        gp[1::2] *= 0.1
        tau = np.full(tau.shape, 0.02 * d.span)
    N = d.lwls.shape[1]
    got = np.empty((N, N))
    mf.fill_V11_timevar(got, d.lwls, d.times, gp, tau, sigma=d.sigma)
    want, args = tv.matrix_f64(d.lwls, d.times, gp, tau, d.sigma, want_args=True)
    dead = np.all(args <= -746.0, axis=0)
    print(f"{tv.case_id(case)} narrow={narrow}: max ulp {int(_ulp_diff(got, want).max())}, exact zeros {int(dead.sum())} of {N * N}")
    # +0 where the shortcut applies (the twin's exp() is +0 there as well); everywhere else -- the subnormal results just
    # above the underflow included -- the 4 ulp, which leave a normal number no way to be zero
    assert np.all(got[dead] == 0.0) and np.all(want[dead] == 0.0) and not np.any(np.signbit(got))
    assert _ulp_diff(got, want).max() <= FILL_ULP
    assert np.array_equal(got, got.T)
    if narrow:
        assert dead.sum() > N * N // 2


# ---- value and gradient ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tv.CASES, ids=tv.case_id)
def test_value_and_gradient_against_long_double(case):
    d, ref = tv.case_data(case), tv.case_ext(case)
    with _handle(d) as h:
        lnp, g_gp, g_tau, g_lwl, g_mu = h.lnlike_tv_grad(d.lwls, d.gp, d.tau, tv.MU_GP)
        value_only = h.lnlike_tv(d.lwls, d.gp, d.tau, tv.MU_GP)
    got = tv.TvGrad(lnp, g_gp, g_tau, g_lwl, g_mu, None, None, None, None)
    err = tv.errors(got, ref)
    print(f"{tv.case_id(case)}: lnp {lnp!r} long double {ref.lnp!r}; grad_tau {g_tau} long double "
          f"{np.asarray(ref.tau, dtype=np.float64)}; error / S: " + ", ".join(f"{k} {v:.2e} (bound {TOL[k]:.2e})" for k, v in err.items()))
    assert abs(lnp - ref.lnp) <= LNP_RTOL * max(1.0, abs(ref.lnp))
    assert _same_bits([value_only], [lnp])
    assert g_lwl.shape == d.lwls.shape and np.all(np.isfinite(g_lwl))
    assert np.all(g_tau[np.isinf(d.tau)] == 0.0) and np.all(g_tau[np.isfinite(d.tau)] != 0.0)
    for k in tv.OUTPUTS:
        assert err[k] <= TOL[k], (k, err[k], TOL[k])


@pytest.mark.parametrize("shape", gr.CASES, ids=gr.case_id)
def test_all_infinite_tau_has_the_bits_of_lnlike_grad(shape):
    ch, gp = gr.case_chunk(shape), gr.case_gp(shape)
    from psoap_amd.chunk import ChunkHandle
    with ChunkHandle(ch.fl, ch.sigma) as h:
        h.set_times(ch.dates[ch.epoch_index] - ch.dates.min())
        static = h.lnlike_grad(ch.lwls, gp, gr.MU_GP)
        lnp, g_gp, g_tau, g_lwl, g_mu = h.lnlike_tv_grad(ch.lwls, gp, np.full(shape[1], INF), gr.MU_GP)
        again = h.lnlike_grad(ch.lwls, gp, gr.MU_GP)
    assert _same_bits([lnp, g_gp, g_lwl, g_mu], static) and _same_bits(again, static)
    assert g_tau.shape == (shape[1],) and np.all(g_tau == 0.0)


def _proposals(d, B, seed):
    """B different proposals on the case's chunk: perturbed grids, hyper-parameters and time scales (one tau stays inf)"""
    rng = np.random.default_rng(seed)
    c, N = d.lwls.shape
    lw = d.lwls[None] + rng.normal(0.0, 2.0 / syn.C_KMS, size=(B, c, 1))
    gps = d.gp[None] * rng.uniform(0.8, 1.25, size=(B, 2 * c))
    taus = np.where(np.isfinite(d.tau), 1.0, INF)[None] * np.where(np.isfinite(d.tau), d.tau, 1.0)[None] * rng.uniform(0.5, 2.0, size=(B, c))
    return np.ascontiguousarray(lw), np.ascontiguousarray(gps), np.ascontiguousarray(taus)


def test_batches_are_bit_reproducible_and_independent_of_the_grouping():
    """B = 3 different proposals = three B = 1 calls, bit for bit; the same call twice; B = 10 -- above the cap of 8 matrices
    per group -- equals its proposals one by one; the value-only call returns the bits of lnp of the full call."""
    d = tv.case_data(tv.CASES[2])           # N = 129: two tile rows
    lw, gps, taus = _proposals(d, 10, 7800)
    with _handle(d) as h:
        three = h.lnlike_tv_grad(lw[:3], gps[:3], taus[:3], tv.MU_GP)
        again = h.lnlike_tv_grad(lw[:3], gps[:3], taus[:3], tv.MU_GP)
        ten = h.lnlike_tv_grad(lw, gps, taus, tv.MU_GP)
        values = h.lnlike_tv(lw, gps, taus, tv.MU_GP)
        singles = [h.lnlike_tv_grad(lw[b], gps[b], taus[b], tv.MU_GP) for b in range(10)]
    N = d.lwls.shape[1]
    assert [v.shape for v in three] == [(3,), (3, 4), (3, 2), (3, 2, N), (3,)]
    assert _same_bits(three, again)
    assert len({float(v) for v in ten[0]}) == 10 and np.all(np.isfinite(ten[0]))
    assert values.shape == (10,) and _same_bits([values], [ten[0]])
    for b in range(10):
        one = [np.atleast_1d(v) for v in singles[b]]
        assert _same_bits([ten[k][b] for k in range(5)], one), b
        if b < 3:
            assert _same_bits([three[k][b] for k in range(5)], one), b


@pytest.mark.parametrize("bad", (0.0, -3.0, float("nan")), ids=("zero", "negative", "nan"))
def test_a_tau_that_is_no_time_scale_gives_minus_inf_there_and_leaves_the_others(bad):
    d = tv.case_data(tv.CASES[0])
    lw, gps, taus = _proposals(d, 3, 7900)
    with _handle(d) as h:
        good = h.lnlike_tv_grad(lw, gps, taus, tv.MU_GP)
        taus2 = taus.copy()
        taus2[1, 0] = bad
        lnp, g_gp, g_tau, g_lwl, g_mu = h.lnlike_tv_grad(lw, gps, taus2, tv.MU_GP)
        value = h.lnlike_tv(lw, gps, taus2, tv.MU_GP)
    assert np.isneginf(lnp[1]) and np.isneginf(value[1])
    assert np.all(np.isnan(g_gp[1])) and np.all(np.isnan(g_tau[1])) and np.all(np.isnan(g_lwl[1])) and np.isnan(g_mu[1])
    keep = [0, 2]
    assert np.all(np.isfinite(good[0]))
    assert _same_bits([v[keep] for v in (lnp, g_gp, g_tau, g_lwl, g_mu)], [v[keep] for v in good])
    assert _same_bits([value[keep]], [good[0][keep]])


def test_conventions_null_outputs_missing_times_baseline_release():
    from psoap_amd._lib import PsoapError, check, dptr
    from psoap_amd.chunk import ChunkHandle
    d = tv.case_data(tv.CASES[0])
    lw, gps, taus = _proposals(d, 3, 8000)
    N = d.lwls.shape[1]
    with ChunkHandle(d.fl, d.sigma) as h:
        # before set_times: refused, and the message names the setter
        with pytest.raises(PsoapError, match="psoap_chunk_set_times"):
            h.lnlike_tv_grad(lw, gps, taus, tv.MU_GP)
        with pytest.raises(PsoapError, match="psoap_chunk_set_times"):
            h.lnlike_tv(lw, gps, taus, tv.MU_GP)
        h.set_times(d.times)
        full = h.lnlike_tv_grad(lw, gps, taus, tv.MU_GP)
        # NULL for the optional outputs: the same bits in the others
        lnp2, g2, t2 = np.empty(3), np.empty((3, 4)), np.empty((3, 2))
        check(h._L.psoap_chunk_lnlike_tv_grad(h._h, 3, 2, dptr(lw), dptr(gps), dptr(taus), tv.MU_GP, dptr(lnp2), dptr(g2), dptr(t2),
                                              None, None), "psoap_chunk_lnlike_tv_grad")
        assert _same_bits([lnp2, g2, t2], full[:3])
        # value only: the other gradients must be NULL too
        rc = h._L.psoap_chunk_lnlike_tv_grad(h._h, 3, 2, dptr(lw), dptr(gps), dptr(taus), tv.MU_GP, dptr(lnp2), None, dptr(t2),
                                             None, None)
        assert rc != 0 and b"grad_gp == NULL" in h._L.psoap_last_error()
        # an open stream refuses the call and the setter
        h.stream_open(2, 1)
        try:
            with pytest.raises(PsoapError, match="open stream"):
                h.lnlike_tv_grad(lw, gps, taus, tv.MU_GP)
            with pytest.raises(PsoapError, match="open stream"):
                h.set_times(d.times)
        finally:
            h.stream_close()
        # release twice, then another call: the workspace comes back, the times stayed, and so do the bits
        h.grad_release()
        h.grad_release()
        assert _same_bits(h.lnlike_tv_grad(lw[0], gps[0], taus[0], tv.MU_GP), [v[0] for v in full])
        # a handle with a baseline is refused for now
        ch = gr.case_chunk(tv.CASES[0][1])
        h.set_baseline(1, ch.lwl, ch.epoch_index, ch.n_epochs, [0.1, 0.1])
        with pytest.raises(PsoapError, match="baseline"):
            h.lnlike_tv_grad(lw, gps, taus, tv.MU_GP)
    assert full[3].shape == (3, 2, N)


def test_times_need_not_be_sorted_a_permuted_chunk_gives_the_permuted_gradient():
    """the likelihood does not depend on the order of the pixels: the permuted case against the same chunk in epoch order
    (another summation order: the value to 1e-10 relative, the wavelength gradient to the bound of the table)"""
    d = tv.case_data(tv.CASES[7])
    perm = np.random.default_rng(7200 + 300 + 2).permutation(d.lwls.shape[1])
    inv = np.argsort(perm)
    with _handle(d) as h:
        lnp_p, gp_p, tau_p, lwl_p, _ = h.lnlike_tv_grad(d.lwls, d.gp, d.tau, tv.MU_GP)
    from psoap_amd.chunk import ChunkHandle
    with ChunkHandle(d.fl[inv], d.sigma[inv]) as h:
        h.set_times(d.times[inv])
        lnp_s, gp_s, tau_s, lwl_s, _ = h.lnlike_tv_grad(d.lwls[:, inv], d.gp, d.tau, tv.MU_GP)
    assert np.all(np.diff(d.times[inv]) >= 0)
    ref = tv.case_ext(tv.CASES[7])
    assert abs(lnp_p - lnp_s) <= LNP_RTOL * max(1.0, abs(lnp_s))
    assert gr.rel_to_scale(gp_p, gp_s, ref.s_gp) <= 2 * TOL["gp"] and tv.rel_tau(tau_p, tau_s, ref.s_tau) <= 2 * TOL["tau"]
    assert gr.rel_to_scale(lwl_p[:, inv], lwl_s, ref.s_lwl[:, inv]) <= 2 * TOL["lwl"]


# ---- the fit -----------------------------------------------------------------------------------------------------------------
def test_optimize_GP_timevar_agrees_with_the_same_driver_on_the_float64_twin():
    """Flux drawn on the host from the time-variable model itself (N = 300, 6 epochs, c = 2, tau_true = (0.25 x span, inf)),
    the second component's tau held at inf with ``free_tau``.  ``optimize_GP_timevar`` on the device and the same L-BFGS-B
    driver (covariance._fit_timevar) on ``tv_f64`` start from the same point.  Asserted: agreement with the twin, not
    recovery of the truth -- six epochs do not pin tau tightly.

    The bounds.  The optimum's lnp: 1e-8 relative.  The parameters: both runs end within delta = 1e-8 |lnp| of the maximum
    (that is what the first bound says of them), and near a maximum with Hessian H (of -lnL in the log-parameters the fit
    works in) a deficit delta confines a point to |x - x*| <= sqrt(2 delta / lambda_min(H)); two such points are at most
    twice that apart.  H comes from central differences (step 1e-4 in log-parameters) of the twin's own analytic gradient
    at the twin's optimum."""
    from psoap_amd import covariance
    shape = gr.CASES[4]
    ch = gr.case_chunk(shape)
    assert ch.N == 300 and ch.n_epochs == 6
    times = ch.dates[ch.epoch_index]                      # Julian dates: covariance subtracts the minimum
    t0 = times - times.min()
    span = float(t0.max())
    gp_true, tau_true = gr.case_gp(shape), np.array([0.25 * span, INF])
    K = tv.matrix_f64(ch.lwls, t0, gp_true, tau_true, ch.sigma)
    fl = 1.0 + np.linalg.cholesky(K) @ np.random.default_rng(8100).standard_normal(ch.N)
    sigma = ch.sigma.copy()
    gp0, tau0, free = gp_true * np.array([1.3, 0.8, 0.8, 1.25]), np.array([0.6 * span, INF]), [True, False]

    def twin(gp, tau):
        g = tv.tv_f64(ch.lwls, t0, fl, sigma, gp, tau, 1.0)
        return g.lnp, g.gp, g.tau

    try:
        gp_d, tau_d, lnp_d, lnp_static, res_d = covariance.optimize_GP_timevar(ch.lwls, fl, sigma, gp0, tau0, times, free_tau=free,
                                                                               full_output=True)
    finally:
        covariance.release_handles()
    gp_t, tau_t, res_t = covariance._fit_timevar(twin, 2, gp0, tau0, free, 1e-10)
    lnp_t = -float(res_t["fun"])
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
    print(f"device: gp {gp_d} tau {tau_d} lnp {lnp_d!r} in {res_d.nfev} evaluations; twin: gp {gp_t} tau {tau_t} lnp {lnp_t!r} in "
          f"{res_t.nfev}; truth gp {gp_true} tau {tau_true}; lambda_min {lam:.3e}, |dx| {np.linalg.norm(x_d - x_t):.3e} "
          f"(bound {bound:.3e}); variability statistic lnp - lnp(tau = inf) = {lnp_d - lnp_static:.4f}")
    assert tau_d[1] == INF and tau_t[1] == INF and np.isfinite(tau_d[0]) and np.all(gp_d > 0)
    assert abs(lnp_d - lnp_t) <= 1e-8 * abs(lnp_t)
    assert lam > 0, "the twin's optimum is no maximum in the free parameters"
    assert np.linalg.norm(x_d - x_t) <= bound
    assert lnp_d >= lnp_static            # the static model is inside the family (tau -> inf)
