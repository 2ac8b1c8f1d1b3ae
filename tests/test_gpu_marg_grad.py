"""GPU tests of the gradient of the continuum-marginalised likelihood (psoap_chunk_lnlike_marg_grad,
psoap_chunk_lnprob_marg_grad; psoap_amd/csrc/marg_grad_kernels.hpp, marg_grad_plan.hpp).

The cases of tests/marg_reference.py, each with weight = None and weight = fl, against the long-double gradient on the dense
K + H Lambda H^T (marg_grad_reference.marg_grad_ext), entry by entry relative to the cancellation scale
S = 1/2 sum_ij |Q_m,ij| |dK_ij/dtheta| (sum_i |alpha_m,i| for mu_GP).

The tolerance is derived, not fitted: the float64 SciPy evaluation of the device's own Woodbury route
(marg_grad_reference.marg_grad_f64) measured against the long-double one on these very cases
(python tests/marg_grad_reference.py):

    case                      grad_gp    grad_mu   grad_lwl
    a-N100-c2-o1-one         1.73e-15   1.24e-14   3.05e-13
    a-N100-c2-o1-flux        3.00e-15   1.21e-14   4.32e-13
    b-N128-c1-o0-one         2.48e-17   9.91e-17   2.21e-15
    b-N128-c1-o0-flux        2.07e-17   1.71e-16   2.23e-15
    c-N129-c2-o2-one         9.56e-17   1.29e-15   3.73e-14
    c-N129-c2-o2-flux        1.43e-16   1.45e-17   2.18e-13
    d-N384-c1-o3-one         3.06e-17   1.13e-16   7.91e-14
    d-N384-c1-o3-flux        1.39e-16   3.03e-15   4.43e-14
    e-N300-c3-o1-one         3.28e-16   1.33e-16   1.23e-13
    e-N300-c3-o1-flux        3.21e-16   2.75e-17   1.08e-13
    f-N312-c2-o4-one         5.60e-16   3.10e-15   2.44e-12
    f-N312-c2-o4-flux        2.74e-16   3.08e-15   2.27e-12
    max                      3.00e-15   1.24e-14   2.44e-12

(the five digits the abscissa map of the basis cancels -- tests/test_gpu_marg.py -- are what the larger figures are made of).
The device sums in another order and fuses multiply-adds but is fp64 throughout: it gets the largest measured value of each
output times the project's margin of 8 (tests/test_gpu_grad.py).  The four seeded defects of
tests/test_marg_grad_reference.py miss these bounds by factors of 1e7 and more.

Through the orbit (psoap_chunk_lnprob_marg_grad on marg_reference.orbit_case) the reference stands on the grids of the
long-double orbit; the float64 host composition (restated device velocities, host shift, marg_grad_f64, velocity_gradient,
jacobian_f64) against it, relative to S_orb and the scales above:

    SB2-N240 orbit chain   grad_orb 1.11e-12 grad_gp 5.36e-15 grad_mu 2.57e-14

again times 8.

Measured on the device (MI355X), largest error / scale: grad_gp 4.69e-16, grad_mu 4.07e-15, grad_lwl 2.14e-12 over the twelve
cases; through the orbit grad_orb 1.11e-12, grad_gp 5.43e-15, grad_mu 2.57e-14.
"""
import ctypes

import numpy as np
import pytest

import grad_reference as gr
import marg_grad_reference as mg
import marg_reference as mr
from psoap_amd import synthetic as syn
from psoap_amd.utils import MODEL_ID

pytestmark = pytest.mark.gpu

MARGIN = 8
F64 = {"grad_gp": 3.00e-15, "grad_mu": 1.24e-14, "grad_lwl": 2.44e-12}              # the table above, last row
TOL = {k: MARGIN * v for k, v in F64.items()}
F64_ORBIT = {"grad_orb": 1.11e-12, "grad_gp": 5.36e-15, "grad_mu": 2.57e-14}        # the SB2 row above
TOL_ORBIT = {k: MARGIN * v for k, v in F64_ORBIT.items()}
TOL_LNP_ORBIT = MARGIN * 3.47e-12           # tests/test_gpu_marg.py: lnp of a worker against the long-double orbit


def _handle(ch, **kw):
    from psoap_amd.chunk import ChunkHandle
    return ChunkHandle(ch.fl, ch.sigma, **kw)


def _baseline(h, case, kind):
    ch = mr.case_chunk(case)
    h.set_baseline(ch.order, ch.x, ch.epoch_index, ch.n_epochs, mr.prior_sd(ch.order), mr.case_weight(case, kind))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).copy()


def _same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


class _Got:
    def __init__(self, t):
        self.lnp, self.gp, self.lwl, self.mu = t


@pytest.mark.parametrize("kind", mr.WEIGHTS)
@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_id)
def test_gradient_against_long_double_and_value_bits(case, kind):
    ch, gp, c = mr.case_chunk(case), mr.case_gp(case), case[2]
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))      # noqa: E731
    with _handle(ch) as h:
        _baseline(h, case, kind)
        value = h.lnlike_marg(ch.lwls, gp, mr.MU_GP, want_beta=True)
        got = h.lnlike_marg_grad(ch.lwls, gp, mr.MU_GP)
        lw, lnp, parts, g_gp = np.ascontiguousarray(ch.lwls), np.empty(1), np.empty(4), np.empty(2 * c)
        assert h._L.psoap_chunk_lnlike_marg_grad(h._h, 1, c, dp(lw), dp(gp), mr.MU_GP, dp(lnp), dp(parts), dp(g_gp), None, None) == 0
    assert got[1].shape == (2 * c,) and got[2].shape == ch.lwls.shape
    # lnp and the four parts: the bits of psoap_chunk_lnlike_marg; the gradient does not depend on the outputs asked for
    assert _same_bits([got[0], lnp[0], parts], [value.lnp, value.lnp, value.parts])
    assert _same_bits([g_gp], [got[1]])
    err = mg.errors(_Got(got), mg.case_ext(case, kind))
    print(f"{mr.case_id(case)}-{kind}: " + ", ".join(f"{k} {v:.2e} ({TOL[k]:.2e})" for k, v in err.items()))
    for k, v in err.items():
        assert v <= TOL[k], (k, v, TOL[k])


def test_batches_groups_and_repeats_keep_the_bits():
    """B = 3 and B = 10 (more than GRAD_GROUP_MAX = 8: two groups, 8 + 2) against single calls, and a call repeated"""
    case = mr.case_named("f")
    ch, c = mr.case_chunk(case), case[2]
    gps = syn.make_walkers(c, 10, seed=9801)
    gps[0] = mr.case_gp(case)
    lw = np.stack([ch.lwls + 1e-6 * k for k in range(10)])
    with _handle(ch) as h:
        _baseline(h, case, "flux")
        ten = h.lnlike_marg_grad(lw, gps, mr.MU_GP)
        again = h.lnlike_marg_grad(lw, gps, mr.MU_GP)
        three = h.lnlike_marg_grad(lw[:3], gps[:3], mr.MU_GP)
        singles = [h.lnlike_marg_grad(lw[b], gps[b], mr.MU_GP) for b in range(10)]
    assert ten[0].shape == (10,) and ten[2].shape == (10, c, ch.fl.shape[0]) and len({float(v) for v in ten[0]}) == 10
    assert _same_bits(ten, again)
    for b in range(10):
        assert _same_bits([v[b] for v in ten], singles[b]), b
        if b < 3:
            assert _same_bits([v[b] for v in three], singles[b]), b


def test_plain_gradient_keeps_its_bits():
    case = mr.case_named("e")
    ch, gp = mr.case_chunk(case), mr.case_gp(case)
    with _handle(ch) as h:
        never = h.lnlike_grad(ch.lwls, gp, mr.MU_GP)
    with _handle(ch) as h:
        _baseline(h, case, "one")
        before = h.lnlike_grad(ch.lwls, gp, mr.MU_GP)
        marg = h.lnlike_marg_grad(ch.lwls, gp, mr.MU_GP)
        after = h.lnlike_grad(ch.lwls, gp, mr.MU_GP)
        value = h.lnlike_marg(ch.lwls, gp, mr.MU_GP)
    assert _same_bits(before, never) and _same_bits(after, never)
    assert _same_bits([marg[0]], [value]) and not _same_bits([marg[1]], [never[1]])


def test_degenerate_proposals_inside_a_batch():
    from psoap_amd.chunk import ChunkHandle
    case = mr.case_named("a")
    ch, gp = mr.case_chunk(case), mr.case_gp(case)
    neg = gp.copy()
    neg[0] = -neg[0]
    with _handle(ch) as h:
        _baseline(h, case, "one")
        good = h.lnlike_marg_grad(ch.lwls, gp, mr.MU_GP)
        out = h.lnlike_marg_grad(np.stack([ch.lwls, ch.lwls, ch.lwls]), np.stack([gp, neg, gp]), mr.MU_GP)
    assert out[0][1] == -np.inf and all(np.all(np.isnan(v[1])) for v in out[1:])
    assert _same_bits([v[0] for v in out], good) and _same_bits([v[2] for v in out], good)
    # not positive definite: zero noise and two identical pixels (the degenerate input of tests/test_gpu_marg.py), between
    # two proposals that are
    lw = ch.lwls.copy()
    lw[:, 1] = lw[:, 0]
    amp = gp.copy()
    amp[0] *= 1.5
    with ChunkHandle(ch.fl, np.zeros_like(ch.sigma)) as h:
        _baseline(h, case, "one")
        far = ch.lwls + 1e-3 * np.arange(ch.lwls.shape[1])[None, :]          # pixels far apart: K is nearly diagonal
        solo = h.lnlike_marg_grad(far, amp, mr.MU_GP)
        out = h.lnlike_marg_grad(np.stack([far, lw, far]), np.stack([amp, gp, amp]), mr.MU_GP)
    assert np.isfinite(solo[0]) and out[0][1] == -np.inf and all(np.all(np.isnan(v[1])) for v in out[1:])
    assert _same_bits([v[0] for v in out], solo) and _same_bits([v[2] for v in out], solo)


def test_refusals_and_release():
    from psoap_amd._lib import PsoapError, load
    case = mr.case_named("c")
    ch, gp, c = mr.case_chunk(case), mr.case_gp(case), case[2]
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))      # noqa: E731
    last = lambda: load().psoap_last_error()      # noqa: E731
    with _handle(ch) as h:
        with pytest.raises(PsoapError, match="set_baseline"):
            h.lnlike_marg_grad(ch.lwls, gp, mr.MU_GP)
        with pytest.raises(PsoapError, match="set_baseline"):
            h.lnprob_marg_grad(SB2, np.array(syn.ORBIT_BASE["SB2"]), gp)
        lw, lnp, g = np.ascontiguousarray(ch.lwls), np.empty(1), np.empty(2 * c)
        assert h._L.psoap_chunk_lnlike_marg_grad(h._h, 1, c, dp(lw), dp(gp), mr.MU_GP, dp(lnp), None, dp(g), None, None) != 0
        assert b"psoap_chunk_lnlike_marg_grad: call psoap_chunk_set_baseline first" in last()
        _baseline(h, case, "flux")
        good = h.lnlike_marg_grad(ch.lwls, gp, mr.MU_GP)
        h.marg_release()
        assert _same_bits(h.lnlike_marg_grad(ch.lwls, gp, mr.MU_GP), good)
        h.grad_release()
        h.marg_release()
        assert _same_bits(h.lnlike_marg_grad(ch.lwls, gp, mr.MU_GP), good)
        # a set_data after a weighted baseline: refused, with the message of lnlike_marg
        h.set_data(ch.fl, ch.sigma)
        with pytest.raises(PsoapError, match="set_baseline again"):
            h.lnlike_marg_grad(ch.lwls, gp, mr.MU_GP)
        assert h._L.psoap_chunk_lnlike_marg_grad(h._h, 0, c, dp(lw), dp(gp), mr.MU_GP, dp(lnp), None, dp(g), None, None) != 0
        assert b"B must be at least 1" in last()


# ---- lnprob(p): grids from the orbit -------------------------------------------------------------------------------------
SB2 = MODEL_ID["SB2"]
BASE = {"order": 1, "sd": list(mr.PLANT_SD), "weight": "one"}


def _orbit_worker(baseline, fix=(), max_batch=1):
    from psoap_amd.lnprob import ChunkWorker
    from psoap_amd.utils import registered_params
    ch, p_orb, gp, _, _ = mr.orbit_case()
    full = dict(zip(registered_params["SB2"], list(p_orb) + list(gp)))
    w = ChunkWorker("SB2", ch.lwl, ch.fl, ch.sigma, ch.epoch_index, ch.dates, fix_params=list(fix), defaults=full,
                    max_batch=max_batch, baseline=baseline)
    names = [n for n in registered_params["SB2"] if n not in fix]
    return ch, w, np.array([full[n] for n in names]), names, np.asarray(p_orb, dtype=np.float64), np.asarray(gp, dtype=np.float64)


def test_orbit_entry_against_the_long_double_chain_and_the_bits_of_its_pieces():
    from psoap_amd import orbit
    ch, w, _, _, p_orb, gp = _orbit_worker(BASE)
    ref, orb, s_orb = mg.chain_ext()
    try:
        lnp, g_orb, g_gp, g_mu, g_vel = w.lnprob_grad_orbits(p_orb, gp, mr.MU_GP, want_vel=True)
        lw = ch.lwl + (-orbit.velocities("SB2", p_orb[None], ch.dates)[:, :, ch.epoch_index]) / syn.C_KMS
        pieces = w.handle.lnlike_marg_grad(lw, gp[None], mr.MU_GP)
        value = w.lnprob(np.concatenate([p_orb, gp]), mr.MU_GP)
    finally:
        w.close()
    assert g_orb.shape == (1, 7) and g_vel.shape == (1, 2, mr.PLANT_EPOCHS)
    assert _same_bits([lnp, g_gp, g_mu], [pieces[0], pieces[1], pieces[3]]) and _same_bits([lnp[0]], [value])
    err = {"grad_orb": gr.rel_to_scale(g_orb[0], orb, s_orb), "grad_gp": gr.rel_to_scale(g_gp[0], ref.gp, ref.s_gp),
           "grad_mu": gr.rel_to_scale(g_mu[0], ref.mu, ref.s_mu)}
    print("SB2 orbit: " + ", ".join(f"{k} {v:.2e} ({TOL_ORBIT[k]:.2e})" for k, v in err.items()))
    for k, v in err.items():
        assert v <= TOL_ORBIT[k], (k, v, TOL_ORBIT[k])


# Steps of the central differences: 1e-4 of a proposal step of each parameter (synthetic.make_orbit_proposals: a tenth of the
# value; synthetic.GP_JUMP for amplitudes and length scales).  T0 takes the step of P; P itself moves the phase (t - T0) / P
# times as much as T0 does -- the thousands of cycles between T0 and the dates -- and its step is divided by that count in
# the test.
FD_STEP = {"q": 6e-6, "K": 1.2e-4, "e": 5e-6, "omega": 4e-4, "P": 2.3e-4, "T0": 2.3e-4, "amp_f": 5e-6, "l_f": 5e-5, "amp_g": 5e-6,
           "l_g": 5e-5}


def test_worker_gradient_is_the_gradient_of_the_workers_lnprob():
    """``ChunkWorker(baseline=...).lnprob_grad(p)`` against central differences D(h) of the same worker's ``lnprob``, every
    fitted parameter (gamma fixed, as in tests/test_gpu_marg.py).  The bound is stated from what is known of the value:
    its error is at most eps = TOL_LNP_ORBIT max(1, |lnp|) (the derived bound of tests/test_gpu_marg.py), so D(h) carries at
    most eps / h of it; the truncation of D(h) is |D(2h) - D(h)| / 3 (tests/test_grad_reference.py), taken twice over and
    with the noise of the two differences it is formed from.  The gradient of the PLAIN likelihood -- what this entry returned
    before it knew of the baseline -- must miss that bound."""
    ch, w, p, names, p_orb, gp = _orbit_worker(BASE, fix=("gamma",))
    try:
        lnp, grad = w.lnprob_grad(p, mr.MU_GP)
        assert lnp == w.lnprob(p, mr.MU_GP)
        plain = w.handle.lnprob_grad(SB2, p_orb, gp, mr.MU_GP)
        plain = np.concatenate([plain[1][0], plain[2][0]])[[i for i in range(11) if i != 6]]
        eps = TOL_LNP_ORBIT * max(1.0, abs(lnp))
        missed = []
        for k, name in enumerate(names):
            def D(h, k=k):
                up, dn = p.copy(), p.copy()
                up[k] += h
                dn[k] -= h
                return (w.lnprob(up, mr.MU_GP) - w.lnprob(dn, mr.MU_GP)) / (up[k] - dn[k])
            h = FD_STEP[name]
            if name == "P":
                h /= np.max(np.abs(ch.dates - p_orb[5])) / p_orb[4]
            d1, d2 = D(h), D(2 * h)
            noise1, noise2 = eps / h, eps / (2 * h)
            bound = 2 * (abs(d2 - d1) + noise1 + noise2) / 3 + noise1
            print(f"{name:6s} analytic {grad[k]:+.9e} difference {d1:+.9e} bound {bound:.2e} plain {plain[k]:+.9e}")
            assert abs(grad[k] - d1) <= bound, (name, grad[k], d1, bound)
            missed.append(abs(plain[k] - d1) > bound)
    finally:
        w.close()
    assert any(missed)


def test_fast_orbit_inside_a_batch():
    ch, w, _, _, p_orb, gp = _orbit_worker(BASE)
    fast = p_orb.copy()
    fast[1] = 4.0e6                       # K thirteen times c_kms
    try:
        solo = w.lnprob_grad_orbits(p_orb, gp, mr.MU_GP, want_vel=True)
        out = w.lnprob_grad_orbits(np.stack([p_orb, fast, p_orb]), np.stack([gp] * 3), mr.MU_GP, want_vel=True)
    finally:
        w.close()
    assert np.isneginf(out[0][1]) and all(np.all(np.isnan(v[1])) for v in out[1:])
    assert _same_bits([v[0] for v in out], [v[0] for v in solo]) and _same_bits([v[2] for v in out], [v[0] for v in solo])


def test_worker_without_a_baseline_takes_the_plain_path():
    ch, w, _, _, p_orb, gp = _orbit_worker(None)
    try:
        a = w.lnprob_grad_orbits(p_orb, gp, mr.MU_GP)
        b = w.handle.lnprob_grad(SB2, p_orb, gp, mr.MU_GP)
    finally:
        w.close()
    assert _same_bits(a, b)


# ---- fits under a baseline ---------------------------------------------------------------------------------------------------
def test_optimize_gp_under_a_baseline():
    from psoap_amd import covariance
    ch, gp, _ = mr.planted()
    base = dict(x=ch.x, epoch_index=ch.epoch_index, order=1, prior_sd=mr.PLANT_SD)
    start = gp * np.array([1.3, 0.8, 0.7, 1.2])
    args = (ch.x, ch.epoch_index, 1, mr.PLANT_SD, None, mr.MU_GP)
    try:
        res = covariance.optimize_GP(ch.lwls, ch.fl, ch.sigma, start, mr.MU_GP, full_output=True, baseline=base)
        l_start = covariance.lnlike_marginal(ch.lwls, ch.fl, ch.sigma, start, *args)
        l_end, g_end, _, _ = covariance.lnlike_marginal_grad(ch.lwls, ch.fl, ch.sigma, res.x, *args)
        with pytest.raises(ValueError, match="baseline needs"):
            covariance.optimize_GP(ch.lwls, ch.fl, ch.sigma, start, baseline={"order": 1})
    finally:
        covariance.release_handles()
    print(f"start {start} lnL {l_start!r}; L-BFGS-B {res.x} lnL {l_end!r} in {res.nfev} evaluations: {res.message}")
    assert res.success and l_end >= l_start and -res.fun == l_end
    assert np.array_equal(np.asarray(res.jac), -g_end)


def test_optimize_orbit_with_baseline_workers():
    """the planted SB2 chunk of marg_reference.orbit_case (marg_reference.planted has grids but no orbit to fit): K and q
    fitted from a start 5 % off the orbit the chunk's flux was drawn at"""
    from psoap_amd.lnprob import ChunkWorker, baseline_fit, optimize_orbit
    from psoap_amd.utils import registered_params
    ch, p_orb, gp, _, _ = mr.orbit_case()
    full = dict(zip(registered_params["SB2"], list(p_orb) + list(gp)))
    fix = [n for n in registered_params["SB2"] if n not in ("q", "K")]
    w = ChunkWorker("SB2", ch.lwl, ch.fl, ch.sigma, ch.epoch_index, ch.dates, fix_params=fix, defaults=full, baseline=BASE)
    try:
        start = np.array([full["q"] * 1.05, full["K"] * 0.95])
        res = optimize_orbit([w], start, bounds=[(0.1, 2.0), (1.0, 40.0)], full_output=True)
        l_start, l_end = w.lnprob(start), w.lnprob(res.x)
        fresh = w.lnprob_grad(res.x)[1]
        fit = baseline_fit([w], res.x)[0]
    finally:
        w.close()
    print(f"start {start} lnprob {l_start!r}; L-BFGS-B {res.x} lnprob {l_end!r} in {res.nfev} evaluations: {res.message}")
    assert res.success and l_end >= l_start and fit["lnp"] == l_end
    assert np.array_equal(np.asarray(res.jac), -fresh)
