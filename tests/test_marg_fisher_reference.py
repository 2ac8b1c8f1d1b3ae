"""CPU checks of the references for the Fisher information and the leave-one-out cross-validation under the marginalised
continuum (tests/marg_fisher_reference.py) that the GPU tests are measured against.

The long-double Fisher reference is checked against something that does not share its derivation: F = -E[Hessian of lnL],
by direct construction.  With data drawn at theta, E[lnL(theta')] = -1/2 (tr(Kt(theta')^-1 Kt(theta)) + log det Kt(theta')),
and minus its second central difference along a tangent (a four-point mixed difference for a pair) is F up to a truncation
error of second order: halving the step divides the discrepancy by 4 (between 3 and 5 here).

The conditions the GPU tests rest on are checked here, on the CPU: the float64 evaluation of the device's route stays within
the derived tolerance; on every case the marginal F and pix_mean differ from their plain-K twins by more than 100 times that
tolerance (an implementation that drops the Vt loop cannot pass); the planted continuum offset is decided by the long-double
reference alone, under the baseline and without it.
"""
import numpy as np
import pytest

import fisher_reference as fr
import loo_reference as lr
import marg_fisher_reference as mf
import marg_reference as mr

_LD = np.longdouble
KINDS = [(case, kind) for case in mr.CASES for kind in mr.WEIGHTS]
KIND_IDS = [f"{mr.case_id(case)}-{kind}" for case, kind in KINDS]


def _expected_lnl(case, kind, dlwl, dgp):
    """E[lnL] at (lwls + dlwl, gp + dgp) for data drawn at the case's own parameters, long double"""
    import oracle
    ch = mr.case_chunk(case)
    args = mf._dense_args(case, kind)
    _, L0, _ = mf.dense_ext(*args)
    lw = np.asarray(ch.lwls, dtype=_LD) + dlwl
    _, L1, _ = mf.dense_ext(lw, args[1], np.asarray(args[2], dtype=_LD) + dgp, *args[3:])
    B = oracle._fsolve_ext(L1, L0)                      # tr(Kt'^-1 Kt) = |L'^-1 L|_F^2
    return _LD(-0.5) * (np.sum(B * B) + _LD(2) * np.sum(np.log(np.diag(L1))))


def test_fisher_reference_is_minus_the_expected_hessian():
    case, kind = mr.case_named("a"), "flux"
    c = case[2]
    tan_lwl, tan_gp = (np.asarray(a, dtype=_LD) for a in mf.case_tangents(case))
    F = mf.case_ext(case, kind)[0]
    gp = mr.case_gp(case)
    steps = [_LD(0.02) * gp[t] if t < 2 * c else _LD(0.05) for t in range(tan_gp.shape[0])]
    g0 = _expected_lnl(case, kind, 0 * tan_lwl[0], 0 * tan_gp[0])

    def second(s, t, scale):
        hs, ht = scale * steps[s], scale * steps[t]
        if s == t:
            up = _expected_lnl(case, kind, hs * tan_lwl[s], hs * tan_gp[s])
            dn = _expected_lnl(case, kind, -hs * tan_lwl[s], -hs * tan_gp[s])
            return -(up - 2 * g0 + dn) / (hs * hs)
        v = [_expected_lnl(case, kind, a * hs * tan_lwl[s] + b * ht * tan_lwl[t], a * hs * tan_gp[s] + b * ht * tan_gp[t])
             for a, b in ((1, 1), (1, -1), (-1, 1), (-1, -1))]
        return -(v[0] - v[1] - v[2] + v[3]) / (4 * hs * ht)

    T = tan_gp.shape[0]
    pairs = [(t, t) for t in range(T)] + [(0, 1), (1, 2 * c), (2 * c, 2 * c + 2)]
    for s, t in pairs:
        scale = np.sqrt(F[s, s] * F[t, t])
        e1, e2 = (abs(second(s, t, k) - F[s, t]) / scale for k in (_LD(1), _LD(0.5)))
        print(f"F[{s},{t}] = {float(F[s, t]):.6e}: discrepancy / sqrt(F_ss F_tt) {float(e1):.3e} at h, {float(e2):.3e} at h/2, "
              f"ratio {float(e1 / e2):.3f}")
        assert e1 < 0.05 and 3.0 <= e1 / e2 <= 5.0, (s, t, float(e1), float(e2))


@pytest.mark.parametrize("case,kind", KINDS, ids=KIND_IDS)
def test_reference_is_symmetric_positive_and_keeps_the_marginal_value(case, kind):
    F, F_mu, loo = mf.case_ext(case, kind)
    assert np.array_equal(F, F.T) and F_mu > 0
    Fd = np.asarray(F, dtype=np.float64)
    assert np.min(np.linalg.eigvalsh(Fd)) >= -1e-12 * np.max(np.diag(Fd))
    assert np.all(loo.pix_var > 0) and np.all(loo.ep_chi2 >= 0)
    assert np.array_equal(loo.ep_npix, np.bincount(mr.case_chunk(case).epoch_index, minlength=case[3]))
    # lnp is marg_reference's, made there by another sequence of long-double steps
    ref = mr.case_ext(case, kind).lnp
    assert abs(loo.lnp - ref) <= 1e-15 * abs(ref)


def test_epoch_outputs_are_the_deleted_epochs_prediction_under_kt():
    """case a, epoch 1, really deleted: fl[I] minus its prediction from the other epochs under Kt, and its chi-squared"""
    import oracle
    case, kind = mr.case_named("a"), "one"
    ch = mr.case_chunk(case)
    C, _, _ = mf.dense_ext(*mf._dense_args(case, kind))
    loo = mf.case_ext(case, kind)[2]
    I = np.flatnonzero(ch.epoch_index == 1)
    r = np.asarray(ch.fl, dtype=_LD) - _LD(mr.MU_GP)
    resid, cov = lr._condition_ext(C, r, I)
    y = oracle._fsolve_ext(oracle._chol_ext(cov), resid)
    assert np.max(np.abs(resid - loo.ep_resid[I])) <= 1e-14
    assert abs(y @ y - loo.ep_chi2[1]) <= 1e-13 * loo.ep_chi2[1]
    i = int(I[3])
    res1, var1 = lr._condition_ext(C, r, [i])
    assert abs((_LD(ch.fl[i]) - res1[0]) - loo.pix_mean[i]) <= 1e-14 and abs(var1[0, 0] - loo.pix_var[i]) <= 1e-14 * var1[0, 0]


@pytest.mark.parametrize("name,kind", [("a", "flux"), ("c", "one"), ("f", "one")])
def test_float64_route_is_within_the_device_tolerance(name, kind):
    """the Woodbury route in float64 against the long-double dense one, on the smallest and the largest Q and on the case
    that reaches into the second tile: what the device's tolerance is derived from stays below it (the whole table: python
    tests/marg_fisher_reference.py)"""
    case = mr.case_named(name)
    err = mf.errors(mf.case_f64(case, kind), mf.case_ext(case, kind))
    print(f"{mr.case_id(case)}-{kind}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    for k, v in err.items():
        assert v <= mf.TOL[k], (name, k, v, mf.TOL[k])


@pytest.mark.parametrize("case,kind", KINDS, ids=KIND_IDS)
def test_marginal_outputs_are_far_from_their_plain_twins(case, kind):
    """the condition of the GPU tests: without the Vt loop F and pix_mean miss the reference by more than 100 tolerances"""
    sep = mf.separation(case, kind)
    print(f"{mr.case_id(case)}-{kind}: F {sep['F']:.2e} = {sep['F'] / mf.TOL['F']:.1e} tolerances, "
          f"pix_mean {sep['pix_mean']:.2e} = {sep['pix_mean'] / mf.TOL['pix_mean']:.1e} tolerances")
    assert sep["F"] > 100 * mf.TOL["F"] and sep["pix_mean"] > 100 * mf.TOL["pix_mean"]


def test_dropping_the_vt_loop_in_float64_is_the_plain_reference():
    """``dropped=True`` really is the plain likelihood's Fisher information and leave-one-out (tests/fisher_reference.py,
    tests/loo_reference.py), in both number types"""
    case, kind = mr.case_named("c"), "one"
    ch, gp = mr.case_chunk(case), mr.case_gp(case)
    F, F_mu, loo = mf.case_ext(case, kind, True)
    F_ref, mu_ref = fr.fisher_ext(ch.lwls, ch.sigma, gp, *mf.case_tangents(case))
    assert fr.rel_to_scale(F, F_ref) <= 1e-15 and abs(F_mu - mu_ref) <= 1e-16 * mu_ref
    ref = lr.loo_ext(ch.lwls, ch.fl, ch.sigma, gp, mr.MU_GP, ch.epoch_index, ch.n_epochs)
    assert max(lr.errors(loo, ref).values()) <= 1e-15
    err = mf.errors(mf.case_f64(case, kind, True), (F, F_mu, loo))
    assert all(v <= mf.TOL[k] for k, v in err.items()), err


def test_planted_offset_is_decided_by_the_long_double_reference_alone():
    """the epoch moved by a constant within the prior: flagged under the plain K with a factor of ten to spare below the
    threshold of ``lnprob.loo_outliers`` (1e-4), and no epoch anywhere near it under the baseline"""
    marg, plain = mf.offset_epoch_sf(False), mf.offset_epoch_sf(True)
    print("epoch_sf under the baseline", marg, "under the plain K", plain)
    assert mf.OFFSET <= 2 * mf.WORKER_BASELINE["sd"][0]
    assert plain[mf.OFFSET_EPOCH] < 1e-5
    assert np.min(marg) > 1e-2


def test_worker_reference_under_the_baseline_is_far_from_the_plain_one():
    import orbit_ext as oe
    import orbit_grad_reference as ogr
    case = ogr.CHAIN_CASES[0]
    assert (case.model, case.N) == ("SB2", 129)
    ch = case.chunk
    vel = np.asarray(oe.velocities_ext("SB2", case.p_orb, ch.dates), dtype=np.float64)
    lwls = ch.lwl[None, :] + (-vel[:, ch.epoch_index]) / mf.C_KMS
    keep = list(range(6))                                 # every orbital parameter but gamma
    F = mf.worker_fisher_ext(ch, lwls, case.p_orb, case.gp, keep)
    plain = mf.worker_fisher_ext(ch, lwls, case.p_orb, case.gp, keep, dropped=True)
    sep = fr.rel_to_scale(plain, F)
    print(f"worker Fisher, marginal against plain: {sep:.2e} = {sep / mf.TOL['F']:.1e} tolerances")
    assert F.shape == (10, 10) and sep > 100 * mf.TOL["F"]
