"""CPU tests of tests/marg_tv_reference.py, the references of the time-variable kernel under the marginalised continuum:
the float64 twin of the device's route against the long-double evaluation on the dense Kt within the table the device's
tolerances are taken from; tau = inf reproduces the static marginal references exactly; every seeded defect of the twin's
dlnL/dtau leaves the device's tolerance."""
import numpy as np
import pytest

import marg_fisher_reference as mfr
import marg_grad_reference as mgr
import marg_reference as mr
import marg_tv_reference as mt

INF = float("inf")


@pytest.fixture(scope="module")
def table():
    return mt.measure_f64()


def test_the_twin_agrees_with_long_double_within_the_recorded_table(table):
    """a fresh measurement does not exceed F64_MAX (the last row of ``python tests/marg_tv_reference.py``), and is of its
    size: a table ten times too generous would hide a twin that got worse"""
    assert len(table) == len(mr.CASES) * len(mr.WEIGHTS)
    for k, bound in mt.F64_MAX.items():
        worst = max(err[k] for _, err in table)
        assert worst <= bound * 1.005, (k, worst, bound)          # (the table is printed with three digits)
        assert worst >= bound / 10, (k, worst, bound)
    worst = max(err["lnp"] for _, err in table)
    assert worst <= mt.LNP_RTOL / mt.MARGIN and mt.LNP_F64_MAX / 10 <= worst <= mt.LNP_F64_MAX * 1.005


def test_the_cases_mix_finite_and_infinite_time_scales():
    for case in mr.CASES:
        tau, (t, span) = mt.case_tau(case), mt.case_times(case)
        assert tau.shape == (case[2],) and np.any(np.isfinite(tau)) and (case[2] == 1 or np.any(np.isinf(tau)))
        assert t.shape == (case[1],) and t.min() == 0.0 and t.max() == span > 0
        # one time per run of pixels
        ep = mr.case_chunk(case).epoch_index
        assert all(len(set(t[ep == e])) <= 1 for e in range(case[3]))
        ref = mt.case_ext(case, "one")
        assert np.all(np.asarray(ref.tau)[np.isinf(tau)] == 0) and np.all(np.asarray(ref.tau)[np.isfinite(tau)] != 0)
        dead = 2 * case[2] + np.flatnonzero(np.isinf(tau))
        assert np.all(ref.F[dead, :] == 0) and np.all(ref.F[:, dead] == 0) and ref.F.shape == (3 * case[2] + 1,) * 2


@pytest.mark.parametrize("kind", mr.WEIGHTS)
@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_id)
def test_infinite_tau_reproduces_the_static_marginal_twins_exactly(case, kind):
    """float64, bit for bit.  At tau = inf the temporal term is a signed zero and the arguments of exp() keep the static bits;
    the static twins fill K with the oracle's exp() and ``matrix_f64`` with numpy's, so the twin is given the static twins'
    own K: the value and the gradient of ``marg_grad_reference.marg_grad_f64``, parts, beta, beta_cov and fl_cor of
    ``marg_reference.marg_f64`` to the float64 table, F and F_mu of ``marg_fisher_reference``, and an exactly-zero grad_tau and dtau rows"""
    import oracle
    import timevar_reference as tr
    ch, c, gp = mr.case_chunk(case), case[2], mr.case_gp(case)
    tau = np.full(c, INF)
    _, args = tr.matrix_f64(ch.lwls, mt.case_times(case)[0], gp, tau, ch.sigma, want_args=True)
    for k in range(c):
        D = ch.lwls[k][None, :] - ch.lwls[k][:, None]
        static = -0.5 * (tr.C_KMS * tr.C_KMS) / (gp[2 * k + 1] * gp[2 * k + 1]) * D * D
        assert np.array_equal(args[k].view(np.int64), static.view(np.int64))
    K = np.empty((case[1], case[1]))
    oracle.fill_sym(K, ch.lwls, gp)
    K[np.diag_indices_from(K)] += ch.sigma ** 2
    got = mt.case_f64(case, kind, tau=tau, K=K)
    assert np.all(got.tau == 0.0)
    dead = slice(2 * c, 3 * c)
    assert np.all(got.F[dead, :] == 0.0) and np.all(got.F[:, dead] == 0.0)
    value, grad = mr.marg_f64(*mr._case_args(case, kind)), mgr.marg_grad_f64(*mr._case_args(case, kind))
    assert got.lnp == grad.lnp
    # (``marg_reference.marg_f64`` hands SciPy the factor in another memory order: the same formulas, not the same bits)
    side = mr.errors(got, value, mr.prior_sd(case[5]))
    assert all(side[k] <= mt.F64_MAX.get(k, 1e-13) for k in side), side
    assert np.array_equal(got.gp, grad.gp) and np.array_equal(got.lwl, grad.lwl) and got.mu == grad.mu
    wood = mfr.woodbury_f64(*mr._case_args(case, kind))
    tan_lwl, tan_gp, _ = mt.case_tangents(case)
    keep = [k for k in range(3 * c + 1) if not 2 * c <= k < 3 * c]
    F_static, F_mu = mfr.fisher_f64(wood, ch.lwls, gp, tan_lwl[keep], tan_gp[keep])
    assert np.array_equal(got.F[np.ix_(keep, keep)], F_static) and got.F_mu == F_mu


def test_infinite_tau_in_long_double_is_the_static_marginal_reference():
    """... and the long-double evaluation at tau = inf has the bits of ``marg_grad_reference.marg_grad_ext``"""
    case = mr.case_named("a")
    ref = mt.marg_tv_ext(*mt.case_args(case, "flux", tau=np.full(2, INF)))
    static = mgr.case_ext(case, "flux")
    assert ref.lnp == static.lnp and ref.mu == static.mu
    assert np.array_equal(ref.gp, static.gp) and np.array_equal(ref.lwl, static.lwl)
    assert np.all(ref.tau == 0) and np.all(ref.s_tau == 0)


@pytest.mark.parametrize("defect", mt.DEFECTS)
def test_every_seeded_defect_leaves_the_tolerance(defect, table):
    """on every case and weight the defective dlnL/dtau misses the device's bound on grad_tau, by orders of magnitude"""
    rows = mt.measure_f64(defect, fisher=False)
    smallest = min(err["grad_tau"] for _, err in rows)
    print(f"{defect}: smallest grad_tau error / scale over the cases {smallest:.2e}, tolerance {mt.TOL['grad_tau']:.2e}")
    assert smallest > 1e6 * mt.TOL["grad_tau"]
    # ... and touches nothing else
    sound = dict(table)
    for name, err in rows:
        assert all(err[k] == sound[name][k] for k in err if k != "grad_tau")
