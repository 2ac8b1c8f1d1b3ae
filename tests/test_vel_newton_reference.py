"""CPU tests of the references of the observed information of the epoch velocities (tests/vel_newton_reference.py): the
long-double generic J pinned by central differences of the long-double gradient, its symmetry, null directions and
expectation; the float64 twin of the device's structured form within its recorded table; the seeded defects; the twins of the
two fits."""
import numpy as np
import pytest

import vel_fisher_reference as vr
import vel_newton_reference as nr

SMALL = nr.SHAPES[0]                     # N = 100, c = 2, 4 epochs


@pytest.mark.parametrize("order", nr.BASELINES, ids=lambda o: "plain" if o is None else f"b{o}")
def test_long_double_J_against_central_differences_of_the_long_double_gradient(order):
    err, bound, h = nr.fd_pin(SMALL, order)
    print(f"order {order}: h = {h:.3e} km/s, |J_fd - J| / sqrt(F_ss F_tt) = {err:.2e} (bound {bound:.2e})")
    assert err <= bound


@pytest.mark.parametrize("order", nr.BASELINES, ids=lambda o: "plain" if o is None else f"b{o}")
def test_symmetry_null_directions_and_the_twin(order):
    pr = nr.problem(SMALL)
    lnp, g, F, J = nr.shape_ext(SMALL, order)
    d = np.sqrt(np.abs(np.diag(F))).astype(np.float64)
    asym = float(np.max(np.abs(np.asarray(J - J.T, dtype=np.float64)) / np.outer(d, d)))
    assert asym <= 1e-17 * 100                       # U^T G U is formed as a product: symmetric to long double's rounding
    scale = d * np.sum(d)
    null = float(max(np.max(np.abs(np.asarray(J @ u, dtype=np.float64)) / scale) for u in vr.null_vectors(pr.c, pr.E)))
    assert null <= 1e-17 * 100                       # long double: 100 roundings of 2^-64
    assert vr.null_residual(np.asarray(F, dtype=np.float64), pr.c, pr.E) <= 1e-15
    assert abs(float(np.sum(g.reshape(pr.c, pr.E), axis=1).max())) <= 1e-15 * float(np.max(np.abs(g)) + d.max())
    err = nr.errors(nr.shape_f64(SMALL, order), (lnp, g, F, J))
    print(f"order {order}: " + ", ".join(f"{k} {err[k]:.2e}" for k in nr.OUTPUTS) + f"; |J u_c| {null:.2e}")
    assert all(err[k] <= 1.01 * nr.F64_MAX[k] for k in nr.OUTPUTS)     # the recorded table (three digits) holds what the twin gives


def test_the_recorded_maxima_are_what_the_twin_gives_at_their_rows():
    """F64_MAX is the last row of the float64 table (python tests/vel_newton_reference.py: every shape x baseline, half a
    minute); here the rows that set it.  The figures are recorded to three digits, and the twin's rounding may differ a little
    between BLAS builds: at its own row each maximum is met within [1/2, 1.01] -- a table that drifted by a factor either way
    fails -- and no output of those rows exceeds it."""
    shapes = {sh.name: sh for sh in nr.SHAPES}
    for k, (name, order) in nr.F64_MAX_AT.items():
        err = nr.errors(nr.shape_f64(shapes[name], order), nr.shape_ext(shapes[name], order))
        print(f"{name} order {order}: " + ", ".join(f"{o} {err[o]:.2e} (max {nr.F64_MAX[o]:.2e})" for o in nr.OUTPUTS))
        assert 0.5 * nr.F64_MAX[k] <= err[k] <= 1.01 * nr.F64_MAX[k], k
        assert all(err[o] <= 1.01 * nr.F64_MAX[o] for o in nr.OUTPUTS)


@pytest.mark.parametrize("order", (None, 0), ids=("plain", "b0"))
def test_seeded_defects_leave_the_bound_and_the_within_epoch_block_cancels(order):
    ref = nr.shape_ext(SMALL, order)
    for defect in nr.DEFECTS:
        err = nr.errors(nr.shape_f64(SMALL, order, defect), ref)["J"]
        print(f"{defect}: J {err:.2e} (bound {nr.TOL['J']:.2e})")
        assert err > 1e4 * nr.TOL["J"], defect
    kept = nr.errors(nr.shape_f64(SMALL, order, nr.NOT_A_DEFECT), ref)["J"]
    print(f"{nr.NOT_A_DEFECT}: J {kept:.2e}")
    assert kept <= nr.TOL["J"]                       # W_k's within-epoch block goes in and out of T_k again: no defect


def test_the_mean_of_J_over_model_drawn_fluxes_approaches_F():
    """E[alpha alpha^T] = G, so E[J] = F.  n draws of the float64 twin at fluxes N(mu, K + sigma^2): every entry of the mean,
    in units of sqrt(F_ss F_tt), is bounded by 5 times its own standard error over the draws (a 5 sigma excursion in one of
    64 entries: 4e-5), and the draws are enough to tell F from 0.75 F on the diagonal at that level."""
    import oracle
    pr = nr.problem(SMALL)
    K = np.empty((pr.lwls.shape[1],) * 2)
    oracle.fill_sym(K, pr.lwls, pr.gp)
    K[np.diag_indices_from(K)] += pr.sigma ** 2
    L = np.linalg.cholesky(K)
    rng = np.random.default_rng(8600)
    n = 400
    Js = []
    for _ in range(n):
        fl = nr.MU_GP + L @ rng.standard_normal(pr.lwls.shape[1])
        _, _, F, J = nr.info_f64(pr.lwls, fl, pr.sigma, pr.gp, pr.ep, pr.E)
        Js.append(J)
    Js = np.array(Js)
    d = np.sqrt(np.diag(F))
    mean, se = Js.mean(axis=0) / np.outer(d, d), Js.std(axis=0, ddof=1) / np.sqrt(n) / np.outer(d, d)
    dev = np.abs(mean - F / np.outer(d, d))
    print(f"{n} draws: max |mean J - F| / se = {np.max(dev / se):.2f}; largest se {se.max():.3f}")
    assert np.all(dev <= 5.0 * se)
    assert np.all(0.25 >= 5.0 * np.diag(se))


def test_twins_of_the_fits_and_the_hard_seed():
    """Newton's twin converges on fit_chunk in no more iterations than scoring's; at HARD_SEED scoring misses 20 iterations and
    Newton does not; under the baseline a prior-sized continuum offset per epoch moves the plain fit by more than the
    marginalised one, which stays within its error bars"""
    ch = vr.fit_chunk()
    assert np.array_equal(nr.fit_chunk().fl, ch.fl)
    scoring, start = vr.cpu_fit_optimum()
    newton = nr.cpu_newton(ch, vr.fit_gp(), start)
    again = vr.cpu_fit(ch, vr.fit_gp(), start)
    sig = np.sqrt(np.diag(newton["cov"])).reshape(newton["vel"].shape)
    print(f"newton {newton['n_iter']} iterations, scoring {again['n_iter']}; max |v_newton - v_scoring| / sigma "
          f"{np.max(np.abs(newton['vel'] - again['vel']) / sig):.2e}")
    assert newton["converged"] and newton["cov_kind"] == "observed" and newton["n_iter"] <= again["n_iter"]
    assert newton["lnp"] >= newton["lnp_start"]
    assert np.max(np.abs(newton["vel"] - again["vel"]) / sig) <= 1e-4
    hard = nr.fit_chunk(nr.HARD_SEED)
    assert not vr.cpu_fit(hard, vr.fit_gp(), hard.velocities)["converged"]
    assert nr.cpu_newton(hard, vr.fit_gp(), hard.velocities)["converged"]
    fl_off, off = nr.offset_flux(ch)
    assert np.max(np.abs(off)) <= 3 * nr.FIT_BASELINE["sd"][0]
    v0, sd = ch.velocities, nr.FIT_BASELINE["sd"]
    plain = [nr.cpu_newton(ch, vr.fit_gp(), v0, fl=f) for f in (ch.fl, fl_off)]
    marg = [nr.cpu_newton(ch, vr.fit_gp(), v0, fl=f, order=0, sd=sd) for f in (ch.fl, fl_off)]
    s_plain = np.sqrt(np.diag(plain[1]["cov"])).reshape(v0.shape)
    s_marg = np.sqrt(np.diag(marg[1]["cov"])).reshape(v0.shape)
    move_plain = np.max(np.abs(plain[1]["vel"] - plain[0]["vel"]) / s_plain)
    move_marg = np.max(np.abs(marg[1]["vel"] - marg[0]["vel"]) / s_marg)
    print(f"offsets {np.round(off, 3)}: the plain fit moves by {move_plain:.3f} sigma, the marginalised one by {move_marg:.3f}")
    assert all(f["converged"] for f in plain + marg)
    assert move_marg <= 1.0 and move_plain > move_marg
