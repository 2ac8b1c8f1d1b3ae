"""GPU tests of the gradient of ``lnprob(p)`` through the Kepler solve and the Doppler shift (psoap_chunk_lnprob_grad,
psoap_orbit_velocity_jacobian; psoap_amd/csrc/orbit_grad_kernels.hpp).

The tolerances are derived on the CPU, not fitted to the device (python tests/orbit_grad_reference.py):

* TOL_J: ``jacobian_f64`` (float64 NumPy on the device's Newton iteration restated) against ``jacobian_ext`` (long double,
  bisection) over orbit_cases.VEL_CASES, max |f64 - ext| / S_J with S_J the sum of the absolute product-rule terms of the entry:

      model         ecc     epochs      phase      roles
      SB1      3.33e-08   2.62e-12   1.30e-10   3.15e-14
      SB2      3.33e-08   2.89e-12   1.30e-10   3.55e-14
      ST1      3.33e-08   2.62e-12   1.30e-10   8.23e-14
      ST2      3.33e-08   7.52e-12   1.30e-10   1.58e-13
      ST3      3.33e-08   5.05e-12   1.30e-10   1.58e-13
      max      3.33e-08

  (the largest figure is e = 0.999 at a periastron passage, where D = 1 - e cos E = 1e-3 enters as 1/D^2 and one ulp of E
  costs 1e3 ulp of df/dM).  TOL_J = 8 x 3.33e-08 = 2.66e-07.

* TOL_ORB: the float64 host composition (``grad_f64`` on host-shifted grids, ``velocity_gradient``, ``jacobian_f64``) against
  ``chain_ext`` on CHAIN_CASES, max error / scale (S_orb[k] = sum_ce s_v[c, e] |J[c, e, k]|):

      case         grad_orb    grad_gp    grad_mu
      SB2-N129     1.62e-17   6.78e-18   4.58e-17
      SB1-N300     2.63e-17   1.70e-17   2.68e-17
      SB2-N300     9.63e-18   3.17e-17   1.02e-17
      ST3-N300     7.98e-17   5.49e-17   5.28e-18
      ST1-N128     2.66e-17   2.23e-17   3.02e-17
      max          7.98e-17   5.49e-17   4.58e-17

  TOL_ORB = 8 x 7.98e-17 = 6.38e-16; grad_gp and grad_mu keep the bounds of tests/test_gpu_grad.py (1.17e-15, 2.18e-16).

Measured on the device (MI355X): Jacobian 3.33e-08 of S_J for every model; grad_orb at most 1.87e-16 of S_orb, grad_gp
9.69e-17, grad_mu 7.72e-17; the fold at most 0.58 and the chain at most 0.006 of their summation bounds.

The margin of 8 is that of tests/test_gpu_grad.py: another summation order and fused multiply-adds, fp64 throughout.
The fold and the chain are held to the standard summation bound n u sum |terms|, u = 2^-53.
"""
import numpy as np
import pytest

import grad_reference as gr
import orbit_cases as oc
import orbit_grad_reference as ogr
from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu

MARGIN = 8
TOL_J = MARGIN * 3.33e-08
TOL_ORB = MARGIN * 7.98e-17
TOL_GP, TOL_MU = MARGIN * 1.46e-16, MARGIN * 2.73e-17          # tests/test_gpu_grad.py
LNP_RTOL = 1e-10
U = 2.0 ** -53
MODEL_OF_C = {1: "SB1", 2: "SB2", 3: "ST3"}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).copy()


def _same_bits(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _worker(model, lwl, fl, sigma, epoch_index, dates, **kw):
    from psoap_amd.lnprob import ChunkWorker
    return ChunkWorker(model, lwl, fl, sigma, epoch_index, dates, **kw)


def _case_worker(case, **kw):
    ch = case.chunk
    return _worker(case.model, ch.lwl, ch.fl, ch.sigma, ch.epoch_index, ch.dates, **kw)


# ---- 1. the Jacobian against long double ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", oc.MODELS)
def test_jacobian_against_long_double(model):
    from psoap_amd import orbit
    worst, n_cases = 0.0, 0
    for case in oc.VEL_CASES:
        if case.model != model:
            continue
        n_cases += 1
        vel, jac = orbit.velocity_jacobian(model, case.P, case.dates)
        assert np.array_equal(_bits(vel), _bits(orbit.velocities(model, case.P, case.dates))), case.name
        assert jac.shape == (len(case.P), oc.N_COMPONENTS[model], len(case.dates), ogr.N_ORB[model])
        for b, p in enumerate(case.P):
            Je, Se = ogr.jacobian_ext(model, p, case.dates)
            assert np.all(jac[b][Se == 0] == 0.0), case.name     # structural zeros
            r = ogr.rel_to_scale(jac[b], Je, Se)
            worst = max(worst, r)
            assert r <= TOL_J, (case.name, b, r, TOL_J)
    print(f"{model}: {n_cases} cases, largest |jac - ext| / S_J {worst:.2e} (bound {TOL_J:.2e})")
    assert n_cases >= 15


def test_st3_tertiary_has_zeros_in_the_inner_columns():
    from psoap_amd import orbit
    _, jac = orbit.velocity_jacobian("ST3", syn.make_orbit_proposals("ST3", 3, seed=800), oc.front_dates(65, seed=801))
    assert np.all(jac[:, 2, :, :6] == 0.0) and np.all(jac[:, 0, :, [0, 6]] == 0.0) and np.all(jac[:, 1, :, 6] == 0.0)
    assert np.all(jac[:, :, :, 12] == 1.0) and np.all(jac[:, 2, :, 6:12] != 0.0)


# ---- 2. the chain against long double ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ogr.CHAIN_CASES, ids=lambda c: c.id)
def test_chain_against_long_double(oracle, case):
    ch, ref = case.chunk, ogr.chain_ext(case)
    w = _case_worker(case)
    try:
        lnp, g_orb, g_gp, g_mu = w.lnprob_grad_orbits(case.p_orb, case.gp, gr.MU_GP)
    finally:
        w.close()
    vel = oc.kernel_restated(case.model, case.p_orb, ch.dates)
    want = oracle.lnlike(ch.lwl + (-vel[:, ch.epoch_index]) / oc.C_KMS, ch.fl, ch.sigma, case.gp, gr.MU_GP)
    err = {"orb": gr.rel_to_scale(g_orb[0], ref.orb, ref.s_orb), "gp": gr.rel_to_scale(g_gp[0], ref.grad.gp, ref.grad.s_gp),
           "mu": gr.rel_to_scale(g_mu[0], ref.grad.mu, ref.grad.s_mu)}
    tol = {"orb": TOL_ORB, "gp": TOL_GP, "mu": TOL_MU}
    print(f"{case.id}: lnp {lnp[0]!r} oracle {want!r}; error / S: " +
          ", ".join(f"{k} {v:.2e} (bound {tol[k]:.2e})" for k, v in err.items()))
    print("   grad_orb", g_orb[0], "ext", np.asarray(ref.orb, dtype=np.float64))
    assert abs(lnp[0] - want) <= LNP_RTOL * max(1.0, abs(want))
    for k in err:
        assert err[k] <= tol[k], (k, err[k], tol[k])


# ---- 3. the fold and the chain against their pinned inputs, at the reduction edges ------------------------------------------
def _front_cases():
    out = [(c, ne, 1000) for ne in oc.EPOCH_COUNTS for c in (1, 2, 3)]
    return out + [(2, 300, 100)]             # n_epochs > n_target: one pixel per epoch at most, two epochs in three empty


@pytest.mark.parametrize("c,ne,n_target", _front_cases(), ids=lambda v: str(v))
def test_fold_and_chain_against_their_inputs(c, ne, n_target):
    from psoap_amd import covariance, orbit
    model = MODEL_OF_C[c]
    fc = oc.front_chunk(c, ne, seed=900 + 7 * ne + c, n_target=n_target)
    counts = np.bincount(fc.epoch_index, minlength=ne)
    if n_target < ne:
        assert counts.min() == 0
    P = syn.make_orbit_proposals(model, 2, seed=910 + ne)
    gps = syn.make_walkers(c, 2, seed=911 + ne)
    w = _worker(model, fc.lwl, fc.fl, fc.sigma, fc.epoch_index, fc.dates)
    try:
        lnp, g_orb, g_gp, g_mu, g_vel = w.lnprob_grad_orbits(P, gps, gr.MU_GP, want_vel=True)
        vel, jac = orbit.velocity_jacobian(model, P, fc.dates)
        _, _, g_lwl, _ = w.handle.lnlike_grad(oc.grids_from_velocities(fc, vel), gps, gr.MU_GP)
    finally:
        w.close()
    assert np.all(np.isfinite(lnp)) and g_vel.shape == (2, c, ne)
    # the fold: n = the largest pixel count of an epoch
    host = covariance.velocity_gradient(g_lwl, fc.epoch_index, ne)
    mag = covariance.velocity_gradient(-np.abs(g_lwl), fc.epoch_index, ne)          # sum |terms| / c_kms
    bound = counts.max() * U * mag
    print(f"c{c} ne{ne}: fold largest |device - host| / bound {np.max(np.abs(g_vel - host) / np.where(bound > 0, bound, 1)):.3f}")
    assert np.all(np.abs(g_vel - host) <= bound)
    assert np.all(g_vel[:, :, counts == 0] == 0.0) and not np.any(np.signbit(g_vel[:, :, counts == 0]))
    # the chain: n = c * n_epochs
    want = np.einsum("bce,bcek->bk", g_vel, jac)
    bound = c * ne * U * np.einsum("bce,bcek->bk", np.abs(g_vel), np.abs(jac))
    print(f"c{c} ne{ne}: chain largest |device - host| / bound {np.max(np.abs(g_orb - want) / np.where(bound > 0, bound, 1)):.3f}")
    assert np.all(np.abs(g_orb - want) <= bound)


# ---- 4. bits ---------------------------------------------------------------------------------------------------------------
def test_bits_against_the_pieces_and_across_batches():
    from psoap_amd import orbit
    case = ogr.CHAIN_CASES[0]                   # SB2, N = 129: two tile rows
    ch = case.chunk
    P = syn.make_orbit_proposals("SB2", 10, seed=920)
    gps = syn.make_walkers(2, 10, seed=921)
    w = _case_worker(case)
    try:
        three = w.lnprob_grad_orbits(P[:3], gps[:3], gr.MU_GP, want_vel=True)
        again = w.lnprob_grad_orbits(P[:3], gps[:3], gr.MU_GP, want_vel=True)
        ten = w.lnprob_grad_orbits(P, gps, gr.MU_GP, want_vel=True)
        singles = [w.lnprob_grad_orbits(P[b], gps[b], gr.MU_GP, want_vel=True) for b in range(10)]
        lw = ch.lwl + (-orbit.velocities("SB2", P, ch.dates)[:, :, ch.epoch_index]) / oc.C_KMS
        pieces = w.handle.lnlike_grad(lw, gps, gr.MU_GP)
    finally:
        w.close()
    assert three[0].shape == (3,) and three[1].shape == (3, 7) and three[2].shape == (3, 4) and three[4].shape == (3, 2, 5)
    assert _same_bits(three, again)
    assert len({float(v) for v in ten[0]}) == 10
    # lnp, grad_gp, grad_mu: the bits of lnlike_grad on the grids of psoap_orbit_velocities and the host shift
    assert _same_bits([ten[0], ten[2], ten[3]], [pieces[0], pieces[1], pieces[3]])
    for b in range(10):
        assert _same_bits([v[b] for v in ten], [v[0] for v in singles[b]]), b
        if b < 3:
            assert _same_bits([v[b] for v in three], [v[0] for v in singles[b]]), b


# ---- 5. conventions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", oc.FAST_POSITIONS)
def test_fast_proposals_give_minus_inf_and_leave_the_others_alone(where):
    B = 4
    for case in oc.FAST_CASES:
        c = oc.N_COMPONENTS[case.model]
        fc = oc.front_chunk(c, len(case.dates), seed=930 + c, n_target=120)
        fast, _slow, i = oc.fast_batch(case, B, where)
        gps = syn.make_walkers(c, B, seed=931)
        w = _worker(case.model, fc.lwl, fc.fl, fc.sigma, fc.epoch_index, case.dates)
        try:
            out = w.lnprob_grad_orbits(fast, gps, gr.MU_GP, want_vel=True)
            solo = {b: w.lnprob_grad_orbits(fast[b], gps[b], gr.MU_GP, want_vel=True) for b in range(B) if b != i}
        finally:
            w.close()
        assert np.isneginf(out[0][i]) and all(np.all(np.isnan(v[i])) for v in out[1:]), case.name
        for b, one in solo.items():
            assert np.isfinite(out[0][b]) and _same_bits([v[b] for v in out], [v[0] for v in one]), (case.name, b)


def test_negative_amplitude_open_stream_and_the_handle_is_left_as_it_was():
    from psoap_amd._lib import PsoapError
    case = ogr.CHAIN_CASES[2]                   # SB2, N = 300
    ch = case.chunk
    P = syn.make_orbit_proposals("SB2", 4, seed=940)
    gps = syn.make_walkers(2, 4, seed=941)
    lw = syn.walker_lwls(ch, syn.make_walker_velocities(ch, 4, seed=942))
    w = _case_worker(case, max_batch=4)
    try:
        h = w.handle
        h.upload(lw, gps, gr.MU_GP)
        h.eval()
        before = h.fetch()
        bad = gps.copy()
        bad[1, 0] = -0.5
        out = w.lnprob_grad_orbits(P, bad, 1.1, want_vel=True)
        assert np.isneginf(out[0][1]) and all(np.all(np.isnan(v[1])) for v in out[1:])
        assert np.all(np.isfinite(out[0][[0, 2, 3]])) and np.all(np.isfinite(out[1][[0, 2, 3]]))
        assert _same_bits([h.fetch()], [before])                 # the earlier evaluation's results, untouched
        h.upload(lw[::-1].copy(), gps[::-1].copy(), gr.MU_GP)    # and an uploaded batch survives a gradient call
        w.lnprob_grad_orbits(P[:2], gps[:2], gr.MU_GP)
        h.eval()
        assert _same_bits([h.fetch()], [before[::-1]])
        w.stream_open()
        with pytest.raises(PsoapError, match="open stream"):
            w.lnprob_grad_orbits(P, gps, gr.MU_GP)
        w.stream_close()
        h.grad_release()
        assert _same_bits(w.lnprob_grad_orbits(P[0], gps[0], 1.1, want_vel=True), [v[:1] for v in out])
    finally:
        w.close()


# ---- 6. optimize_orbit -----------------------------------------------------------------------------------------------------
def _orbit_chunk(p_true, seed, n_epochs=6, n_pix=50):
    """a synthetic SB2 chunk whose spectra move with the orbit ``p_true`` (the recipe of synthetic.make_chunk)"""
    rng = np.random.default_rng(seed)
    dates = syn.make_dates(n_epochs, seed)
    delta = 2.7 / syn.C_KMS
    lwl = (np.log(5200.0) + np.arange(n_pix) * delta + (rng.uniform(-0.5, 0.5, size=n_epochs) * delta)[:, None]).ravel()
    mask = np.ones((n_epochs, n_pix), dtype=bool)
    lwls = syn.replicate_wls(lwl, oc.kernel_restated("SB2", p_true, dates), mask)
    fl = np.ones_like(lwl)
    for k, ratio in enumerate((1.0, 0.4)):
        centres = rng.uniform(lwls[k].min() + 15 * delta, lwls[k].max() - 15 * delta, size=2)
        fl = fl + syn._template(lwls[k], centres, rng.uniform(0.2, 0.5, size=2) * ratio)
    fl = fl + 0.02 * rng.standard_normal(lwl.shape[0])
    return lwl, fl, np.full(lwl.shape[0], 0.02), syn.epoch_index_from_mask(mask), dates


def test_optimize_orbit_on_two_chunks():
    from psoap_amd.lnprob import optimize_orbit
    from psoap_amd.utils import registered_params
    p_true = np.array(syn.ORBIT_BASE["SB2"])
    full = dict(zip(registered_params["SB2"], list(p_true) + list(syn.GP_BASE[2])))
    fix = [n for n in registered_params["SB2"] if n not in ("q", "K")]
    workers = [_worker("SB2", *_orbit_chunk(p_true, seed), fix_params=fix, defaults=full) for seed in (950, 951)]
    try:
        assert all(w.handle.N == 300 for w in workers)
        start = np.array([full["q"] * 1.05, full["K"] * 0.95])
        res = optimize_orbit(workers, start, bounds=[(0.1, 2.0), (1.0, 40.0)], full_output=True)
        l_start = sum(w.lnprob(start) for w in workers)
        l_end = sum(w.lnprob(res.x) for w in workers)
        fresh = sum(w.lnprob_grad(res.x)[1] for w in workers)
    finally:
        for w in workers:
            w.close()
    print(f"start {start} lnprob {l_start!r}; L-BFGS-B {res.x} lnprob {l_end!r} in {res.nfev} evaluations: {res.message}")
    assert res.success and l_end >= l_start
    assert np.array_equal(np.asarray(res.jac), -fresh)
