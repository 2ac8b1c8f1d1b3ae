"""GPU tests of the epoch-velocity Fisher information (psoap_chunk_fisher_vel, psoap_amd/csrc/vel_fisher_kernels.hpp) and of
the per-epoch velocity fit on top of it (psoap_amd.lnprob.epoch_velocities).

Shapes at the edges of the 128-row tiles (tests/fisher_reference.py: CASES), masked chunks with unequal epochs, an epoch that
straddles row 128, the benchmark hyper-parameters; all c E velocity tangents.  The device's F against the long-double
reference (fisher_reference.fisher_ext with those tangents), every entry, relative to sqrt(F_ss F_tt).

The tolerance is derived, not fitted: the float64 SciPy evaluation of the structured formula (vel_fisher_reference.vel_fisher_f64)
measured against the long-double one on these very cases (python tests/vel_fisher_reference.py):

    case                F
    N100-c2      7.50e-15
    N128-c2      4.47e-14
    N129-c2      1.21e-14
    N300-c1      2.48e-14
    N300-c2      3.25e-14
    N300-c3      1.95e-14
    max          4.47e-14

The device sums in another order and fuses multiply-adds but is fp64 throughout: it gets the largest measured value times the
project's margin of 8 (tests/test_gpu_grad.py): 8 x 4.47e-14 = 3.58e-13.  Against the device's own generic Fisher
information the two tests' tolerances add: 3.58e-13 + 4.06e-13 (tests/test_gpu_fisher.py).
"""
import numpy as np
import pytest

import fisher_reference as fr
import grad_reference as gr
import vel_fisher_reference as vr
from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu

MARGIN = 8
F64_REL = 4.47e-14                     # the table above, last row
TOL = MARGIN * F64_REL
TOL_GENERIC = TOL + 8 * 5.07e-14       # + tests/test_gpu_fisher.py: TOL["F"]


def _handle(ch, **kw):
    from psoap_amd.chunk import ChunkHandle
    return ChunkHandle(ch.fl, ch.sigma, **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).copy()


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _null_residual(F, c, E):
    d = np.sqrt(np.diag(F))
    scale = d * np.sum(d)
    scale[scale == 0.0] = 1.0
    return float(max(np.max(np.abs(F @ u) / scale) for u in vr.null_vectors(c, E)))


@pytest.mark.parametrize("case", vr.CASES, ids=fr.case_id)
def test_against_long_double(case):
    ch, gp, c, E = gr.case_chunk(case), gr.case_gp(case), case[1], case[2]
    F_ref = vr.case_ext(case)
    with _handle(ch) as h:
        F = h.fisher_vel(ch.lwls, gp, ch.epoch_index, E)
    err, null = vr.rel_to_scale(F, F_ref), _null_residual(F, c, E)
    print(f"{fr.case_id(case)}: F {err:.2e}, |F u_c| {null:.2e} (bound {TOL:.2e})")
    assert F.shape == (c * E, c * E) and np.all(np.isfinite(F))
    assert _same_bits(F, F.T)
    assert err <= TOL and null <= TOL


def test_more_tangents_than_the_generic_path_takes():
    """c = 3, 12 epochs: c E = 36; the same recipe with 11 epochs: c E = 33; the generic call with the 36 tangents is refused"""
    from psoap_amd._lib import PsoapError
    for case in (vr.CASE_36, vr.CASE_33):
        ch, gp, c, E = gr.case_chunk(case), gr.case_gp(case), case[1], case[2]
        assert ch.N == 300 and c * E > 32 and np.all(np.bincount(ch.epoch_index, minlength=E) > 0)
        F_ref = vr.case_ext(case)
        with _handle(ch) as h:
            F = h.fisher_vel(ch.lwls, gp, ch.epoch_index, E)
            if case is vr.CASE_36:
                tan_lwl, tan_gp = vr.vel_tangents(case)
                with pytest.raises(PsoapError, match="tangents"):
                    h.fisher(ch.lwls, gp, tan_gp, tan_lwl)
        err = vr.rel_to_scale(F, F_ref)
        print(f"c E = {c * E}: F {err:.2e} (bound {TOL:.2e})")
        assert F.shape == (c * E, c * E) and _same_bits(F, F.T) and err <= TOL


@pytest.mark.parametrize("case", vr.CASES, ids=fr.case_id)
def test_against_the_generic_fisher_of_the_device(case):
    ch, gp, c, E = gr.case_chunk(case), gr.case_gp(case), case[1], case[2]
    tan_lwl, tan_gp = vr.vel_tangents(case)
    assert c * E <= 32
    with _handle(ch) as h:
        F = h.fisher_vel(ch.lwls, gp, ch.epoch_index, E)
        generic = h.fisher(ch.lwls, gp, tan_gp, tan_lwl)
    err = vr.rel_to_scale(F, generic)
    print(f"{fr.case_id(case)}: against h.fisher {err:.2e} (bound {TOL_GENERIC:.2e})")
    assert err <= TOL_GENERIC


def test_structure_repeat_single_epoch_unused_indices_permutation():
    case = vr.CASES[4]                        # N = 300, c = 2, 6 unequal epochs: three tile rows
    ch, gp, c, E = gr.case_chunk(case), gr.case_gp(case), case[1], case[2]
    ep = ch.epoch_index
    wide = np.array([0, 2, 3, 5, 6, 7])[ep]   # the same epochs under 8 indices: 1 and 4 unused
    perm = np.random.default_rng(8100).permutation(ch.N)
    from psoap_amd.chunk import ChunkHandle
    with _handle(ch) as h:
        F = h.fisher_vel(ch.lwls, gp, ep, E)
        again = h.fisher_vel(ch.lwls, gp, ep, E)
        one = h.fisher_vel(ch.lwls, gp, np.zeros(ch.N, dtype=np.int64), 1)
        Fw = h.fisher_vel(ch.lwls, gp, wide, 8)
        default_E = h.fisher_vel(ch.lwls, gp, ep)
    with ChunkHandle(ch.fl[perm], ch.sigma[perm]) as h:
        Fp = h.fisher_vel(ch.lwls[:, perm], gp, ep[perm], E)
    assert _same_bits(F, F.T) and _same_bits(F, again) and _same_bits(F, default_E)
    assert one.shape == (c, c) and np.all(one == 0.0)
    used = [k * 8 + e for k in range(c) for e in (0, 2, 3, 5, 6, 7)]
    unused = [k * 8 + e for k in range(c) for e in (1, 4)]
    assert Fw.shape == (c * 8, c * 8) and np.all(Fw[unused] == 0.0) and np.all(Fw[:, unused] == 0.0)
    assert _same_bits(Fw[np.ix_(used, used)], F) and _same_bits(Fw, Fw.T)
    err = vr.rel_to_scale(Fp, vr.case_ext(case))
    err_perm = vr.rel_to_scale(Fp, F)
    print(f"permuted pixels: against long double {err:.2e}, against the unpermuted chunk {err_perm:.2e} (bound {TOL:.2e}); "
          f"|F u_c| {_null_residual(F, c, E):.2e}")
    assert _same_bits(Fp, Fp.T) and err <= TOL and err_perm <= TOL
    assert _null_residual(F, c, E) <= TOL


def test_conventions_and_the_handle_is_left_as_it_was():
    from psoap_amd._lib import PsoapError
    from psoap_amd.chunk import ChunkHandle
    case = vr.CASES[4]
    ch, gp, c, E = gr.case_chunk(case), gr.case_gp(case), case[1], case[2]
    ep = ch.epoch_index
    gps = syn.make_walkers(c, 4, seed=8200)
    lw = syn.walker_lwls(ch, syn.make_walker_velocities(ch, 4, seed=8201))
    with _handle(ch, max_batch=4) as h:
        before = h.lnlike_batch(lw, gps, 0.9)
        h.upload(lw[::-1].copy(), gps[::-1].copy(), 0.9)
        good = h.fisher_vel(ch.lwls, gp, ep, E)
        h.eval()
        assert _same_bits(h.fetch(), before[::-1]) and _same_bits(h.lnlike_batch(lw, gps, 0.9), before)
        neg = gp.copy()
        neg[0] = -neg[0]
        F = h.fisher_vel(ch.lwls, neg, ep, E)                 # status 0: no exception
        assert F.shape == (c * E, c * E) and np.all(np.isnan(F))
        bad = ep.copy()
        bad[17] = E
        with pytest.raises(PsoapError, match="epoch index out of range"):
            h.fisher_vel(ch.lwls, gp, bad, E)
        bad[17] = -1
        with pytest.raises(PsoapError, match="epoch index out of range"):
            h.fisher_vel(ch.lwls, gp, bad, E)
        with pytest.raises(PsoapError, match="n_epochs must be at least 1"):
            h.fisher_vel(ch.lwls, gp, ep, 0)
        h.stream_open(c, 1)
        try:
            with pytest.raises(PsoapError, match="open stream"):
                h.fisher_vel(ch.lwls, gp, ep, E)
        finally:
            h.stream_close()
        # release, twice, then another call: the workspace comes back, and so do the bits
        h.fisher_vel_release()
        h.fisher_vel_release()
        h.fisher_release()
        assert _same_bits(h.fisher_vel(ch.lwls, gp, ep, E), good)
    # not positive definite: zero noise and two identical pixels
    lw1 = ch.lwls.copy()
    lw1[:, 1] = lw1[:, 0]
    with ChunkHandle(ch.fl, np.zeros_like(ch.sigma)) as h:
        assert np.all(np.isnan(h.fisher_vel(lw1, gp, ep, E)))


def test_covariance_velocity_information_through_the_cached_handle():
    from psoap_amd import covariance
    case = vr.CASES[0]
    ch, gp, c, E = gr.case_chunk(case), gr.case_gp(case), case[1], case[2]
    try:
        F = covariance.velocity_information(ch.lwls, ch.fl, ch.sigma, gp, ch.epoch_index)
        bad = covariance.velocity_information(ch.lwls, ch.fl, ch.sigma, [-0.2, 5.0, 0.1, 7.0], ch.epoch_index)
    finally:
        covariance.release_handles()
    assert F.shape == (c * E, c * E) and np.all(np.isnan(bad)) and bad.shape == F.shape
    assert vr.rel_to_scale(F, vr.case_ext(case)) <= TOL


# ---- the fit: lnprob.epoch_velocities -----------------------------------------------------------------------------------
def _fit_worker(ch, keep=None, **kw):
    from psoap_amd.lnprob import ChunkWorker
    from psoap_amd.utils import registered_params
    full = dict(zip(registered_params["SB2"], list(syn.ORBIT_BASE["SB2"]) + list(vr.fit_gp())))
    sel = slice(None) if keep is None else keep
    return full, ChunkWorker("SB2", ch.lwl[sel], ch.fl[sel], ch.sigma[sel], ch.epoch_index[sel], ch.dates, defaults=full, **kw)


def _fit_from(workers, full, start):
    """epoch_velocities started from the table ``start`` instead of the orbit's velocities at p"""
    from psoap_amd import lnprob
    from psoap_amd.utils import registered_params
    p = np.array([full[n] for n in registered_params["SB2"]])
    return lnprob.epoch_velocities(workers, p, mu_GP=vr.FIT_MU, vel0=start)


def test_fit_against_the_cpu_twin(tmp_path):
    """SB2, 6 epochs x 50 pixels, from 1 km/s off the CPU twin's optimum: both fits are within sqrt(1e-10) = 1e-5 sigma of the
    stationary point by the stopping rule; the bound of 1e-4 sigma leaves the rest to rounding in F^+.

    The chunk rests on a chosen seed (vel_fisher_reference.FIT_SEED): Fisher scoring converges linearly and most seeds of this
    small shape do not reach the decrement within 20 iterations.  A change to synthetic.make_chunk or to NumPy's random stream
    moves the chunk and can turn this test and tests/test_vel_fisher_reference.py::test_cpu_twin_of_the_fit_converges red for
    no fault of the device code: if the CPU twin fails too, choose a seed at which it converges (the comment at FIT_SEED says how
    the present one was found) before looking for a defect here."""
    ch = vr.fit_chunk()
    twin, start = vr.cpu_fit_optimum()
    full, w = _fit_worker(ch)
    try:
        res = _fit_from([w], full, start)
    finally:
        w.close()
    sig = np.sqrt(np.diag(twin["cov"])).reshape(twin["vel"].shape)
    off = np.max(np.abs(res.vel - twin["vel"]) / sig)
    mean_shift = np.max(np.abs(res.vel.mean(axis=1) - start.mean(axis=1)))
    print(f"device fit: {res.n_iter} iterations, decrement {res.decrement:.2e}, lnp {res.lnp_start:.6f} -> {res.lnp:.6f}; "
          f"max |v - twin| / sigma {off:.2e}; mean shift {mean_shift:.2e} km/s; sigma {np.nanmin(res.sigma):.3f} .. "
          f"{np.nanmax(res.sigma):.3f} km/s")
    assert res.converged and res.n_iter <= 20 and res.decrement <= 1e-10
    assert res.lnp >= res.lnp_start
    assert mean_shift <= 1e-12 * 60.0
    assert off <= 1e-4
    assert res.cov.shape == (12, 12) and np.all(np.isfinite(res.sigma))
    assert np.max(np.abs(res.sigma - sig)) <= 1e-4 * np.max(sig)      # (F is smooth on the scale of sigma; the tables agree to 1e-4 sigma)
    table = np.loadtxt(res.write_table(str(tmp_path / "rv.txt")))
    assert table.shape == (6, 5)
    assert np.array_equal(table[:, 0], ch.dates) and np.array_equal(table[:, 1::2].T, res.vel) and np.array_equal(table[:, 2::2].T, res.sigma)


def test_two_workers_sum_in_the_host_order_and_refusals():
    from psoap_amd import lnprob
    from psoap_amd._lib import PsoapError
    from psoap_amd.utils import registered_params
    ch = vr.fit_chunk()
    order = np.argsort(ch.lwl, kind="stable")
    blue, red = np.sort(order[:ch.N // 2]), np.sort(order[ch.N // 2:])
    full, wa = _fit_worker(ch, blue)
    _, wb = _fit_worker(ch, red)
    _, wm = _fit_worker(ch, baseline={"order": 0, "sd": [0.1]})
    p = np.array([full[n] for n in registered_params["SB2"]])
    gp = vr.fit_gp()
    try:
        vel = ch.velocities
        Fa, Fb = wa.fisher_vel_at(vel, gp), wb.fisher_vel_at(vel, gp)
        lnp_a, ga = wa.lnlike_grad_vel(vel, gp, vr.FIT_MU)
        want = wa.handle.lnlike_grad(ch.lwls[:, blue], gp, vr.FIT_MU)
        fast = vel.copy()
        fast[1, 2] = 3.0e5
        assert np.all(np.isnan(wa.fisher_vel_at(fast, gp))) and wa.lnlike_grad_vel(fast, gp)[0] == -np.inf
        for call in (lambda: wm.fisher_vel_at(vel, gp), lambda: wm.lnlike_grad_vel(vel, gp), lambda: lnprob.epoch_velocities([wa, wm], p)):
            with pytest.raises(PsoapError, match="this worker has a baseline"):
                call()
        other = _fit_worker(ch, red)[1]
        other.dates = other.dates + 1.0
        with pytest.raises(ValueError, match="share"):
            lnprob.epoch_velocities([wa, other], p)
        other.close()
        # one scoring iteration over both workers is the sum of the per-worker calls, in the order of the list
        seen = {}
        real = lnprob.velocity_scoring

        def spy(value, grad_info, vel0, seen_epochs, max_iter, tol):
            seen["start"] = np.array(vel0)
            seen["g"], seen["F"] = grad_info(np.array(vel))
            return real(value, grad_info, vel0, seen_epochs, 0, tol)

        lnprob.velocity_scoring = spy
        try:
            res = lnprob.epoch_velocities([wa, wb], p, mu_GP=vr.FIT_MU)
        finally:
            lnprob.velocity_scoring = real
    finally:
        for w in (wa, wb, wm):
            w.close()
    assert _same_bits(lnp_a, want[0]) and ga.shape == (2, 6)
    assert _same_bits(seen["F"], np.zeros_like(Fa) + Fa + Fb)
    assert res.n_iter == 0 and res.vel.shape == (2, 6)
    from psoap_amd import orbit
    assert _same_bits(seen["start"], orbit.velocities("SB2", np.array(syn.ORBIT_BASE["SB2"])[None], ch.dates)[0])      # the orbit's at p
