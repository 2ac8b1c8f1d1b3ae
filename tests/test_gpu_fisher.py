"""GPU tests of the Fisher information of the likelihood (psoap_chunk_fisher, psoap_amd/csrc/fisher_kernels.hpp).

Shapes at the edges of the 128-row tiles (tests/fisher_reference.py: CASES), masked chunks with unequal epochs, the benchmark
hyper-parameters; per case the 2c hyper-parameter unit tangents, two velocity tangents and one random grid tangent.  The
device's F against the long-double reference, every entry, relative to sqrt(F_ss F_tt) (F is positive semi-definite: that
bounds |F_st|); F_mu relative to itself.

The tolerance is derived, not fitted: the float64 SciPy evaluation of the same formulas (cho_factor / cho_solve,
fisher_reference.fisher_f64) measured against the long-double one on these very cases (python tests/fisher_reference.py):

    case                F       F_mu
    N100-c2      8.46e-15   7.78e-17
    N128-c2      4.69e-14   7.52e-17
    N129-c2      1.28e-14   3.26e-16
    N300-c1      5.07e-14   2.51e-16
    N300-c2      2.53e-14   2.85e-16
    N300-c3      1.61e-14   2.29e-16
    max          5.07e-14   3.26e-16

The device sums in another order and fuses multiply-adds but is fp64 throughout: it gets the largest measured value of each
output times the project's margin of 8 (tests/test_gpu_grad.py):

    F  8 x 5.07e-14 = 4.06e-13      F_mu  8 x 3.26e-16 = 2.61e-15
"""
import numpy as np
import pytest

import fisher_reference as fr
from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu

MARGIN = 8
F64_REL = {"F": 5.07e-14, "mu": 3.26e-16}        # the table above, last row
TOL = {k: MARGIN * v for k, v in F64_REL.items()}
_LD = np.longdouble


def _handle(ch, **kw):
    from psoap_amd.chunk import ChunkHandle
    return ChunkHandle(ch.fl, ch.sigma, **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).copy()


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("case", fr.CASES, ids=fr.case_id)
def test_fisher_against_long_double(case):
    ch, gp = fr.case_chunk(case), fr.case_gp(case)
    tan_lwl, tan_gp = fr.case_tangents(case)
    F_ref, mu_ref = fr.case_ext(case)
    with _handle(ch) as h:
        F, F_mu = h.fisher(ch.lwls, gp, tan_gp, tan_lwl, want_mu=True)
    err = {"F": fr.rel_to_scale(F, F_ref), "mu": float(abs(_LD(F_mu) - mu_ref) / mu_ref)}
    print(f"{fr.case_id(case)}: " + ", ".join(f"{k} {v:.2e} (bound {TOL[k]:.2e})" for k, v in err.items()))
    assert F.shape == (tan_gp.shape[0],) * 2 and np.all(np.isfinite(F))
    assert _same_bits(F, F.T)
    for k in ("F", "mu"):
        assert err[k] <= TOL[k], (k, err[k], TOL[k])


def test_one_tangent_null_grid_tangents_null_mu():
    """T = 1, tan_lwl = NULL and fisher_mu = NULL: the hyper-parameter block against the long-double reference, and the bits
    of the same tangents passed with explicit zeros"""
    case = fr.CASES[2]                        # N = 129: two tile rows
    ch, gp, c = fr.case_chunk(case), fr.case_gp(case), case[1]
    tan_lwl, tan_gp = fr.case_tangents(case)
    F_ref, _ = fr.case_ext(case)
    with _handle(ch) as h:
        one = h.fisher(ch.lwls, gp, tan_gp[1:2])
        hyper = h.fisher(ch.lwls, gp, tan_gp[:2 * c])
        zeros = h.fisher(ch.lwls, gp, tan_gp[:2 * c], np.zeros((2 * c, c, ch.N)))
        grid_one = h.fisher(ch.lwls, gp, tan_gp[2 * c:2 * c + 1], tan_lwl[2 * c:2 * c + 1])
    assert one.shape == (1, 1) and hyper.shape == (2 * c, 2 * c)
    assert _same_bits(hyper, zeros) and _same_bits(one[0, 0], hyper[1, 1])
    err = fr.rel_to_scale(hyper, F_ref[:2 * c, :2 * c])
    err_one = float(abs(_LD(grid_one[0, 0]) - F_ref[2 * c, 2 * c]) / F_ref[2 * c, 2 * c])
    print(f"hyper-parameter block {err:.2e}, one velocity tangent {err_one:.2e} (bound {TOL['F']:.2e})")
    assert err <= TOL["F"] and err_one <= TOL["F"]


def test_bits_repeat_and_a_subsequence_of_the_tangents_shares_them():
    case = fr.CASES[4]                        # N = 300, c = 2: three tile rows, T = 7
    ch, gp = fr.case_chunk(case), fr.case_gp(case)
    tan_lwl, tan_gp = fr.case_tangents(case)
    pick = [1, 4]
    with _handle(ch) as h:
        six, mu = h.fisher(ch.lwls, gp, tan_gp[:6], tan_lwl[:6], want_mu=True)
        again, mu2 = h.fisher(ch.lwls, gp, tan_gp[:6], tan_lwl[:6], want_mu=True)
        two = h.fisher(ch.lwls, gp, tan_gp[pick], tan_lwl[pick])
    assert _same_bits(six, again) and _same_bits(mu, mu2)
    assert _same_bits(six, six.T) and _same_bits(two, two.T)
    assert _same_bits(two, six[np.ix_(pick, pick)])
    assert len({float(v) for v in six[np.triu_indices(6)]}) == 21


def test_conventions_negative_amplitude_not_positive_definite_bad_T_open_stream_release():
    from psoap_amd._lib import PsoapError
    from psoap_amd.chunk import ChunkHandle
    case = fr.CASES[0]
    ch, gp, c = fr.case_chunk(case), fr.case_gp(case), case[1]
    tan_lwl, tan_gp = fr.case_tangents(case)
    T = tan_gp.shape[0]
    with _handle(ch) as h:
        good = h.fisher(ch.lwls, gp, tan_gp, tan_lwl)
        neg = gp.copy()
        neg[0] = -neg[0]
        F, mu = h.fisher(ch.lwls, neg, tan_gp, tan_lwl, want_mu=True)         # status 0: no exception
        assert F.shape == (T, T) and np.all(np.isnan(F)) and np.isnan(mu)
        with pytest.raises(PsoapError, match="tangents"):
            h.fisher(ch.lwls, gp, np.zeros((0, 2 * c)))
        with pytest.raises(PsoapError, match="tangents"):
            h.fisher(ch.lwls, gp, np.zeros((33, 2 * c)))
        assert h.fisher(ch.lwls, gp, np.tile(tan_gp[:1], (32, 1))).shape == (32, 32)
        h.stream_open(c, 1)
        try:
            with pytest.raises(PsoapError, match="open stream"):
                h.fisher(ch.lwls, gp, tan_gp, tan_lwl)
        finally:
            h.stream_close()
        # release, twice, then another call: the workspace comes back, and so do the bits
        h.fisher_release()
        h.fisher_release()
        assert _same_bits(h.fisher(ch.lwls, gp, tan_gp, tan_lwl), good)
    # not positive definite: zero noise and two identical pixels
    lw = ch.lwls.copy()
    lw[:, 1] = lw[:, 0]
    with ChunkHandle(ch.fl, np.zeros_like(ch.sigma)) as h:
        F, mu = h.fisher(lw, gp, tan_gp, tan_lwl, want_mu=True)
    assert np.all(np.isnan(F)) and np.isnan(mu)


def test_fisher_leaves_the_handle_as_it_was():
    """an evaluation before and after a Fisher call on the same handle: identical bits, and an uploaded batch survives"""
    case = fr.CASES[4]
    ch, gp = fr.case_chunk(case), fr.case_gp(case)
    tan_lwl, tan_gp = fr.case_tangents(case)
    gps = syn.make_walkers(ch.n_components, 4, seed=7800)
    lw = syn.walker_lwls(ch, syn.make_walker_velocities(ch, 4, seed=7801))
    with _handle(ch, max_batch=4) as h:
        one_before = h.lnlike(ch.lwls, gp, 0.9)
        before = h.lnlike_batch(lw, gps, 0.9)
        h.upload(lw[::-1].copy(), gps[::-1].copy(), 0.9)
        h.fisher(ch.lwls, gp, tan_gp, tan_lwl)
        h.eval()
        pending = h.fetch()
        after = h.lnlike_batch(lw, gps, 0.9)
        one_after = h.lnlike(ch.lwls, gp, 0.9)
    assert _same_bits(before, after) and _same_bits(pending, before[::-1]) and _same_bits(one_before, one_after)


# ---- lnprob(p): tangents through the orbit Jacobian ---------------------------------------------------------------------
def _sb2_worker(seed_case, fix=("gamma",)):
    from psoap_amd.lnprob import ChunkWorker
    from psoap_amd.utils import registered_params
    ch = fr.case_chunk(seed_case)
    full = dict(zip(registered_params["SB2"], list(syn.ORBIT_BASE["SB2"]) + list(syn.GP_BASE[2])))
    return ch, full, ChunkWorker("SB2", ch.lwl, ch.fl, ch.sigma, ch.epoch_index, ch.dates, fix_params=list(fix), defaults=full)


def test_worker_fisher_against_long_double_composed_with_the_long_double_jacobian():
    """SB2 with gamma fixed (it moves every grid alike: the data do not constrain it), N = 129, 5 epochs.  The reference:
    fisher_ext on the grids the worker uses (the device's velocities, shifted as the device shifts them) with the tangents
    dx_i = -J[c, epoch, i] / c_kms of the LONG-DOUBLE Jacobian (tests/orbit_grad_reference.py), at the tolerance above."""
    import orbit_grad_reference as ogr
    from psoap_amd import orbit
    from psoap_amd.utils import registered_params
    case = fr.CASES[2]
    assert case[0] == 129 and case[2] == 5
    ch, full, w = _sb2_worker(case)
    try:
        names = [n for n in registered_params["SB2"] if n != "gamma"]
        p = np.array([full[n] for n in names])
        F = w.fisher(p)
        lnp, grad = w.lnprob_grad(p)
    finally:
        w.close()
    assert F.shape == (len(names),) * 2 == (grad.shape[0],) * 2 and _same_bits(F, F.T)
    p_orb, gp = np.array(syn.ORBIT_BASE["SB2"]), np.array(syn.GP_BASE[2])
    vel = orbit.velocities("SB2", p_orb[None], ch.dates)[0]
    ep = ch.epoch_index
    lwls = ch.lwl[None, :] + (-vel[:, ep]) / fr.C_KMS
    J, _ = ogr.jacobian_ext("SB2", p_orb, ch.dates)
    n_orb = p_orb.shape[0]
    keep = [i for i in range(n_orb) if registered_params["SB2"][i] != "gamma"]
    tan_lwl = [-np.moveaxis(J, 2, 0)[i][:, ep] / _LD(fr.C_KMS) for i in keep] + [np.zeros((2, ch.N), dtype=_LD)] * 4
    tan_gp = np.zeros((len(keep) + 4, 4))
    tan_gp[len(keep):] = np.eye(4)
    F_ref, _ = fr.fisher_ext(lwls, ch.sigma, gp, tan_lwl, tan_gp)
    err = fr.rel_to_scale(F, F_ref)
    print(f"SB2-N129 worker Fisher, {len(names)} parameters: error {err:.2e} (bound {TOL['F']:.2e})")
    assert err <= TOL["F"]


def test_laplace_covariance_over_two_workers_and_fisher_jumps_as_opt_jump(tmp_path):
    from psoap_amd import lnprob, sample_parallel
    from psoap_amd.utils import registered_params
    made = [_sb2_worker(case) for case in (fr.CASES[2], fr.CASES[0])]
    workers, full = [m[2] for m in made], made[0][1]
    names = [n for n in registered_params["SB2"] if n != "gamma"]
    p = np.array([full[n] for n in names])
    fname = str(tmp_path / "opt_jump.npy")
    try:
        F_sum = lnprob.fisher_information(workers, p)
        assert _same_bits(F_sum, workers[0].fisher(p) + workers[1].fisher(p))
        C = lnprob.laplace_covariance(workers, p)
        jumps = lnprob.fisher_jumps(workers, p, fname)
        with pytest.raises(np.linalg.LinAlgError):
            lnprob.laplace_covariance(workers, p, prior_precision=-2.0 * F_sum)
    finally:
        for w in workers:
            w.close()
    d = len(names)
    cond = np.linalg.cond(F_sum)
    dev = np.max(np.abs(C @ F_sum - np.eye(d)))
    print(f"cond(F_sum) = {cond:.3e}, max |C F - I| = {dev:.3e} (bound {1e-8 * cond:.3e})")
    assert dev <= 1e-8 * cond
    assert _same_bits(jumps, 2.38 ** 2 / d * C)
    config = {"opt_jump": fname, "fix_params": ["gamma"], "jumps": {n: 1.0 for n in names}}
    assert _same_bits(sample_parallel.proposal_covariance(config, "SB2", d), jumps)


def test_covariance_fisher_information_is_the_hyper_parameter_block():
    from psoap_amd import covariance
    case = fr.CASES[0]
    ch, gp, c = fr.case_chunk(case), fr.case_gp(case), case[1]
    F_ref, _ = fr.case_ext(case)
    try:
        F = covariance.fisher_information(ch.lwls, ch.fl, ch.sigma, gp)
        cached = list(covariance._handles.values())
        again = covariance.fisher_information(ch.lwls, ch.fl, ch.sigma, gp)      # the cached handle, no new one
        assert [id(h) for h in covariance._handles.values()] == [id(h) for h in cached]
        bad = covariance.fisher_information(ch.lwls, ch.fl, ch.sigma, [-0.2, 5.0, 0.1, 7.0])
    finally:
        covariance.release_handles()
    assert F.shape == (2 * c, 2 * c) and _same_bits(F, again) and np.all(np.isnan(bad))
    assert fr.rel_to_scale(F, F_ref[:2 * c, :2 * c]) <= TOL["F"]
