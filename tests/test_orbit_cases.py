"""CPU: the references and the case table behind tests/test_gpu_orbit_front.py.

* oracle/orbit_ext.py (bisection, atan2, long double) against oracle/orbit_oracle.py (Newton, tan, double) over the whole
  table, in units of the condition of the map; the measured maximum is the constant the GPU bound is 4x of;
* both against the modelled project's own velocities (golden_orbit_v1.npz) within 1e-8 km/s;
* the table covers what it claims: the eccentricity ladder, the phase edges, the epoch counts;
* the margins of the faster-than-light cases;
* every seeded defect of a restated kernel is rejected by the table at the GPU tolerance."""
import os
import sys

import numpy as np
import pytest

import orbit_cases as oc
from orbit_cases import orbit_ext
from psoap_amd import synthetic as syn

sys.path.insert(0, os.path.join(oc.ROOT, "oracle"))
import orbit_oracle  # noqa: E402

VEL_ATOL = 1e-8       # km/s: against the modelled project's own output (its Kepler solve: fsolve, xtol 1.5e-8)

needs_ext = pytest.mark.skipif(not orbit_ext.have_ext(), reason=orbit_ext.skip_reason())


@pytest.fixture(scope="module")
def ext_table():
    """velocities_ext of every proposal of every case: {case name: [(c, n_dates) long double, ...]}"""
    return {case.name: [orbit_ext.velocities_ext(case.model, p, case.dates) for p in case.P] for case in oc.VEL_CASES}


@needs_ext
def test_fp64_oracle_agrees_with_ext(ext_table):
    """The measurement behind the tolerance: max |orbit_oracle - ext| / u over the table.  The committed constant must cover
    it and must not be slack (within a factor two of what is measured), so the GPU bound stays 4x a measured figure."""
    worst, where = 0.0, None
    per_tag = {}
    for case in oc.VEL_CASES:
        for i, p in enumerate(case.P):
            d = oc.units_off(case.model, p, orbit_oracle.velocities(case.model, p, case.dates), ext_table[case.name][i])
            per_tag[case.tags[0]] = max(per_tag.get(case.tags[0], 0.0), d)
            if d > worst:
                worst, where = d, (case.name, i)
    print(f"ORBITCPU max |oracle - ext| / u = {worst:.3f} at {where}; per group {per_tag}")
    assert worst <= oc.CPU_ORACLE_MAX_UNITS, (worst, where)
    assert worst >= 0.5 * oc.CPU_ORACLE_MAX_UNITS, "the committed constant is slack: re-measure it"
    assert oc.GPU_BOUND_UNITS == 4.0 * oc.CPU_ORACLE_MAX_UNITS


@needs_ext
def test_both_references_match_the_modelled_projects_velocities():
    gorb = dict(np.load(os.path.join(oc.ROOT, "tests", "golden", "golden_orbit_v1.npz")))
    dates = gorb["dates"]
    for model in oc.MODELS:
        P = syn.make_orbit_proposals(model, 6, seed=500)
        for i, p in enumerate(P):
            ext = orbit_ext.velocities_ext(model, p, dates)
            assert ext.dtype == np.longdouble and ext.shape == (oc.N_COMPONENTS[model], len(dates))
            np.testing.assert_allclose(ext.astype(np.float64), gorb[f"vel_{model}"][i], rtol=0, atol=VEL_ATOL)
            np.testing.assert_allclose(orbit_oracle.velocities(model, p, dates), gorb[f"vel_{model}"][i], rtol=0, atol=VEL_ATOL)
    ext = orbit_ext.velocities_ext("SB2", gorb["p_SB2_ecc"], dates)
    np.testing.assert_allclose(ext.astype(np.float64), gorb["vel_SB2_ecc"], rtol=0, atol=VEL_ATOL)


@needs_ext
def test_ext_solves_keplers_equation_and_shifts():
    """the reference against its own definition: the residual of Kepler's equation at long-double level, the closed forms at
    e = 0 and at M = pi, and the Doppler step against synthetic.replicate_wls"""
    M = np.linspace(0, 2 * np.pi, 41).astype(np.longdouble)
    for e in oc.E_LADDER:
        E = orbit_ext.eccentric_anomaly(M, e)
        assert np.max(np.abs(E - np.longdouble(e) * np.sin(E) - M)) <= 16 * np.finfo(np.longdouble).eps
    # e = 0: f = M, so v = K cos(w + M) + gamma
    dates = np.array([0.0, 1.25, 2.5, 7.0, -1.0])
    v = orbit_ext.velocities_ext("SB1", (10.0, 0.0, 30.0, 5.0, 0.0, 2.0), dates)[0]
    want = 10 * np.cos(orbit_ext.PI / 6 + orbit_ext.TWO_PI * np.array([0, 1.25, 2.5, 2.0, 4.0], dtype=np.longdouble) / 5) + 2
    assert np.max(np.abs(v - want)) <= 1e-17
    # M = pi: E = f = pi whatever e, so v = K (-cos w + e cos w) + gamma
    v = orbit_ext.velocities_ext("SB1", (10.0, 0.875, 0.0, 5.0, 0.0, 0.0), np.array([2.5]))[0, 0]
    assert abs(v - (-1.25)) <= 1e-17
    ch = syn.make_chunk(2, 4, 30, seed=5, masked_fraction=0.2)
    got = orbit_ext.shift_ext(ch.lwl, ch.velocities, ch.epoch_index)
    assert got.dtype == np.longdouble
    assert np.max(np.abs(got.astype(np.float64) - syn.replicate_wls(ch.lwl, ch.velocities, ch.mask))) <= 2e-15


def test_the_table_covers_what_it_claims():
    names = [c.name for c in oc.VEL_CASES]
    assert len(set(names)) == len(names)
    for model in oc.MODELS:
        mine = [c for c in oc.VEL_CASES if c.model == model]
        assert {t for c in mine for t in c.tags} == {"ecc", "phase", "roles", "epochs"}
        # the ladder on every orbit of the model
        for orb in oc.ORBITS[model]:
            j = oc.NAMES[model].index("e" + orb)
            ladder = [c for c in mine if c.name == f"ecc-{model}{orb}"][0]
            assert tuple(ladder.P[:, j]) == oc.E_LADDER
        assert {len(c.dates) for c in mine if "epochs" in c.tags} == set(oc.EPOCH_COUNTS) | {oc.MAX_EPOCHS}
        # omega in all four quadrants and above 180; q from 0.05 to 1
        roles = [c for c in mine if "roles" in c.tags][0]
        om = roles.P[:, oc.NAMES[model].index("omega" + oc.ORBITS[model][0])]
        assert {int(w // 90) % 4 for w in om} == {0, 1, 2, 3} and om.max() > 180
        if oc.NAMES[model][0].startswith("q"):
            assert roles.P[:, 0].min() == 0.05 and roles.P[:, 0].max() == 1.0
    assert oc.E_LADDER[4] < 0.8 and np.nextafter(oc.E_LADDER[4], 1.0) == 0.8
    # ST3's two orbits share no parameter value: a swap of roles cannot be silent
    b = oc.with_params("ST3")
    for n in ("q", "K", "e", "omega", "P", "T0"):
        assert b[oc.NAMES["ST3"].index(n + "_in")] != b[oc.NAMES["ST3"].index(n + "_out")]
    # the phase edges are what their builder says, in the arithmetic both sides share: tt = mod(fl(t - T0), P)
    periods = set()
    for per, T0 in ((0.5, 0.0), (23.0, 0.0), (2000.0, 2455010.0), (23.0, 2455010.0)):
        periods.add(per)
        d = oc._edge_dates(per, T0)
        tt = orbit_ext.phase(d, T0, per)
        assert d[0] == T0 and np.sum(tt == 0.0) >= 5 and np.sum(tt == 0.5 * per) >= 3 and np.sum(d < T0) >= 5
        assert np.all((tt >= 0.0) & (tt <= per))
        if T0 == 0.0:
            ph = tt / per
            assert np.any((ph > 0) & (ph < 1e-12)) and np.any((ph < 1) & (ph > 1 - 1e-12)) and np.max(d / per) > 1000
            assert np.max(d) > 2.4e6
    assert min(periods) == 0.5 and max(periods) == 2000.0
    # the LDS bound of psoap_stream_open, restated: the largest count fits, one more does not
    for lanes in (1, oc.STREAM_LANES, 64):
        ne = oc.max_stream_epochs(lanes)
        assert (3 * ne + 16) * 8 + 4 * lanes <= 73728 < (3 * (ne + 1) + 16) * 8 + 4 * lanes
    assert oc.MAX_EPOCHS == 3066


@pytest.mark.parametrize("ne", oc.EPOCH_COUNTS + (oc.MAX_EPOCHS,))
def test_front_chunks_are_small_ragged_and_not_monotone(ne):
    fc = oc.front_chunk(2, ne, seed=800 + ne % 89)
    assert fc.dates.shape == (ne,) and fc.epoch_index.shape == (fc.N,) and 800 <= fc.N <= 1300
    assert fc.epoch_index.min() >= 0 and fc.epoch_index.max() < ne
    if ne > 1:
        counts = np.bincount(fc.epoch_index, minlength=ne)
        assert len(set(counts)) > 1 and np.any(np.diff(fc.epoch_index) < 0) and np.any(np.diff(fc.dates) < 0)
    vel = np.arange(2 * ne, dtype=np.float64).reshape(2, ne)
    g = oc.grids_from_velocities(fc, vel)
    assert g.shape == (2, fc.N) and g[1, 0] == fc.lwl[0] + (-vel[1, fc.epoch_index[0]]) / oc.C_KMS


@needs_ext
@pytest.mark.parametrize("case", oc.FAST_CASES, ids=[c.name for c in oc.FAST_CASES])
def test_margins_of_the_faster_than_light_cases(case):
    """no case sits on the boundary: by the long-double reference the fast proposal has |v| >= 1.001 c in exactly the named
    components (and, where the case says so, in exactly that many epochs) and |v| <= 0.999 c everywhere else; the slow
    replacement and every row of the batches built around it stay <= 0.999 c"""
    c_fast, c_slow = oc.FAST_MARGIN * oc.C_KMS, oc.SLOW_MARGIN * oc.C_KMS
    v = np.abs(orbit_ext.velocities_ext(case.model, case.fast, case.dates))
    for k in range(v.shape[0]):
        if k in case.fast_components:
            assert v[k].max() >= c_fast, (k, float(v[k].max()))
            assert np.all((v[k] >= c_fast) | (v[k] <= c_slow)), "an epoch sits on the boundary"
        else:
            assert v[k].max() <= c_slow, (k, float(v[k].max()))
    if case.fast_epochs:
        assert int(np.sum(np.any(v >= c_fast, axis=0))) == case.fast_epochs and len(case.dates) >= 10
    assert np.abs(orbit_ext.velocities_ext(case.model, case.slow, case.dates)).max() <= c_slow
    for where in oc.FAST_POSITIONS:
        fast, slow, i = oc.fast_batch(case, 7, where)
        assert np.array_equal(fast[i], case.fast) and np.array_equal(np.delete(fast, i, 0), np.delete(slow, i, 0))
        for p in slow:
            assert np.abs(orbit_ext.velocities_ext(case.model, p, case.dates)).max() <= c_slow
    assert {"first", "middle", "last"} == set(oc.FAST_POSITIONS)


def test_every_way_of_exceeding_c_has_a_case():
    kinds = {c.name.rsplit("-", 1)[0] for c in oc.FAST_CASES}
    assert kinds == {"primary-K", "secondary-q", "tertiary-qout", "gamma", "v3", "one-epoch"}


# ---- sensitivity --------------------------------------------------------------------------------------------------------
@needs_ext
def test_the_restated_kernel_passes_the_table(ext_table):
    """the restatement without a defect is inside the GPU bound (or the test below proves nothing)"""
    for case in oc.VEL_CASES:
        for i, p in enumerate(case.P):
            d = oc.units_off(case.model, p, oc.kernel_restated(case.model, p, case.dates), ext_table[case.name][i])
            assert d <= oc.GPU_BOUND_UNITS, (case.name, i, d)


@needs_ext
@pytest.mark.parametrize("defect", oc.DEFECTS)
def test_a_seeded_defect_is_rejected_by_the_table(ext_table, defect):
    """one defect at a time in the restated orbit_velocities_at: at least one case of the table is off by more than the
    bound the GPU test asserts"""
    caught = []
    for case in oc.VEL_CASES:
        worst = max(oc.units_off(case.model, p, oc.kernel_restated(case.model, p, case.dates, defect), ext_table[case.name][i])
                    for i, p in enumerate(case.P))
        if not worst <= oc.GPU_BOUND_UNITS:           # (a NaN is caught too)
            caught.append((case.name, worst))
    print(f"ORBITDEFECT {defect}: rejected by {len(caught)} of {len(oc.VEL_CASES)} cases, e.g. "
          f"{[(n, f'{w:.3g} u') for n, w in caught[:3]]}")
    assert caught, defect
