"""GPU: the orbit and Doppler front end -- what turns a parameter vector into the (c, N) rest-frame grids and applies the
"faster than light -> -inf" rule -- against an independent long-double reference (oracle/orbit_ext.py), over the case table
of tests/orbit_cases.py.

* ``orbit.velocities`` (k_orbit_velocities) against ``velocities_ext`` for every case of the table, all five models, within
  ``GPU_BOUND_UNITS`` of the condition unit (orbit_cases.py).
* A chain of identities carries that check into the entry points whose velocities cannot be read back:
  ``upload_orbits(P)`` == ``upload_velocities(orbit.velocities(P))`` == ``upload(grid + (-v) / c_kms)`` bit for bit, and under
  PSOAP_FIXED_PLAN=1 the resident stream's ``submit_orbits`` / ``submit_velocities`` == the batch path bit for bit -- for all
  five models and the epoch counts 1, 63, 64, 65, 257 (the dispatcher's epoch loop takes a second trip) and 3066 (the
  largest count ``psoap_stream_open`` admits for the lane count used).
* lnprob against ``oracle.lnlike`` on grids made from ``velocities_ext``: ST1 and ST2 included, and a high-e vector.
* The -inf rule through every path that finalises -- persistent launch, staged with 1, 2 and 3 stream groups, a group
  launch of two chunks, the stream -- one case per way of exceeding c, the fast proposal first, in the middle and last:
  the flagged proposal is -inf, every other one has the bits of a run with a slow proposal in its place.
* Slot hygiene: after an orbit upload that raised flags, plain and velocity uploads into the same slots (a smaller batch
  included) return no -inf and the bits of a fresh handle.

Every test prints ``ORBITROW`` JSON lines (run with -s); a second call gives the same bits everywhere."""
import json

import numpy as np
import pytest

import gpu_form_cases as fc
import orbit_cases as oc
from orbit_cases import orbit_ext
from psoap_amd import synthetic as syn

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not orbit_ext.have_ext(), reason=orbit_ext.skip_reason())]

LNP_RTOL = fc.LNP_RTOL            # 1e-10: the project's lnprob contract; not loosened here
LANES = oc.STREAM_LANES
ALL_COUNTS = oc.EPOCH_COUNTS + (oc.MAX_EPOCHS,)


def _row(**row):
    print("ORBITROW " + json.dumps(row))


def _fit(model, B, seed, high_e=True):
    """(B, n_orb) proposals (the last one at e = 0.93 on the model's last orbit), (B, 2c) GP parameters, and both side by side
    as the fitted vectors of a worker with nothing fixed"""
    c = oc.N_COMPONENTS[model]
    P = syn.make_orbit_proposals(model, B, seed=seed)
    if high_e:
        P[-1] = oc.with_params(model, base=P[-1], **{"e" + oc.ORBITS[model][-1]: 0.93})
    G = syn.make_walkers(c, B, seed=seed + 1)
    return P, G, np.hstack([P, G])


def _worker(model, ch, max_batch):
    from psoap_amd.lnprob import ChunkWorker
    return ChunkWorker(model, ch.lwl, ch.fl, ch.sigma, ch.epoch_index, ch.dates, max_batch=max_batch)


def _upload(w, fit):
    if w.model != "ST2":
        return w.upload_proposals(fit)
    n = oc.orbit_ext.N_PARAMS[w.model]
    w.upload_orbits(fit[:, :n], fit[:, n:])


def _lnprob(w, fit):
    """ChunkWorker.lnprob_batch on fitted vectors [orbit | GP] with nothing fixed.  ST2 goes through the split entry: its
    registry (utils.registered_params) holds two of the four GP parameters its two-component likelihood takes, so a
    registered ST2 vector is refused (test_registered_st2_vectors_are_refused_not_over_read)."""
    if w.model != "ST2":
        return w.lnprob_batch(fit)
    n = oc.orbit_ext.N_PARAMS[w.model]
    w.upload_orbits(fit[:, :n], fit[:, n:])
    w.handle.eval()
    return w.handle.fetch()


def _submit(w, fit):
    if w.model != "ST2":
        return w.stream_submit(fit)
    n = oc.orbit_ext.N_PARAMS[w.model]
    return w.handle.stream_submit_orbits(3, fit[:, :n], fit[:, n:])


# ---- 1. the stand-alone kernel against the long-double reference --------------------------------------------------------
@pytest.mark.parametrize("case", oc.VEL_CASES, ids=[c.name for c in oc.VEL_CASES])
def test_device_velocities_against_the_long_double_reference(case):
    from psoap_amd import orbit
    v = orbit.velocities(case.model, case.P, case.dates)
    assert v.shape == (case.P.shape[0], oc.N_COMPONENTS[case.model], len(case.dates)) and np.all(np.isfinite(v))
    worst, where, worst_abs = 0.0, None, 0.0
    for i, p in enumerate(case.P):
        ext = orbit_ext.velocities_ext(case.model, p, case.dates)
        d = oc.units_off(case.model, p, v[i], ext)
        worst_abs = max(worst_abs, float(np.max(np.abs(v[i] - ext))))
        if d >= worst:
            worst, where = d, i
    _row(test="velocities", case=case.name, model=case.model, B=int(case.P.shape[0]), n_dates=len(case.dates),
         units=round(worst, 3), bound_units=oc.GPU_BOUND_UNITS, max_abs_kms=worst_abs, proposal=where)
    assert worst <= oc.GPU_BOUND_UNITS, (case.name, where, worst)
    assert np.array_equal(orbit.velocities(case.model, case.P, case.dates), v)
    # one proposal alone (another grid shape) gives the same bits as in the batch
    assert np.array_equal(orbit.velocities(case.model, case.P[-1:], case.dates)[0], v[-1])


# ---- 2. the chain of identity on the batch path, and lnprob against the oracle ------------------------------------------
@pytest.mark.parametrize("ne", ALL_COUNTS)
@pytest.mark.parametrize("model", oc.MODELS)
def test_orbit_upload_is_velocity_upload_is_grid_upload(oracle, model, ne):
    """Same kernels, same evaluation: lnprob from upload_orbits(P), from upload_velocities(orbit.velocities(P)) and from
    upload(lwl) with lwl formed on the host agree to the last bit.  The host expression that reproduces the device's bits is
    ``grid + (-v) / c_kms`` (orbit_cases.grids_from_velocities): a negation, one IEEE division and one addition -- nothing a
    compiler may contract."""
    from psoap_amd import orbit
    c = oc.N_COMPONENTS[model]
    ch = oc.front_chunk(c, ne, seed=900 + ne % 83 + c)
    P, G, fit = _fit(model, LANES, seed=910 + c)
    w = _worker(model, ch, LANES)
    h = w.handle
    try:
        by_orbit = _lnprob(w, fit)
        v = orbit.velocities(model, P, ch.dates)
        h.upload_velocities(v, G)
        h.eval()
        by_velocity = h.fetch()
        lw = oc.grids_from_velocities(ch, v)
        h.upload(lw, G)
        h.eval()
        by_grid = h.fetch()
        again = _lnprob(w, fit)
    finally:
        w.close()
    assert np.all(np.isfinite(by_orbit)), by_orbit
    same = [bool(np.array_equal(by_orbit, by_velocity)), bool(np.array_equal(by_velocity, by_grid)),
            bool(np.array_equal(again, by_orbit))]
    row = dict(test="batch-chain", model=model, n_epochs=ne, N=ch.N, orbit_eq_velocity=same[0], velocity_eq_grid=same[1],
               second_call=same[2])
    if ne in (1, 65):
        # the value itself: the oracle on grids from the long-double velocities (rounded to double once, at the end)
        want = np.empty(LANES)
        for b in range(LANES):
            ext = orbit_ext.shift_ext(ch.lwl, orbit_ext.velocities_ext(model, P[b], ch.dates), ch.epoch_index)
            want[b] = oracle.lnlike(ext.astype(np.float64), ch.fl, ch.sigma, G[b])
        rel = float(np.max(np.abs(by_orbit - want) / np.maximum(1.0, np.abs(want))))
        row["lnp_rel_to_oracle"] = rel
    _row(**row)
    assert same == [True, True, True], (by_orbit, by_velocity, by_grid, again)
    if ne in (1, 65):
        assert rel <= LNP_RTOL, (by_orbit, want)


# ---- 3. the resident stream's own copy of the orbit code and of the shift -----------------------------------------------
@pytest.mark.parametrize("ne", ALL_COUNTS)
@pytest.mark.parametrize("model", oc.MODELS)
def test_stream_orbits_and_velocities_equal_the_batch_path_bit_for_bit(monkeypatch, model, ne):
    """PSOAP_FIXED_PLAN=1: a matrix has the task structure of a stream lane whatever the launch, so the only thing that can
    differ between the two paths is the front end -- k_orbit_velocities + k_doppler_shift there, the dispatcher's inlined copy
    (own LDS staging, own strided epoch loop: 257 epochs take a second trip, 3066 fill the staging to its limit) here."""
    from psoap_amd import orbit
    from psoap_amd._lib import PsoapError
    monkeypatch.setenv("PSOAP_FIXED_PLAN", "1")
    c = oc.N_COMPONENTS[model]
    ch = oc.front_chunk(c, ne, seed=900 + ne % 83 + c)
    P, G, fit = _fit(model, LANES, seed=910 + c)
    w = _worker(model, ch, LANES)
    h = w.handle
    refused = None
    try:
        want = _lnprob(w, fit)
        v = orbit.velocities(model, P, ch.dates)
        h.upload_velocities(v, G)
        h.eval()
        want_v = h.fetch()
        w.stream_open(LANES, 0)
        got = w.stream_fetch(_submit(w, fit))
        one = np.array([w.stream_fetch(_submit(w, fit[b:b + 1]))[0] for b in range(LANES)])
        if ne <= ch.N:
            got_v = h.stream_fetch(h.stream_submit_velocities(v, G))
        else:
            # a lane's pinned buffer holds c x N doubles: more epochs than pixels do not fit, and the library says so
            with pytest.raises(PsoapError, match="pinned buffer") as refused:
                h.stream_submit_velocities(v, G)
            got_v = want_v
        w.stream_close()
        after = _lnprob(w, fit)
    finally:
        w.close()
    same = [bool(np.array_equal(got, want)), bool(np.array_equal(got_v, want_v)), bool(np.array_equal(one, got)),
            bool(np.array_equal(want, want_v)), bool(np.array_equal(after, want))]
    _row(test="stream-chain", model=model, n_epochs=ne, N=ch.N, epoch_loop_trips=-(-ne // 256), orbits_eq_batch=same[0],
         velocities_eq_batch=same[1] if refused is None else "refused: n_epochs > N", alone_eq_together=same[2],
         orbit_eq_velocity=same[3], batch_after_close=same[4])
    assert np.all(np.isfinite(want)), want
    assert same == [True] * 5, (want, want_v, got, got_v, one, after)


# ---- 4. the -inf rule on every path that finalises ----------------------------------------------------------------------
def _check_flagged(tag, got, ref, i):
    assert np.all(np.isfinite(ref)), (tag, ref)
    assert got[i] == -np.inf, (tag, i, got)
    keep = np.arange(len(got)) != i
    assert np.array_equal(got[keep], ref[keep]), (tag, got, ref)


@pytest.mark.parametrize("case", oc.FAST_CASES, ids=[c.name for c in oc.FAST_CASES])
def test_faster_than_light_is_minus_infinity_on_every_path(case):
    B = 7                                        # staged groups of 7: [0,7) | [0,3) [3,7) | [0,2) [2,4) [4,7)
    c = oc.N_COMPONENTS[case.model]
    ne = len(case.dates)
    src = syn.make_chunk(c, ne, 600 // ne, seed=930 + c, masked_fraction=0.1)
    ch = oc.FrontChunk(c, ne, src.lwl, src.fl, src.sigma, src.epoch_index.astype(np.int32), case.dates)
    G = syn.make_walkers(c, B, seed=931)
    paths = []
    w = _worker(case.model, ch, B)
    h = w.handle
    try:
        for where in oc.FAST_POSITIONS:
            fast, slow, i = oc.fast_batch(case, B, where)
            f_fit, s_fit = np.hstack([fast, G]), np.hstack([slow, G])
            for mode, groups in (("dag", 1), ("staged", 1), ("staged", 2), ("staged", 3)):
                h.set_mode(mode)
                h.set_stream_groups(groups)
                ref = _lnprob(w, s_fit)
                got = _lnprob(w, f_fit)
                tag = "persistent" if mode == "dag" else f"staged-{groups}"
                _check_flagged((case.name, where, tag), got, ref, i)
                assert np.array_equal(_lnprob(w, f_fit), got)
                paths.append(tag)
            h.set_mode("dag")
            h.set_stream_groups(1)
            w.stream_open(B)
            ref = w.stream_fetch(_submit(w, s_fit))
            got = w.stream_fetch(_submit(w, f_fit))
            # the flagged lane, re-used at once by a slow proposal
            after = w.stream_fetch(_submit(w, s_fit))
            w.stream_close()
            _check_flagged((case.name, where, "stream"), got, ref, i)
            assert np.array_equal(after, ref)
            paths.append("stream")
    finally:
        w.close()
    _row(test="minus-inf", case=case.name, model=case.model, positions=list(oc.FAST_POSITIONS), B=B, n_epochs=ne,
         paths=sorted(set(paths)), ok=True)


@pytest.mark.parametrize("case", [c for c in oc.FAST_CASES if c.name in
                                  ("primary-K-SB2", "secondary-q-SB2", "tertiary-qout-ST3", "gamma-ST1", "v3-ST2", "one-epoch-SB1")],
                         ids=lambda c: c.name)
def test_faster_than_light_in_one_member_of_a_group_launch(case):
    """two chunks evaluated by ONE launch; only one member holds a fast proposal (each member in turn): its flagged proposal
    is -inf, everything else in both members keeps the bits of the all-slow launch"""
    from psoap_amd.chunk import ChunkGroup
    c = oc.N_COMPONENTS[case.model]
    ne = len(case.dates)
    Bs = (5, 3)
    chs = []
    for k in range(2):
        src = syn.make_chunk(c, ne, (500, 380)[k] // ne, seed=940 + k, masked_fraction=0.1)
        chs.append(oc.FrontChunk(c, ne, src.lwl, src.fl, src.sigma, src.epoch_index.astype(np.int32), case.dates))
    ws = [_worker(case.model, ch, B) for ch, B in zip(chs, Bs)]
    try:
        with ChunkGroup([w.handle for w in ws]) as g:
            def run(fits):
                for w, f in zip(ws, fits):
                    _upload(w, f)
                g.eval()
                return [w.handle.fetch() for w in ws]
            batches = [oc.fast_batch(case, B, where) for B, where in zip(Bs, ("middle", "last"))]
            Gs = [syn.make_walkers(c, B, seed=941 + k) for k, B in enumerate(Bs)]
            slow = [np.hstack([b[1], G]) for b, G in zip(batches, Gs)]
            ref = run(slow)
            for member in (0, 1):
                fits = list(slow)
                fits[member] = np.hstack([batches[member][0], Gs[member]])
                got = run(fits)
                _check_flagged((case.name, "group", member), got[member], ref[member], batches[member][2])
                assert np.array_equal(got[1 - member], ref[1 - member]), (member, got, ref)
                assert all(np.array_equal(a, b) for a, b in zip(run(fits), got))
            assert all(np.array_equal(a, b) for a, b in zip(run(slow), ref))      # the flags are gone with the fast proposal
    finally:
        for w in ws:
            w.close()
    _row(test="minus-inf", case=case.name, model=case.model, paths=["group"], members=list(Bs), n_epochs=ne, ok=True)


# ---- 5. slot hygiene ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dag", "staged"])
def test_raised_flags_do_not_outlive_their_upload(mode):
    """A handle has two proposal slots, used in turn.  Orbit uploads raise |v| >= c flags in both; the plain and the velocity
    uploads that follow -- of the same batch size and of a smaller one -- must see none of them."""
    from psoap_amd import orbit
    from psoap_amd.chunk import ChunkHandle
    case = [c for c in oc.FAST_CASES if c.name == "secondary-q-SB2"][0]
    B, small = 6, 3
    ne = len(case.dates)
    src = syn.make_chunk(2, ne, 60, seed=950, masked_fraction=0.1)
    ch = oc.FrontChunk(2, ne, src.lwl, src.fl, src.sigma, src.epoch_index.astype(np.int32), case.dates)
    G = syn.make_walkers(2, B, seed=951)
    flagged = np.repeat(case.fast[None], B, axis=0)              # every proposal fast: every flag of the slot raised
    slow = oc.fast_batch(case, B, "first")[1]
    v = orbit.velocities("SB2", slow, ch.dates)
    lw = oc.grids_from_velocities(ch, v)

    def plain(h, n):
        h.upload(lw[:n], G[:n])
        h.eval()
        return h.fetch()

    def by_velocity(h, n):
        h.upload_velocities(v[:n], G[:n])
        h.eval()
        return h.fetch()

    with ChunkHandle(ch.fl, ch.sigma, max_batch=B) as fresh:
        fresh.set_grid(ch.lwl, ch.epoch_index, ne)
        fresh.set_mode(mode)
        want = {n: plain(fresh, n) for n in (B, small)}
        assert all(np.array_equal(by_velocity(fresh, n), want[n]) for n in (B, small))
    assert all(np.all(np.isfinite(x)) for x in want.values())
    w = _worker("SB2", ch, B)
    h = w.handle
    h.set_mode(mode)
    seen = []
    try:
        for n in (B, small, B):
            for _ in range(2):                                   # both slots, one after the other
                assert np.all(np.isneginf(_lnprob(w, np.hstack([flagged, G]))))
            for k in range(4):                                   # ... and both revisited twice by the other upload forms
                got = (plain if k % 2 == 0 else by_velocity)(h, n)
                seen.append(bool(np.array_equal(got, want[n])))
                assert np.all(np.isfinite(got)), (mode, n, k, got)
                assert np.array_equal(got, want[n]), (mode, n, k, got, want[n])
            # flagged, then the other form first
            assert np.all(np.isneginf(_lnprob(w, np.hstack([flagged, G]))))
            assert np.array_equal(by_velocity(h, n), want[n]) and np.array_equal(plain(h, n), want[n])
            # a flagged upload that is never evaluated, overwritten in its pending slot
            _upload(w, np.hstack([flagged, G]))
            assert np.array_equal(plain(h, n), want[n])
        # a partly flagged orbit batch after all that: the flags are this upload's own
        fast, slow_b, i = oc.fast_batch(case, B, "middle")
        got = _lnprob(w, np.hstack([fast, G]))
        assert got[i] == -np.inf and np.all(np.isfinite(np.delete(got, i)))
    finally:
        w.close()
    _row(test="slot-hygiene", mode=mode, batch_sizes=[B, small, B], uploads_checked=len(seen), ok=all(seen))


def test_registered_st2_vectors_are_refused_not_over_read():
    """ST2 registers 14 parameters of which two are GP parameters; the library reads four per proposal.  The worker refuses
    the narrow array on both paths (it used to hand it on, and the library read past its end)."""
    ch = oc.front_chunk(2, 5, seed=960, n_target=300)
    P, G, fit = _fit("ST2", 2, seed=961)
    w = _worker("ST2", ch, 2)
    try:
        with pytest.raises(ValueError, match="expected shape"):
            w.lnprob_batch(fit[:, :14])
        with pytest.raises(ValueError, match="fitted parameters"):
            w.lnprob_batch(fit)
        w.stream_open(2)
        with pytest.raises(ValueError, match="expected shape"):
            w.stream_submit(fit[:, :14])
        w.stream_close()
        got = _lnprob(w, fit)
        assert np.all(np.isfinite(got)) and np.array_equal(_lnprob(w, fit), got)
    finally:
        w.close()
    _row(test="st2-registry", refused=True, ok=True)
