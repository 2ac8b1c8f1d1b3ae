"""The skyline on the device: the throughput scheme of a batch evaluated over the tiles that are not provably zero, against
the CPU oracle and against a handle created under PSOAP_SKYLINE=0 (input order, dense list)."""
import numpy as np
import pytest

from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu

B = 16
N = 1250


def lnp_close(got, want):
    return abs(got - want) <= 1e-10 * max(1.0, abs(want))


@pytest.fixture(autouse=True)
def scheme0(monkeypatch):
    monkeypatch.setenv("PSOAP_DAG_SCHEME", "0")
    monkeypatch.delenv("PSOAP_SKYLINE", raising=False)


def chunk(c, seed, n=N):
    ch = syn.make_chunk(c, 4, 320, seed=seed)
    keep = np.arange(ch.N)[:n]
    gps = syn.make_walkers(c, B, seed=seed + 1)
    lwl = syn.walker_lwls(ch, syn.make_walker_velocities(ch, B, seed=seed + 2))[:, :, keep]
    return ch.fl[keep], ch.sigma[keep], np.ascontiguousarray(lwl), gps


def run(fl, sigma, lwl, gps, monkeypatch, oracle=None, twice=True):
    """lnprob of the batch with the skyline, twice on one handle, and from a dense handle; the handle's stats."""
    from psoap_amd.chunk import ChunkHandle
    with ChunkHandle(fl, sigma, max_batch=B) as h:
        got = h.lnlike_batch(lwl, gps)
        stats = h.sky_stats()
        if twice:
            assert np.array_equal(h.lnlike_batch(lwl, gps), got, equal_nan=True)
    monkeypatch.setenv("PSOAP_SKYLINE", "0")
    with ChunkHandle(fl, sigma, max_batch=B) as h:
        dense = h.lnlike_batch(lwl, gps)
        dstats = h.sky_stats()
    monkeypatch.delenv("PSOAP_SKYLINE")
    assert stats["skyline_on"] == 1 and dstats["skyline_on"] == 0 and dstats["tiles_planned"] == dstats["tiles_dense"]
    for b in range(len(got)):
        if np.isfinite(dense[b]):
            assert lnp_close(got[b], dense[b]), (b, got[b], dense[b])
        else:
            assert got[b] == dense[b] or (np.isnan(got[b]) and np.isnan(dense[b])), (b, got[b], dense[b])
        if oracle is not None and np.isfinite(dense[b]):
            want = oracle.lnlike(lwl[b], fl, sigma, list(gps[b]))
            assert lnp_close(got[b], want), (b, got[b], want)
    return got, dense, stats


def test_a_epoch_major_input_has_a_proper_skyline(oracle, monkeypatch):
    fl, sigma, lwl, gps = chunk(2, 300)
    _, _, st = run(fl, sigma, lwl, gps, monkeypatch, oracle)
    assert st["tiles_dense"] == B * 10 * 11 // 2 and st["tiles_planned"] < st["tiles_dense"]
    assert st["units_planned"] < st["units_dense"]


def test_b_one_wide_walker_makes_the_union_dense(oracle, monkeypatch):
    fl, sigma, lwl, gps = chunk(2, 300)
    gps = gps.copy()
    gps[5, 1] = 60.0
    _, _, st = run(fl, sigma, lwl, gps, monkeypatch, oracle)
    # (l = 60 km/s: support 38.6 l / c = 7.7e-3 in ln-wavelength, the chunk spans 320 px of ~1 km/s: 1e-3)
    assert st["tiles_planned"] == st["tiles_dense"] and st["units_planned"] == st["units_dense"]


def test_c_two_separated_ranges_exercise_the_clamp(oracle, monkeypatch):
    fl, sigma, lwl, gps = chunk(2, 301, n=1024)
    lwl = lwl.copy()
    lwl[:, :, 512:] += 1.0
    _, _, st = run(fl, sigma, lwl, gps, monkeypatch, oracle)
    # block-diagonal, 4 + 4 tiles: at most the two triangles and the clamp's tile (3, 4) -- fewer where a block is a band itself
    assert st["tiles_planned"] <= B * (10 + 10 + 1)


def test_d_exact_ties_in_the_sort_key_are_deterministic(oracle, monkeypatch):
    ch = syn.make_chunk(2, 4, 320, seed=302)
    keep = np.arange(ch.N)[:N]
    gps = syn.make_walkers(2, B, seed=303)
    # no jitter, equal velocities in all epochs: every epoch's grid is the same -- four-fold ties
    grid = np.tile(ch.lwl[:320], 4)[keep]
    vel = np.tile(np.array([[3.0], [-2.0]]), (B, 1, 4))
    lwl = np.stack([np.stack([grid - v[c, 0] / syn.C_KMS for c in range(2)]) for v in vel])
    fl, sigma = ch.fl[keep], np.maximum(ch.sigma[keep], 0.02)
    a, _, _ = run(fl, sigma, lwl, gps, monkeypatch, oracle)
    b, _, _ = run(fl, sigma, lwl, gps, monkeypatch, None, twice=False)
    assert np.array_equal(a, b)


def test_e_negative_amplitude_and_a_singular_matrix(oracle, monkeypatch):
    fl, sigma, lwl, gps = chunk(2, 304)
    gps = gps.copy()
    gps[3, 0] = -0.2
    got, dense, _ = run(fl, sigma, lwl, gps, monkeypatch, oracle)
    assert got[3] == -np.inf and np.isfinite(np.delete(got, 3)).all()
    # sigma = 0 and duplicated rows: not positive definite, for every walker
    lw2 = lwl.copy()
    lw2[:, :, 700:710] = lw2[:, :, 690:700]
    got, dense, _ = run(fl, np.zeros_like(sigma), lw2, gps, monkeypatch, None)
    assert np.array_equal(np.isneginf(got), np.isneginf(dense)) and np.isneginf(got[3])


@pytest.mark.parametrize("c", [1, 3])
def test_f_one_and_three_components(oracle, monkeypatch, c):
    fl, sigma, lwl, gps = chunk(c, 305 + c)
    _, _, st = run(fl, sigma, lwl, gps, monkeypatch, oracle, twice=False)
    assert st["tiles_planned"] < st["tiles_dense"]


def check(got, lwl, fl, sigma, gps, oracle, dense):
    """`got` against the oracle and against the values of a PSOAP_SKYLINE=0 handle, at the contract"""
    for b in range(len(got)):
        assert lnp_close(got[b], oracle.lnlike(lwl[b], fl, sigma, list(gps[b]))), (b, got[b])
        assert lnp_close(got[b], dense[b]), (b, got[b], dense[b])


def dense_values(fl, sigma, lwl, gps, monkeypatch):
    from psoap_amd.chunk import ChunkHandle
    monkeypatch.setenv("PSOAP_SKYLINE", "0")
    with ChunkHandle(fl, sigma, max_batch=B) as h:
        out = h.lnlike_batch(lwl, gps)
        assert h.sky_stats()["skyline_on"] == 0
    monkeypatch.delenv("PSOAP_SKYLINE")
    return out


def test_g_upload_paths_slots_and_the_plan_cache(oracle, monkeypatch):
    from psoap_amd.chunk import ChunkHandle
    ch = syn.make_chunk(2, 4, 320, seed=310)
    gps = syn.make_walkers(2, B, seed=311)
    vel = syn.make_walker_velocities(ch, B, seed=312)
    lwl = syn.walker_lwls(ch, vel)
    lwl_r, gps_r = np.roll(lwl, 1, axis=0), np.roll(gps, 1, axis=0)
    with ChunkHandle(ch.fl, ch.sigma, max_batch=B) as h:
        h.set_grid(ch.lwl, ch.epoch_index, ch.n_epochs)
        h.upload(lwl, gps)
        h.eval()
        first = h.fetch()
        s1 = h.sky_stats()
        h.upload_velocities(vel, gps)                                   # the other slot, the device-side Doppler shift
        h.eval()
        second = h.fetch()
        h.upload(lwl_r, gps_r)                                          # walkers rolled by one, back in the first slot
        h.eval()
        third = h.fetch()
        s3 = h.sky_stats()
    dense = dense_values(ch.fl, ch.sigma, lwl, gps, monkeypatch)
    check(first, lwl, ch.fl, ch.sigma, gps, oracle, dense)
    check(second, lwl, ch.fl, ch.sigma, gps, oracle, dense)
    check(third, lwl_r, ch.fl, ch.sigma, gps_r, oracle, np.roll(dense, 1))
    assert np.array_equal(first, second)
    assert s1["tiles_planned"] < s1["tiles_dense"] and s1["plan_builds"] == 1
    assert s3["plan_builds"] == 1 and s3["cache_hits"] == s1["cache_hits"] + 2
    with ChunkHandle(ch.fl, ch.sigma, max_batch=B) as fresh:
        assert np.array_equal(fresh.lnlike_batch(lwl_r, gps_r), third)


def test_h_the_plan_cache_returns_to_an_earlier_skyline(oracle, monkeypatch):
    """Two proposal sets with different envelopes in turn on one handle: two builds, every later change a cache hit, and
    more envelopes than the cache holds evict the oldest -- the values right throughout."""
    from psoap_amd.chunk import ChunkHandle
    fl, sigma, lwl, gps = chunk(2, 320)
    from test_sky_plan import sky_first
    sets, seen = [], set()
    for scale in np.arange(0.3, 4.0, 0.1):        # wider kernels: wider envelopes -- the first five that differ and are proper
        g = gps.copy()
        g[:, 1::2] *= scale
        env = tuple(sky_first(lwl, g)[0])
        if any(env) and env not in seen and len(sets) < 5:
            seen.add(env)
            sets.append((g, dense_values(fl, sigma, lwl, g, monkeypatch)))
    assert len(sets) == 5
    with ChunkHandle(fl, sigma, max_batch=B) as h:
        planned = []
        for g, dense in sets[:2]:
            check(h.lnlike_batch(lwl, g), lwl, fl, sigma, g, oracle, dense)
            planned.append(h.sky_stats()["units_planned"])
        st = h.sky_stats()
        assert planned[0] < planned[1] < st["units_dense"], "two different proper envelopes"
        assert st["plan_builds"] == 2 and st["cache_hits"] == 0
        for turn in range(2):
            for k, (g, dense) in enumerate(sets[:2]):
                got = h.lnlike_batch(lwl, g)
                assert lnp_close(got[0], dense[0]) and h.sky_stats()["units_planned"] == planned[k]
        st = h.sky_stats()
        assert st["plan_builds"] == 2 and st["cache_hits"] == 4
        # five envelopes through a cache of four: the first one is built again, with the same result
        for g, dense in sets[2:]:
            got = h.lnlike_batch(lwl, g)
            assert all(lnp_close(a, b) for a, b in zip(got, dense))
        builds = h.sky_stats()["plan_builds"]
        assert builds == 5, "five different proper envelopes"
        g, dense = sets[0]
        check(h.lnlike_batch(lwl, g), lwl, fl, sigma, g, oracle, dense)
        assert h.sky_stats()["plan_builds"] == builds + 1 and h.sky_stats()["units_planned"] == planned[0]
