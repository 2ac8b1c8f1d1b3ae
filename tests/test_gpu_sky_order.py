"""The skyline's row order on the device: behind every upload the candidate orders are ranked, the cheapest union envelope
wins and the slot is gathered through the winner -- against the CPU oracle, a PSOAP_SKYLINE=0 handle and the host twin
psoap_sky_order, whose counts show that device and host chose the same candidate."""
import numpy as np
import pytest

from psoap_amd import synthetic as syn
from test_sky_order import cost, gpu_case, sky_order
from test_sky_plan import sky_first

pytestmark = pytest.mark.gpu

B = 16
N = 1250
P = 10
UNITS_DENSE = 165       # sum over j < 10 of j (j + 1) / 2
CASES = {"two components, length scales x 0.3": (2, 320, 0.3), "three components": (3, 308, 1.0)}


def lnp_close(got, want):
    return abs(got - want) <= 1e-10 * max(1.0, abs(want))


def tiles(first):
    return int(sum(j - f + 1 for j, f in enumerate(first)))


@pytest.fixture(autouse=True)
def scheme0(monkeypatch):
    monkeypatch.setenv("PSOAP_DAG_SCHEME", "0")
    monkeypatch.delenv("PSOAP_SKYLINE", raising=False)
    monkeypatch.delenv("PSOAP_SKY_ORDER", raising=False)


def evaluate(fl, sigma, lwl, gps, monkeypatch, env=None):
    """values and sky_stats of one batch on a fresh handle created under `env`"""
    from psoap_amd.chunk import ChunkHandle
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        with ChunkHandle(fl, sigma, max_batch=B) as h:
            return h.lnlike_batch(lwl, gps), h.sky_stats()
    finally:
        for k in (env or {}):
            monkeypatch.delenv(k)


_references = {}


def references(name, oracle, monkeypatch):
    """per case, computed once: the inputs, the oracle's values and those of a PSOAP_SKYLINE=0 handle"""
    if name not in _references:
        fl, sigma, lwl, gps = gpu_case(*CASES[name])
        want = np.array([oracle.lnlike(lwl[b], fl, sigma, list(gps[b])) for b in range(B)])
        dense, dstats = evaluate(fl, sigma, lwl, gps, monkeypatch, {"PSOAP_SKYLINE": "0"})
        assert dstats["skyline_on"] == 0 and dstats["tiles_planned"] == dstats["tiles_dense"]
        _references[name] = (fl, sigma, lwl, gps, want, dense)
    return _references[name]


@pytest.mark.parametrize("name", list(CASES))
def test_a_device_and_host_choose_the_same_order(oracle, monkeypatch, name):
    fl, sigma, lwl, gps, want, dense = references(name, oracle, monkeypatch)
    first, _, cand = sky_order(lwl, gps)
    assert cand != 0 and cost(first) < cost(sky_first(lwl, gps)[0]) < UNITS_DENSE
    got, st = evaluate(fl, sigma, lwl, gps, monkeypatch)
    for b in range(B):
        assert lnp_close(got[b], want[b]), (b, got[b], want[b])
        assert lnp_close(got[b], dense[b]), (b, got[b], dense[b])
    assert st["skyline_on"] == 1 and st["units_dense"] == B * UNITS_DENSE
    assert st["units_planned"] == B * cost(first) and st["tiles_planned"] == B * tiles(first)


@pytest.mark.parametrize("name", list(CASES))
def test_b_sky_order_off_is_candidate_zero(oracle, monkeypatch, name):
    fl, sigma, lwl, gps, want, dense = references(name, oracle, monkeypatch)
    first0, perm0 = sky_first(lwl, gps)
    off = {"PSOAP_SKY_ORDER": "0"}
    got, st = evaluate(fl, sigma, lwl, gps, monkeypatch, off)
    assert st["units_planned"] == B * cost(first0) and st["tiles_planned"] == B * tiles(first0)
    for b in range(B):
        assert lnp_close(got[b], want[b]), (b, got[b], want[b])
    # the explicit candidate-0 plan: the rows handed over in psoap_sky_first's order, which the device then leaves as they are
    lwl_s = np.ascontiguousarray(lwl[:, :, perm0])
    assert np.array_equal(sky_first(lwl_s, gps)[1], np.arange(N)) and np.array_equal(sky_first(lwl_s, gps)[0], first0)
    explicit, st2 = evaluate(fl[perm0], sigma[perm0], lwl_s, gps, monkeypatch, off)
    assert st2["units_planned"] == st["units_planned"]
    assert np.array_equal(got, explicit)


def test_c_both_upload_paths_choose_alike_and_repeat(oracle, monkeypatch):
    from psoap_amd.chunk import ChunkHandle
    ch = syn.make_chunk(2, 4, 320, seed=320)
    gps = syn.make_walkers(2, B, seed=321)
    gps[:, 1::2] *= 0.3
    vel = syn.make_walker_velocities(ch, B, seed=322)
    lwl = syn.walker_lwls(ch, vel)
    first, _, cand = sky_order(lwl, gps)
    assert cand != 0
    with ChunkHandle(ch.fl, ch.sigma, max_batch=B) as h:
        h.set_grid(ch.lwl, ch.epoch_index, ch.n_epochs)
        h.upload(lwl, gps)
        h.eval()
        a = h.fetch()
        st = h.sky_stats()
        h.upload_velocities(vel, gps)              # the other slot, the device-side Doppler shift
        h.eval()
        b = h.fetch()
        st_b = h.sky_stats()
        again = h.lnlike_batch(lwl, gps)           # the same batch a second time through the first slot
    assert st["units_planned"] == st_b["units_planned"] == B * cost(first)
    assert np.array_equal(a, b) and np.array_equal(a, again)
    with ChunkHandle(ch.fl, ch.sigma, max_batch=B) as fresh:
        assert np.array_equal(fresh.lnlike_batch(lwl, gps), a)
    for k in range(B):
        assert lnp_close(a[k], oracle.lnlike(lwl[k], ch.fl, ch.sigma, list(gps[k]))), (k, a[k])


def test_d_four_fold_ties_in_every_candidate_key_are_deterministic(oracle, monkeypatch):
    ch = syn.make_chunk(2, 4, 320, seed=302)
    keep = np.arange(ch.N)[:N]
    gps = syn.make_walkers(2, B, seed=303)
    # no jitter, equal velocities in all epochs: every epoch's grid is the same, in both components
    grid = np.tile(ch.lwl[:320], 4)[keep]
    lwl = np.stack([np.stack([grid - 3.0 / syn.C_KMS, grid + 2.0 / syn.C_KMS])] * B)
    fl, sigma = ch.fl[keep], np.maximum(ch.sigma[keep], 0.02)
    first, _, _ = sky_order(lwl, gps)
    a, st = evaluate(fl, sigma, lwl, gps, monkeypatch)
    b, _ = evaluate(fl, sigma, lwl, gps, monkeypatch)
    assert np.array_equal(a, b)
    assert st["units_planned"] == B * cost(first)
    dense, _ = evaluate(fl, sigma, lwl, gps, monkeypatch, {"PSOAP_SKYLINE": "0"})
    for k in range(B):
        assert lnp_close(a[k], dense[k]), (k, a[k], dense[k])
    assert lnp_close(a[0], oracle.lnlike(lwl[0], fl, sigma, list(gps[0])))


def test_e_one_wide_walker_makes_every_candidate_dense(oracle, monkeypatch):
    fl, sigma, lwl, gps, _, _ = references("two components, length scales x 0.3", oracle, monkeypatch)
    gps = gps.copy()
    gps[5, 1] = 60.0
    first, _, cand = sky_order(lwl, gps)
    assert cand == 0 and not first.any()
    got, st = evaluate(fl, sigma, lwl, gps, monkeypatch)
    assert st["tiles_planned"] == st["tiles_dense"] and st["units_planned"] == st["units_dense"]
    dense, _ = evaluate(fl, sigma, lwl, gps, monkeypatch, {"PSOAP_SKYLINE": "0"})
    for k in range(B):
        assert lnp_close(got[k], dense[k]), (k, got[k], dense[k])
    assert lnp_close(got[5], oracle.lnlike(lwl[5], fl, sigma, list(gps[5])))
