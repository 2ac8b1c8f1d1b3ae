"""The per-matrix clip inside the union skyline on the device: every matrix's updates start at its own envelope
(DagMat::first), the results keep their bits -- against a handle created under PSOAP_SKY_CLIP=0, which runs the union's
ranges for every matrix, against the CPU oracle, and the units against the host twin (tests/test_sky_clip.py)."""
import ctypes

import numpy as np
import pytest

from test_sky_clip import sky_clip
from test_sky_order import cost, gpu_case, sky_order
from test_sky_plan import TASK

pytestmark = pytest.mark.gpu

B = 16
N = 1250


@pytest.fixture(autouse=True)
def scheme0(monkeypatch):
    monkeypatch.setenv("PSOAP_DAG_SCHEME", "0")
    monkeypatch.delenv("PSOAP_SKYLINE", raising=False)
    monkeypatch.delenv("PSOAP_SKY_ORDER", raising=False)
    monkeypatch.delenv("PSOAP_SKY_CLIP", raising=False)


def lnp_close(got, want):
    return abs(got - want) <= 1e-10 * max(1.0, abs(want))


def dag_tasks(h):
    """the task list of the handle's last evaluation, from the device"""
    n = ctypes.c_longlong()
    assert h._L.psoap_chunk_dag_tasks(h._h, None, 0, ctypes.byref(n)) == 0
    tasks = np.zeros(n.value, dtype=TASK)
    assert h._L.psoap_chunk_dag_tasks(h._h, tasks.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)) == 0
    return tasks


def emptied(tasks, first_b):
    """task ranges [pa, pb) of the list that the clip empties: the matrix's own envelope starts at or below pb"""
    fb = first_b[tasks["b"].astype(np.int64), tasks["j"].astype(np.int64)]
    return int(np.sum((tasks["pb"] > tasks["pa"]) & (fb >= tasks["pb"])))


def unclipped(fl, sigma, lwl, gps, monkeypatch):
    from psoap_amd.chunk import ChunkHandle
    monkeypatch.setenv("PSOAP_SKY_CLIP", "0")
    with ChunkHandle(fl, sigma, max_batch=B) as h:
        out = h.lnlike_batch(lwl, gps)
        st = h.sky_stats()
    monkeypatch.delenv("PSOAP_SKY_CLIP")
    assert st["skyline_on"] == 1 and st["units_clipped"] == st["units_planned"]
    return out, st


def run(fl, sigma, lwl, gps, monkeypatch, oracle, proper=True):
    """lnprob with the clip against the same library without it (bit for bit) and the oracle; the units against the twin.
    proper: the clip must take units out of the plan and empty at least one task's range."""
    from psoap_amd.chunk import ChunkHandle
    first, _, _ = sky_order(lwl, gps)
    first_b, units, _ = sky_clip(lwl, gps)
    planned = len(lwl) * cost(first)
    assert (first > 0).any()
    assert units < planned if proper else units == planned
    with ChunkHandle(fl, sigma, max_batch=B) as h:
        got = h.lnlike_batch(lwl, gps)
        st = h.sky_stats()
        tasks = dag_tasks(h)
    print(f"planned {planned}, clipped {units}, {emptied(tasks, first_b)} of {len(tasks)} task ranges emptied")
    assert (emptied(tasks, first_b) > 0) == proper
    off, st_off = unclipped(fl, sigma, lwl, gps, monkeypatch)
    assert np.array_equal(got, off, equal_nan=True), np.max(np.abs(got - off))
    for b in range(len(got)):
        want = oracle.lnlike(lwl[b], fl, sigma, list(gps[b]))
        assert lnp_close(got[b], want), (b, got[b], want)
    assert st["skyline_on"] == 1
    assert st["units_planned"] == planned == st_off["units_planned"] and st["tiles_planned"] == st_off["tiles_planned"]
    assert st["units_clipped"] == units
    return got


def odd_walkers_narrow(n=N):
    fl, sigma, lwl, gps = gpu_case(2, 320, N=n)
    gps[1::2, 1::2] *= 0.3
    return fl, sigma, lwl, gps


@pytest.mark.parametrize("n", [N, 1280])
def test_two_components_narrow_odd_walkers(oracle, monkeypatch, n):
    """a large clip: the even walkers' envelopes make the union, the odd ones' lie far inside it (n = 1250: a ragged last tile)"""
    run(*odd_walkers_narrow(n), monkeypatch, oracle)


def test_three_components(oracle, monkeypatch):
    """gpu_case(3, 308): the host twin gives all 16 walkers the union's envelope (1120 units planned, 1120 clipped), so this
    batch cannot meet "clipped < planned"; it stays as the three-component batch the clip must leave alone, and the same
    batch with narrow odd walkers (1120 planned, 760 clipped) carries the full set of assertions"""
    fl, sigma, lwl, gps = gpu_case(3, 308)
    run(fl, sigma, lwl, gps, monkeypatch, oracle, proper=False)
    gps[1::2, 1::2] *= 0.3
    run(fl, sigma, lwl, gps, monkeypatch, oracle)


def test_identical_walkers_clip_nothing(oracle, monkeypatch):
    fl, sigma, lwl, gps = gpu_case(2, 320)
    lwl, gps = np.ascontiguousarray(np.repeat(lwl[:1], B, axis=0)), np.repeat(gps[:1], B, axis=0)
    got = run(fl, sigma, lwl, gps, monkeypatch, oracle, proper=False)
    assert np.all(got == got[0])


def test_the_clip_is_a_function_of_the_slot_alone(monkeypatch):
    """two uploads with different clips, each into both slots of one handle in turn: every result is a fresh handle's"""
    from psoap_amd.chunk import ChunkHandle
    fl, sigma, lwl, gps = odd_walkers_narrow()
    gps2 = gps.copy()
    gps2[1::2, 1::2] /= 0.3
    gps2[0::4, 1::2] *= 0.3
    fresh = []
    for g in (gps, gps2):
        with ChunkHandle(fl, sigma, max_batch=B) as h:
            fresh.append(h.lnlike_batch(lwl, g))
            assert h.sky_stats()["units_clipped"] == sky_clip(lwl, g)[1] < h.sky_stats()["units_planned"]
    assert not np.array_equal(sky_clip(lwl, gps)[0], sky_clip(lwl, gps2)[0])
    with ChunkHandle(fl, sigma, max_batch=B) as h:
        for turn in (0, 1, 1, 0, 0):
            g = (gps, gps2)[turn]
            assert np.array_equal(h.lnlike_batch(lwl, g), fresh[turn], equal_nan=True), turn
            assert h.sky_stats()["units_clipped"] == sky_clip(lwl, g)[1]
