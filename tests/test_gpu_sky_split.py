"""The skyline-aware split and order rules on the device (dag_plan.hpp, PSOAP_SKY_SPLIT): the new lists change the order of
summation and nothing else -- lnprob within the contract 1e-10 max(1, |lnp|) of a handle created under PSOAP_SKY_SPLIT=0 and
of the CPU oracle; the clip's argument does not depend on the split, so the default handle keeps its bits against
PSOAP_SKY_CLIP=0 and PSOAP_SKY_FINE=0 handles on the new lists; a slot evaluated twice and one walker at two batch positions
of different queues give the same bits.  B = 16 at N = 1250 (padded last tile) and N = 1280 (exact tiles), the three
envelope cases of tests/sky_split_cases.py."""
import ctypes

import numpy as np
import pytest

import sky_split_cases as cases
from test_sky_plan import PART, TASK, TYPE_MASK

# (a list whose finals counted on a PART that is not there would leave the kernel spinning up to its own spin limit: the
# time limit is short, and a time-out here is a finding about the list, not something to run again)
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(60)]

B = cases.GPU_B
SKY_ENV = ("PSOAP_SKYLINE", "PSOAP_SKY_ORDER", "PSOAP_SKY_CLIP", "PSOAP_SKY_FINE", "PSOAP_SKY_SPLIT")


@pytest.fixture(autouse=True)
def scheme0(monkeypatch):
    monkeypatch.setenv("PSOAP_DAG_SCHEME", "0")
    for name in SKY_ENV:
        monkeypatch.delenv(name, raising=False)


def device_list(h):
    n = ctypes.c_longlong(0)
    assert h._L.psoap_chunk_dag_tasks(h._h, None, 0, ctypes.byref(n)) == 0
    tasks = np.zeros(n.value, dtype=TASK)
    assert h._L.psoap_chunk_dag_tasks(h._h, tasks.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)) == 0
    return tasks


def evaluate(fl, sigma, lwl, gps, monkeypatch, twice=False, **env):
    """lnprob (of two evaluations of the same slot if `twice`), sky_stats and the task list of a fresh handle created under `env`"""
    from psoap_amd.chunk import ChunkHandle
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with ChunkHandle(fl, sigma, max_batch=B) as h:
        for k in env:
            monkeypatch.delenv(k)          # (read at creation: the evaluation runs without it)
        out = h.lnlike_batch(lwl, gps)
        if twice:
            h.upload(lwl, gps)
            h.eval()
            first_eval = h.fetch()
            h.eval()
            out = (out, first_eval, h.fetch())
        return out, h.sky_stats(), device_list(h)


@pytest.mark.parametrize("name,n", cases.GPU_CASES)
def test_the_new_lists_keep_the_results(monkeypatch, oracle, name, n):
    fl, sigma, lwl, gps = cases.gpu_batch(name, n)
    (got, again1, again2), st, tasks = evaluate(fl, sigma, lwl, gps, monkeypatch, twice=True)
    parent, st_parent, tasks_parent = evaluate(fl, sigma, lwl, gps, monkeypatch, PSOAP_SKY_SPLIT="0")
    noclip, _, tasks_noclip = evaluate(fl, sigma, lwl, gps, monkeypatch, PSOAP_SKY_CLIP="0")
    coarse, _, tasks_coarse = evaluate(fl, sigma, lwl, gps, monkeypatch, PSOAP_SKY_FINE="0")
    parts = lambda t: int(((t["type"] & TYPE_MASK) == PART).sum())
    print(f"{name} N={n}: {len(tasks)} tasks / {parts(tasks)} PARTs, parent {len(tasks_parent)} / {parts(tasks_parent)}; "
          f"max |d| / max(1, |lnp|) against the parent's list {np.max(np.abs(got - parent) / np.maximum(1.0, np.abs(parent))):.3g}")
    assert st["skyline_on"] == st_parent["skyline_on"] == 1
    assert np.all(np.isfinite(got))
    # the host's lists, both ways (tests/test_sky_split.py looks at them)
    first = cases.envelope(name, n)
    from test_sky_plan import plan_sky
    if any(first):          # (length scales x 4: a dense list, in the scheme the fixture pins -- psoap_dag_plan_sky picks its own)
        assert tasks.tobytes() == plan_sky(B, len(first), first, cases.WORKERS)[0].tobytes()
        monkeypatch.setenv("PSOAP_SKY_SPLIT", "0")
        assert tasks_parent.tobytes() == plan_sky(B, len(first), first, cases.WORKERS)[0].tobytes()
        monkeypatch.delenv("PSOAP_SKY_SPLIT")
        assert tasks.tobytes() != tasks_parent.tobytes()
    else:
        assert tasks.tobytes() == tasks_parent.tobytes()
    assert tasks.tobytes() == tasks_noclip.tobytes() == tasks_coarse.tobytes()
    # the order of summation changes: the contract, not the bits
    assert np.all(np.abs(got - parent) <= 1e-10 * np.maximum(1.0, np.abs(parent)))
    for b in (0, 1, B - 1):
        want = oracle.lnlike(lwl[b], fl, sigma, list(gps[b]))
        assert abs(got[b] - want) <= 1e-10 * max(1.0, abs(want)), (b, got[b], want)
    # the clip skips exact zeros whatever the split
    assert np.array_equal(got, noclip), np.max(np.abs(got - noclip))
    assert np.array_equal(got, coarse), np.max(np.abs(got - coarse))
    # the same slot twice
    assert np.array_equal(got, again1) and np.array_equal(again1, again2)


@pytest.mark.parametrize("name,n", [("narrow_odd", 1250), ("three", 1280)])
def test_a_walker_keeps_its_bits_in_another_queue(monkeypatch, name, n):
    """B = 16 runs on 8 queues, matrix b in queue b mod 8: walkers 1 and 2, and 5 and 14, change places (the first walker,
    whose grid gives the sort keys, stays): the same order, the same union skyline and list, every walker's bits as before"""
    fl, sigma, lwl, gps = cases.gpu_batch(name, n)
    where = np.arange(B)
    where[[1, 2, 5, 14]] = [2, 1, 14, 5]
    assert all(a % 8 != b % 8 for a, b in ((1, 2), (5, 14)))
    got, _, tasks = evaluate(fl, sigma, lwl, gps, monkeypatch)
    moved, _, tasks_moved = evaluate(fl, sigma, np.ascontiguousarray(lwl[where]), np.ascontiguousarray(gps[where]), monkeypatch)
    assert tasks.tobytes() == tasks_moved.tobytes()
    assert np.array_equal(got[where], moved)
