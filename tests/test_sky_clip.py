"""CPU validation of the per-matrix clip inside the union skyline (psoap_sky_clip, the host twin of what the persistent
kernel reads through DagMat::first): the winning order's own envelope of every walker, replayed in NumPy, and the tile-GEMM
units those envelopes leave of the union's list."""
import ctypes

import numpy as np
import pytest

from psoap_amd import synthetic as syn
from test_sky_order import batch, cost, gpu_case, numpy_first, sky_order


def sky_clip(lwl, gp):
    from psoap_amd import _lib
    L = _lib.load()
    lwl = np.ascontiguousarray(lwl, dtype=np.float64)
    gp = np.ascontiguousarray(gp, dtype=np.float64)
    B, c, N = lwl.shape
    first_b = np.full((B, (N + 127) // 128), -1, dtype=np.int32)
    units = ctypes.c_longlong(-1)
    cand = ctypes.c_int(-1)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    rc = L.psoap_sky_clip(c, N, B, lwl.ctypes.data_as(dp), gp.ctypes.data_as(dp), first_b.ctypes.data_as(ip), ctypes.byref(units),
                          ctypes.byref(cand))
    assert rc == 0
    return first_b, units.value, cand.value


def numpy_first_b(lwl, gps, perm):
    """each walker's own envelope under `perm`: the replay of tests/test_sky_order.py on a batch of one"""
    return np.stack([numpy_first(lwl[b:b + 1], gps[b:b + 1], perm) for b in range(len(lwl))])


def check_clip(lwl, gps):
    """the twin against the replay: per matrix, inside the union, and the units; returns (first_b, first, units)"""
    first, perm, cand = sky_order(lwl, gps)
    first_b, units, cand_c = sky_clip(lwl, gps)
    assert cand_c == cand
    want = numpy_first_b(lwl, gps, perm)
    assert np.array_equal(first_b, want)
    assert np.array_equal(first_b.min(axis=0), first), "the union is the minimum over the batch"
    assert np.all(first_b >= first[None, :])
    assert units == sum(cost(fb) for fb in want)
    assert units <= len(lwl) * cost(first)
    return first_b, first, units


@pytest.mark.parametrize("c", [1, 2, 3])
def test_every_walkers_envelope_is_the_replays_and_lies_inside_the_union(c):
    lwl, gps = batch(c, 40 + c)
    check_clip(lwl, gps)


def test_narrow_kernels_in_every_other_walker_clip_the_union():
    # (the batches of tests/test_gpu_sky_clip.py)
    _, _, lwl, gps = gpu_case(2, 320)
    gps[1::2, 1::2] *= 0.3
    first_b, first, units = check_clip(lwl, gps)
    assert units < len(lwl) * cost(first)
    assert cost(first_b[1]) < cost(first_b[0])
    _, _, lwl, gps = gpu_case(3, 308)
    check_clip(lwl, gps)


def test_identical_walkers_clip_nothing():
    lwl, gps = batch(2, 42)
    lwl, gps = np.repeat(lwl[:1], 4, axis=0), np.repeat(gps[:1], 4, axis=0)
    first_b, first, units = check_clip(lwl, gps)
    assert (first > 0).any() and np.all(first_b == first[None, :]) and units == 4 * cost(first)


def test_a_walker_with_a_bad_hyperparameter_has_an_all_zero_row():
    lwl, gps = batch(2, 42)
    assert (sky_clip(lwl, gps)[0] > 0).any()
    for bad in (-0.2, 0.0, np.nan, np.inf, -np.inf):
        for col in (0, 1, 2, 3):
            g = gps.copy()
            g[1, col] = bad
            first_b, first, units = check_clip(lwl, g)
            assert not first_b[1].any() and not first.any(), (bad, col)
            # (candidate 0 wins a dense union; the other walkers keep their own envelopes in its order)
            assert (np.delete(first_b, 1, axis=0) > 0).any()


def test_the_headline_batch_executes_at_most_092_of_its_plan():
    """bench.py's 1-GPU input, both proposal sets.  A NumPy replay of the kernels gives clipped / planned = 0.898 (216936 of
    241472 units, 12 distinct envelopes among the 32 walkers); the bound leaves room for a differently rounded near-tie in
    a key."""
    chunk = syn.make_config_chunk(3, chunk_index=0)
    B = 32
    gps = syn.make_walkers(chunk.n_components, B, seed=3500)
    lwls = syn.walker_lwls(chunk, syn.make_walker_velocities(chunk, B, seed=3501))
    for lw, gp in ((lwls, gps), (np.roll(lwls, 1, axis=0).copy(), np.roll(gps, 1, axis=0).copy())):
        first_b, first, units = check_clip(lw, gp)
        planned = B * cost(first)
        per = [cost(fb) for fb in first_b]
        print(f"headline: planned {planned}, clipped {units} ({units / planned:.4f}), per walker {min(per)} .. {max(per)}, "
              f"{len({tuple(fb) for fb in first_b})} distinct envelopes")
        assert units / planned <= 0.92
