"""CPU validation of the row-granular clip (psoap_sky_clip16, the host twin of k_sky_fine: what DagMat::first points at):
per walker and column tile the first 16-row group that is not provably zero, replayed in NumPy, the 16-row stages the
updates then run inside the union's list, and the exact +0 of every row the kernel's K-loops skip."""
import ctypes

import numpy as np
import pytest

from psoap_amd import synthetic as syn
from test_sky_clip import sky_clip
from test_sky_order import batch, cost, gpu_case, sky_order
from test_sky_plan import numpy_cov

G = 16            # rows of a group: one stage of the tile engine's K-loop
GPT = 128 // G    # groups per tile


def sky_clip16(lwl, gp):
    from psoap_amd import _lib
    L = _lib.load()
    lwl = np.ascontiguousarray(lwl, dtype=np.float64)
    gp = np.ascontiguousarray(gp, dtype=np.float64)
    B, c, N = lwl.shape
    first16_b = np.full((B, (N + 127) // 128), -1, dtype=np.int32)
    stages = ctypes.c_longlong(-1)
    cand = ctypes.c_int(-1)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    rc = L.psoap_sky_clip16(c, N, B, lwl.ctypes.data_as(dp), gp.ctypes.data_as(dp), first16_b.ctypes.data_as(ip),
                            ctypes.byref(stages), ctypes.byref(cand))
    assert rc == 0
    return first16_b, stages.value, cand.value


def numpy_first16_b(lwl, gps, perm):
    """Every walker's envelope by 16-row groups under `perm`, replayed: group intervals against tile intervals, the
    p2 g g <= -746 test per component, the clamp to 8 max(j - 1, 0), the running minimum from the right."""
    B, c, N = lwl.shape
    P, NG = (N + 127) // 128, (N + G - 1) // G
    out = np.zeros((B, P), dtype=np.int64)
    for b in range(B):
        amp, ls = gps[b][0::2], gps[b][1::2]
        with np.errstate(over="ignore", invalid="ignore"):
            ok = bool(np.all((amp > 0) & (amp * amp < np.inf) & (ls > 0) & (ls < np.inf)))
        if not ok:
            continue
        x = lwl[b][:, perm]
        lo = np.array([[x[k, t * 128:(t + 1) * 128].min() for t in range(P)] for k in range(c)])
        hi = np.array([[x[k, t * 128:(t + 1) * 128].max() for t in range(P)] for k in range(c)])
        lo16 = np.array([[x[k, g * G:(g + 1) * G].min() for g in range(NG)] for k in range(c)])
        hi16 = np.array([[x[k, g * G:(g + 1) * G].max() for g in range(NG)] for k in range(c)])
        p2 = -0.5 * (syn.C_KMS * syn.C_KMS) / (ls * ls)

        def zero(g, j):
            for k in range(c):
                d = max(lo[k, j] - hi16[k, g], lo16[k, g] - hi[k, j])
                if not d > 0.0 or not p2[k] * d * d <= -746.0:
                    return False
            return True

        for j in range(P):
            g = 0
            while g < GPT * max(j - 1, 0) and zero(g, j):
                g += 1
            out[b, j] = g
        out[b] = np.minimum.accumulate(out[b][::-1])[::-1]
    return out


def stages_of(first, first16_b):
    """The 16-row stages of item 2's rule, per tile of the union's list: tile (q, j), first[j] < q <= j, updates over block
    rows [first[j], q) from row r0 = max(128 first[j], 16 first16) on -- the panels before the last from r0, the last panel
    whole unless r0 lies at or beyond row 128 q."""
    total = 0
    for f16 in first16_b:
        for j, (u, s) in enumerate(zip(first, f16)):
            r0 = max(128 * int(u), G * int(s))
            for q in range(int(u) + 1, j + 1):
                if G * int(s) >= 128 * q:
                    continue
                total += max(128 * (q - 1) - r0, 0) // G + GPT
    return total


def check_fine(lwl, gps):
    """the twin against the replay; returns (first16_b, first_b, first, stages)"""
    first, perm, cand = sky_order(lwl, gps)
    first_b, units, _ = sky_clip(lwl, gps)
    first16_b, stages, cand_c = sky_clip16(lwl, gps)
    P = len(first)
    assert cand_c == cand
    assert np.array_equal(first16_b, numpy_first16_b(lwl, gps, perm))
    assert np.all(first16_b >= GPT * first_b)
    assert np.all(np.diff(first16_b, axis=1) >= 0)
    assert np.all(first16_b <= GPT * np.maximum(np.arange(P) - 1, 0)[None, :])
    assert stages == stages_of(first, first16_b)
    assert stages <= GPT * units == stages_of(first, GPT * first_b)
    return first16_b, first_b, first, stages


@pytest.mark.parametrize("c", [1, 2, 3])
def test_every_walkers_first_row_group_is_the_replays(c):
    lwl, gps = batch(c, 40 + c)
    first16_b, first_b, first, stages = check_fine(lwl, gps)
    assert (first16_b > GPT * first_b).any(), "N = 1250 at l = 5-7 km/s: some column starts inside its first tile"


@pytest.mark.parametrize("c", [1, 2, 3])
def test_the_rows_above_the_first_group_are_exactly_zero(c):
    lwl, gps = batch(c, 40 + c)
    _, perm, _ = sky_order(lwl, gps)
    first16_b, _, _ = sky_clip16(lwl, gps)
    for b in range(len(lwl)):
        K = numpy_cov(lwl[b][:, perm], gps[b])
        for j, s in enumerate(first16_b[b]):
            blk = K[:G * s, 128 * j:128 * j + 128]
            assert np.all(blk == 0.0) and not np.signbit(blk).any(), (b, j)


def test_the_batches_of_the_device_tests():
    # (tests/test_gpu_sky_fine.py)
    for n in (1250, 1280):
        _, _, lwl, gps = gpu_case(2, 320, N=n)
        gps[1::2, 1::2] *= 0.3
        first16_b, first_b, first, stages = check_fine(lwl, gps)
        assert stages < GPT * sky_clip(lwl, gps)[1]
    _, _, lwl, gps = gpu_case(3, 308)
    check_fine(lwl, gps)
    # kernels too wide to clip anything: every column sits on its clamp
    _, _, lwl, gps = gpu_case(2, 320, scale=4.0)
    first16_b, first_b, first, stages = check_fine(lwl, gps)
    assert np.array_equal(first16_b, GPT * first_b) and stages == GPT * sky_clip(lwl, gps)[1]


def test_a_walker_with_a_bad_hyperparameter_has_an_all_zero_row():
    lwl, gps = batch(2, 42)
    assert (sky_clip16(lwl, gps)[0] > 0).any()
    for bad in (-0.2, 0.0, np.nan, np.inf, -np.inf):
        for col in (0, 1, 2, 3):
            g = gps.copy()
            g[1, col] = bad
            first16_b, first_b, first, stages = check_fine(lwl, g)
            assert not first16_b[1].any(), (bad, col)
            assert (np.delete(first16_b, 1, axis=0) > 0).any()


def test_identical_walkers_have_identical_rows():
    lwl, gps = batch(2, 42)
    lwl, gps = np.repeat(lwl[:1], 4, axis=0), np.repeat(gps[:1], 4, axis=0)
    first16_b, first_b, first, stages = check_fine(lwl, gps)
    assert (first16_b > 0).any() and np.all(first16_b == first16_b[0][None, :])


def test_the_headline_batch_runs_at_most_097_of_its_clipped_stages():
    """bench.py's 1-GPU input, both proposal sets.  A NumPy replay of the kernels gives 208872 panel equivalents of the
    216936 units the tile-level clip executes (0.9628); the bound leaves room for a differently rounded near-tie in a key."""
    chunk = syn.make_config_chunk(3, chunk_index=0)
    B = 32
    gps = syn.make_walkers(chunk.n_components, B, seed=3500)
    lwls = syn.walker_lwls(chunk, syn.make_walker_velocities(chunk, B, seed=3501))
    for lw, gp in ((lwls, gps), (np.roll(lwls, 1, axis=0).copy(), np.roll(gps, 1, axis=0).copy())):
        first, perm, cand = sky_order(lw, gp)
        first_b, units, _ = sky_clip(lw, gp)
        first16_b, stages, _ = sky_clip16(lw, gp)
        assert np.all(first16_b >= GPT * first_b) and stages == stages_of(first, first16_b)
        print(f"headline: candidate {cand}, units clipped {units}, stages {stages} = {stages / GPT:.1f} panels, "
              f"stages / (8 units) = {stages / (GPT * units):.4f}")
        assert stages / (GPT * units) <= 0.97
