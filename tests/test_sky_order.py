"""CPU validation of the skyline's row order (psoap_sky_order, the host twin of the upload-side kernels with the choice):
every candidate order is a blend of the first walker's component grids, the cheapest union envelope wins, and whatever
wins is a valid envelope -- every tile outside it exactly +0."""
import ctypes

import numpy as np
import pytest

from psoap_amd import synthetic as syn
from test_sky_plan import masked_chunk, numpy_cov, sky_first


def sky_order(lwl, gp):
    from psoap_amd import _lib
    L = _lib.load()
    lwl = np.ascontiguousarray(lwl, dtype=np.float64)
    gp = np.ascontiguousarray(gp, dtype=np.float64)
    B, c, N = lwl.shape
    first = np.zeros((N + 127) // 128, dtype=np.int32)
    perm = np.zeros(N, dtype=np.int32)
    cand = ctypes.c_int(-1)
    ip = ctypes.POINTER(ctypes.c_int)
    rc = L.psoap_sky_order(c, N, B, lwl.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                           gp.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), first.ctypes.data_as(ip), perm.ctypes.data_as(ip),
                           ctypes.byref(cand))
    assert rc == 0
    return first, perm, cand.value


def weights(c):
    """the candidates' blends, in the library's enumeration"""
    if c == 1:
        return [(1.0,)]
    if c == 2:
        return [(1 - k / 8, k / 8) for k in range(9)]
    return [((4 - a - b) / 4, a / 4, b / 4) for a in range(5) for b in range(5 - a)]


def cand_key(lwl, w):
    """sum of w[c] * lwl[0][c] left to right, terms of weight 0 skipped (NumPy contracts nothing)"""
    key = None
    for c, wc in enumerate(w):
        if wc == 0.0:
            continue
        t = wc * lwl[0, c]
        key = t if key is None else key + t
    return key


def cost(first):
    d = np.arange(len(first)) - np.asarray(first, dtype=np.int64)
    return int(np.sum(d * (d + 1) // 2))


def dense_cost(P):
    return cost(np.zeros(P, dtype=np.int64))


def numpy_first(lwl, gps, perm):
    """The union envelope of the batch under `perm`, replayed: tile intervals, the p2 g g <= -746 test per component, the
    j - 1 clamp, the running minimum from the right, the minimum over the walkers."""
    B, c, N = lwl.shape
    P = (N + 127) // 128
    union = None
    for b in range(B):
        amp, ls = gps[b][0::2], gps[b][1::2]
        with np.errstate(over="ignore", invalid="ignore"):
            ok = bool(np.all((amp > 0) & (amp * amp < np.inf) & (ls > 0) & (ls < np.inf)))
        fb = np.zeros(P, dtype=np.int64)
        if ok:
            x = lwl[b][:, perm]
            lo = np.array([[x[k, t * 128:(t + 1) * 128].min() for t in range(P)] for k in range(c)])
            hi = np.array([[x[k, t * 128:(t + 1) * 128].max() for t in range(P)] for k in range(c)])
            p2 = -0.5 * (syn.C_KMS * syn.C_KMS) / (ls * ls)

            def zero(q, j):
                for k in range(c):
                    g = max(lo[k, j] - hi[k, q], lo[k, q] - hi[k, j])
                    if not g > 0.0 or not p2[k] * g * g <= -746.0:
                        return False
                return True

            for j in range(P):
                q = 0
                while q < j and zero(q, j):
                    q += 1
                fb[j] = q
        fb = np.minimum(fb, np.maximum(np.arange(P) - 1, 0))
        fb = np.minimum.accumulate(fb[::-1])[::-1]
        union = fb if union is None else np.minimum(union, fb)
    return union


def check_order(lwl, gps, first, perm, cand):
    """perm ascends in the chosen candidate's key with ties in input order; first is a clamped monotone envelope outside
    which every walker's covariance is exactly +0"""
    B, c, N = lwl.shape
    P = len(first)
    assert 0 <= cand < len(weights(c))
    assert sorted(perm) == list(range(N))
    key = cand_key(lwl, weights(c)[cand])[perm]
    d = np.diff(key)
    assert np.all(d >= 0)
    assert np.all(perm[1:][d == 0] > perm[:-1][d == 0]), "ties keep the input order"
    assert all(0 <= first[j] <= max(j - 1, 0) for j in range(P)) and all(first[j] <= first[j + 1] for j in range(P - 1))
    for b in range(B):
        K = numpy_cov(lwl[b][:, perm], gps[b])
        for j in range(P):
            if first[j] > 0:
                blk = K[:first[j] * 128, j * 128:(j + 1) * 128]
                assert np.all(blk == 0.0) and not np.signbit(blk).any(), (b, j)


def check_choice(lwl, gps, first, cand):
    """the candidate returned has the smallest cost over all of them (the lowest index among equals), recomputed here"""
    c = lwl.shape[1]
    costs = []
    for w in weights(c):
        perm = np.argsort(cand_key(lwl, w), kind="stable")
        costs.append(cost(numpy_first(lwl, gps, perm)))
    assert cand == int(np.argmin(costs)), (cand, costs)          # (argmin: the first of equal minima)
    assert cost(first) == costs[cand]
    assert cost(first) <= cost(sky_first(lwl, gps)[0]) == costs[0]
    return costs


def batch(c, seed, B=4, N=1250):
    ch, keep = masked_chunk(c, seed=seed, N=N)
    gps = syn.make_walkers(c, B, seed=seed + 1)
    lwl = syn.walker_lwls(ch, syn.make_walker_velocities(ch, B, seed=seed + 2))[:, :, keep]
    return np.ascontiguousarray(lwl), gps


@pytest.mark.parametrize("c", [1, 2, 3])
def test_the_chosen_order_is_a_permutation_with_an_exactly_zero_outside(c):
    lwl, gps = batch(c, 40 + c)
    first, perm, cand = sky_order(lwl, gps)
    check_order(lwl, gps, first, perm, cand)
    check_choice(lwl, gps, first, cand)
    assert (first > 0).any(), "N = 1250 at l = 5-7 km/s has a proper skyline"


def test_one_component_is_the_order_of_today():
    lwl, gps = batch(1, 41)
    first, perm, cand = sky_order(lwl, gps)
    f0, p0 = sky_first(lwl, gps)
    assert cand == 0 and np.array_equal(first, f0) and np.array_equal(perm, p0)


def test_two_separated_ranges_meet_the_clamp_and_ties_are_stable():
    ch, keep = masked_chunk(1, seed=43, N=1024)
    lw = ch.lwls[:, keep].copy()
    lw[:, 512:] += 1.0
    lw[0, 10:20] = lw[0, 10]
    lwl = lw[None]
    gps = np.array([syn.GP_BASE[1]])
    first, perm, cand = sky_order(lwl, gps)
    check_order(lwl, gps, first, perm, cand)
    assert cand == 0 and first[4] == 3
    # two components on the same two ranges, four-fold ties in every candidate's key
    ch2, keep = masked_chunk(2, seed=44, N=1024)
    grid = np.tile(ch2.lwl[:256], 4)
    grid[512:] += 1.0
    lwl2 = np.stack([np.stack([grid - 3.0 / syn.C_KMS, grid + 2.0 / syn.C_KMS])] * 3)
    gps2 = syn.make_walkers(2, 3, seed=45)
    first, perm, cand = sky_order(lwl2, gps2)
    check_order(lwl2, gps2, first, perm, cand)
    check_choice(lwl2, gps2, first, cand)
    assert first[4] == 3


def test_an_exact_tie_goes_to_the_lowest_candidate():
    # equal grids in both components: every blend orders the rows alike, every candidate costs the same
    lwl, gps = batch(2, 46)
    same = lwl.copy()
    same[:, 1] = same[:, 0]
    first, perm, cand = sky_order(same, gps)
    costs = check_choice(same, gps, first, cand)
    assert len(set(costs)) == 1 and costs[0] < dense_cost(len(first)) and cand == 0
    check_order(same, gps, first, perm, cand)
    # one walker whose kernel spans the chunk: every candidate is dense
    wide = gps.copy()
    wide[2, 1] = 2.0 * (lwl.max() - lwl.min()) * syn.C_KMS
    first, perm, cand = sky_order(lwl, wide)
    assert cand == 0 and not first.any()
    assert np.array_equal(perm, sky_first(lwl, wide)[1])


def test_bad_hyperparameters_give_the_dense_envelope_with_candidate_zero():
    lwl, gps = batch(2, 42)
    assert (sky_order(lwl, gps)[0] > 0).any()
    for bad in (-0.2, 0.0, np.nan, np.inf, -np.inf):
        for col in (0, 1, 2, 3):
            g = gps.copy()
            g[1, col] = bad
            first, perm, cand = sky_order(lwl, g)
            assert cand == 0 and not first.any(), (bad, col)
            assert np.array_equal(perm, sky_first(lwl, g)[1])


def gpu_case(c, seed, scale=1.0, B=16, N=1250):
    """the batches of tests/test_gpu_skyline.py: chunk(c, seed), length scales times `scale`"""
    ch = syn.make_chunk(c, 4, 320, seed=seed)
    keep = np.arange(ch.N)[:N]
    gps = syn.make_walkers(c, B, seed=seed + 1)
    gps[:, 1::2] *= scale
    lwl = syn.walker_lwls(ch, syn.make_walker_velocities(ch, B, seed=seed + 2))[:, :, keep]
    return ch.fl[keep], ch.sigma[keep], np.ascontiguousarray(lwl), gps


def test_two_components_narrow_kernels_choose_a_quarter_blend():
    _, _, lwl, gps = gpu_case(2, 320, scale=0.3)
    first, perm, cand = sky_order(lwl, gps)
    check_order(lwl, gps, first, perm, cand)
    check_choice(lwl, gps, first, cand)
    assert (cand, cost(first), cost(sky_first(lwl, gps)[0])) == (2, 25, 46)


def test_three_components_choose_an_interior_blend():
    _, _, lwl, gps = gpu_case(3, 308)
    first, perm, cand = sky_order(lwl, gps)
    check_order(lwl, gps, first, perm, cand)
    check_choice(lwl, gps, first, cand)
    assert weights(3)[10] == (0.25, 0.5, 0.25)
    assert (cand, cost(first), dense_cost(len(first))) == (10, 70, 165)


def test_the_headline_batch_plans_under_half_of_dense():
    """bench.py's 1-GPU input: configs[2] chunk, 32 walkers, both proposal sets.  A NumPy replay of the kernels gives 0.436 of
    the dense tile-GEMM units with candidate 6; the bound leaves room for a differently rounded near-tie in a key."""
    chunk = syn.make_config_chunk(3, chunk_index=0)
    B = 32
    gps = syn.make_walkers(chunk.n_components, B, seed=3500)
    vels = syn.make_walker_velocities(chunk, B, seed=3501)
    lwls = syn.walker_lwls(chunk, vels)
    for lw, gp in ((lwls, gps), (np.roll(lwls, 1, axis=0).copy(), np.roll(gps, 1, axis=0).copy())):
        first, perm, cand = sky_order(lw, gp)
        ratio = cost(first) / dense_cost(len(first))
        old = cost(sky_first(lw, gp)[0]) / dense_cost(len(first))
        print(f"headline: candidate {cand}, planned / dense units = {ratio:.4f} (candidate 0: {old:.4f})")
        assert sorted(perm) == list(range(chunk.N))
        assert ratio <= 0.45
