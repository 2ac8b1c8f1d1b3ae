"""CPU validation of the skyline: the task list inside a monotone envelope (psoap_dag_plan_sky) and the zero test that
produces the envelope (psoap_sky_first, the host twin of the upload-side kernels)."""
import ctypes

import numpy as np
import pytest

from psoap_amd import synthetic as syn

TASK = np.dtype([("type", "u1"), ("q", "u1"), ("j", "u1"), ("S", "u1"), ("b", "<u2"), ("pa", "u1"), ("pb", "u1"),
                 ("slot", "<u4"), ("ctr", "<u4")])
PART, DIAG, OFF = 0, 1, 2
TYPE_MASK, CHAIN, NOSOLVE, WAITNEXT, FUSED = 0x0F, 0x10, 0x20, 0x40, 0x80
CTR_MASK = 0x00FFFFFF


def _raw(call):
    n, slots, ctrs = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
    qf = (ctypes.c_uint32 * 9)()
    assert call(None, 0, n, slots, ctrs, qf) == 0
    tasks = np.zeros(n.value, dtype=TASK)
    assert call(tasks.ctypes.data_as(ctypes.c_void_p), n.value, n, slots, ctrs, qf) == 0
    return tasks, slots.value, ctrs.value, list(qf)


def plan_dense(B, P, workers):
    from psoap_amd import _lib
    L = _lib.load()
    return _raw(lambda out, cap, n, s, c, qf: L.psoap_dag_plan(B, P, workers, out, cap, ctypes.byref(n), ctypes.byref(s),
                                                               ctypes.byref(c), qf))


def plan_sky(B, P, first, workers):
    from psoap_amd import _lib
    L = _lib.load()
    f = (ctypes.c_int * P)(*[int(v) for v in first])
    return _raw(lambda out, cap, n, s, c, qf: L.psoap_dag_plan_sky(B, P, f, workers, out, cap, ctypes.byref(n),
                                                                   ctypes.byref(s), ctypes.byref(c), qf))


@pytest.mark.parametrize("B", [1, 16, 32])
@pytest.mark.parametrize("P", [1, 2, 5, 10, 47])
def test_zero_skyline_is_the_dense_list(B, P, monkeypatch):
    monkeypatch.setenv("PSOAP_DAG_SCHEME", "0")
    a = plan_dense(B, P, 512)
    b = plan_sky(B, P, [0] * P, 512)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]
    # ... and whatever scheme the dense planner picks by itself
    monkeypatch.delenv("PSOAP_DAG_SCHEME")
    a = plan_dense(B, P, 512)
    b = plan_sky(B, P, [0] * P, 512)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]


def _profiles(P, rng):
    """Monotone envelopes with first[j] <= max(j - 1, 0)."""
    out = {"tight": [max(j - 1, 0) for j in range(P)],
           "band": [max(j - max(2, P // 4), 0) for j in range(P)],
           "step": [0 if j < P // 2 else min(P // 2 - 1, j - 1) for j in range(P)]}
    f = np.sort(rng.integers(0, P, size=P))
    out["seeded"] = [int(min(f[j], max(j - 1, 0))) for j in range(P)]
    for f in out.values():
        assert all(0 <= f[j] <= max(j - 1, 0) for j in range(P)) and all(f[j] <= f[j + 1] for j in range(P - 1))
    return out


@pytest.mark.parametrize("B,P,workers", [(1, 10, 512), (16, 10, 512), (32, 47, 512), (32, 64, 512), (3, 5, 8), (16, 2, 512)])
def test_skyline_list_is_complete_inside_the_envelope_and_deadlock_free(B, P, workers):
    rng = np.random.default_rng(1000 * B + P)
    for name, first in _profiles(P, rng).items():
        tasks, n_slots, n_ctrs, qf = plan_sky(B, P, first, workers)
        if not any(first):
            continue
        flags = tasks["type"].copy()
        ttype = tasks["type"] & TYPE_MASK
        assert not (flags & (CHAIN | WAITNEXT)).any(), "a skyline list is a throughput list"
        nq = 8 if B <= 8 else min((8, 4, 2, 1), key=lambda n: ((B + n - 1) // n * n, -n))
        assert qf[0] == 0 and qf[8] == len(tasks)
        for g in range(8):
            assert np.all(tasks["b"][qf[g]:qf[g + 1]] % nq == g)
        row_tiles = [sum(1 for j in range(q, P) if first[j] <= q) for q in range(P)]
        finals, parts, covered = {}, {}, {}
        slots_seen = set()
        for t, k in enumerate(tasks):
            b, q, j = int(k["b"]), int(k["q"]), int(k["j"])
            assert b < B and q <= j < P
            assert q >= first[j], f"{name}: task {t} names tile ({q}, {j}) outside the envelope"
            assert first[j] <= k["pa"] <= k["pb"] <= q
            if ttype[t] == PART:
                assert k["pb"] > k["pa"], "no PART over nothing"
                assert k["slot"] < n_slots and k["ctr"] < n_ctrs and int(k["slot"]) not in slots_seen and k["S"] == 0
                slots_seen.add(int(k["slot"]))
                parts.setdefault((b, q, j), []).append(t)
            else:
                assert (b, q, j) not in finals
                finals[(b, q, j)] = t
                assert (ttype[t] == DIAG) == (q == j)
                # the row's deficit against the dense P - q, in bits 24.. of ctr
                assert int(k["ctr"]) >> 24 == (P - q) - row_tiles[q]
                assert (int(k["ctr"]) & CTR_MASK) < max(n_ctrs, 1)
        # every tile inside the envelope has exactly one final, none outside
        want = {(b, q, j) for b in range(B) for j in range(P) for q in range(first[j], j + 1)}
        assert set(finals) == want
        for key, t in finals.items():
            b, q, j = key
            k = tasks[t]
            ps = parts.get(key, [])
            # S and ctr agree with the number of parts; the parts come first, in slot order, and with the final they
            # partition [first[j], q)
            assert int(k["S"]) == len(ps) + 1
            assert all(p < t for p in ps) and ps == sorted(ps)
            if ps:
                ctr = int(k["ctr"]) & CTR_MASK
                assert all(int(tasks[p]["ctr"]) == ctr for p in ps)
                assert sum(1 for p in np.flatnonzero((ttype == PART) & (tasks["ctr"] == ctr))) == len(ps)
                got = [int(tasks[p]["slot"]) for p in ps]
                assert got == list(range(got[0], got[0] + len(ps))) and int(k["slot"]) == got[0]
            pos = first[j]
            for p in ps + [t]:
                assert int(tasks[p]["pa"]) == pos
                pos = int(tasks[p]["pb"])
            assert pos == q
        # a sequential play-through in ticket order: whatever a task waits for holds a smaller ticket (of its queue: a
        # matrix lives in one queue)
        row_last = {}
        for (b, q, j), t in finals.items():
            row_last[(b, q)] = max(row_last.get((b, q), -1), t)
        for t, k in enumerate(tasks):
            b, q, j = int(k["b"]), int(k["q"]), int(k["j"])
            for m in range(int(k["pa"]), int(k["pb"])):       # the tiles the update reads: inside the envelope, earlier
                assert (b, m, q) in finals and (b, m, j) in finals
                assert finals[(b, m, q)] < t and finals[(b, m, j)] < t
            if ttype[t] == PART:
                continue
            if q > first[j]:
                # the final's range ends at q: behind the tile above it in its column (the right-hand side's turn order)
                assert int(k["pb"]) == q and finals[(b, q - 1, j)] < t
            if ttype[t] == DIAG and q >= 1:
                assert flags[t] & NOSOLVE and finals[(b, q - 1, q)] == t - 1 and flags[t - 1] & FUSED
                for m in range(q - 2):
                    assert row_last[(b, m)] < t
            if ttype[t] == OFF:
                assert finals[(b, q, q)] < t            # potrf(q)
                assert bool(flags[t] & FUSED) == (j == q + 1)


# ---- the zero test ------------------------------------------------------------------------------------------------
def sky_first(lwl, gp):
    from psoap_amd import _lib
    L = _lib.load()
    lwl = np.ascontiguousarray(lwl, dtype=np.float64)
    gp = np.ascontiguousarray(gp, dtype=np.float64)
    B, c, N = lwl.shape
    P = (N + 127) // 128
    first = np.zeros(P, dtype=np.int32)
    perm = np.zeros(N, dtype=np.int32)
    rc = L.psoap_sky_first(c, N, B, lwl.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                           gp.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                           first.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), perm.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    assert rc == 0
    return first, perm


def numpy_cov(lw, gp):
    """a^2 exp(p2 r^2) summed over the components, in the reference's order of operations (no sigma: off-diagonal tiles)"""
    cov = None
    for c in range(lw.shape[0]):
        a2 = gp[2 * c] * gp[2 * c]
        p2 = -0.5 * (syn.C_KMS * syn.C_KMS) / (gp[2 * c + 1] * gp[2 * c + 1])
        r = lw[c][None, :] - lw[c][:, None]
        with np.errstate(under="ignore"):
            t = a2 * np.exp(p2 * r * r)
        cov = t if cov is None else cov + t
    return cov


def masked_chunk(c, seed, N=1250):
    ch = syn.make_chunk(c, 4, 320, seed=seed)
    return ch, np.arange(ch.N)[:N]


def check_envelope(lwl, gps, first, perm):
    B, c, N = lwl.shape
    P = len(first)
    assert sorted(perm) == list(range(N))
    key = lwl[0, 0][perm]
    assert np.all(np.diff(key) >= 0)
    assert np.all(perm[1:][np.diff(key) == 0] > perm[:-1][np.diff(key) == 0]), "ties keep the input order"
    assert all(0 <= first[j] <= max(j - 1, 0) for j in range(P)) and all(first[j] <= first[j + 1] for j in range(P - 1))
    for b in range(B):
        K = numpy_cov(lwl[b][:, perm], gps[b])
        for j in range(P):
            if first[j] > 0:
                blk = K[:first[j] * 128, j * 128:(j + 1) * 128]
                assert np.all(blk == 0.0) and not np.signbit(blk).any(), (b, j)


@pytest.mark.parametrize("c", [1, 2, 3])
def test_tiles_outside_the_envelope_are_exactly_zero(c):
    ch, keep = masked_chunk(c, seed=40 + c)
    B = 4
    gps = syn.make_walkers(c, B, seed=7)
    vel = syn.make_walker_velocities(ch, B, seed=8)
    lwl = syn.walker_lwls(ch, vel)[:, :, keep]
    first, perm = sky_first(lwl, gps)
    check_envelope(lwl, gps, first, perm)
    assert (first > 0).any(), "N = 1250 at l = 5-7 km/s has a proper skyline"


def test_wide_kernel_and_bad_hyperparameters_give_the_dense_envelope():
    ch, keep = masked_chunk(2, seed=42)
    B = 4
    gps = syn.make_walkers(2, B, seed=7)
    lwl = syn.walker_lwls(ch, syn.make_walker_velocities(ch, B, seed=8))[:, :, keep]
    assert (sky_first(lwl, gps)[0] > 0).any()
    lo, hi = lwl.min(), lwl.max()
    wide = gps.copy()
    wide[2, 1] = 2.0 * (hi - lo) * syn.C_KMS          # one walker whose kernel spans the chunk
    first, perm = sky_first(lwl, wide)
    assert not first.any()
    check_envelope(lwl, wide, first, perm)
    for bad in (-0.2, 0.0, np.nan, np.inf, -np.inf):
        for col in (0, 1, 2, 3):
            g = gps.copy()
            g[1, col] = bad
            assert not sky_first(lwl, g)[0].any(), (bad, col)


def test_two_separated_ranges_meet_the_clamp_and_ties_are_stable():
    ch, keep = masked_chunk(1, seed=43, N=1024)
    lw = ch.lwls[:, keep].copy()
    lw[:, 512:] += 1.0                                 # two ranges far further apart than any kernel's support
    lw[0, 10:20] = lw[0, 10]                           # exact ties in the sort key
    lwl = lw[None]
    gps = np.array([syn.GP_BASE[1]])
    first, perm = sky_first(lwl, gps)
    check_envelope(lwl, gps, first, perm)
    assert first[4] == 3, "block-diagonal: column tile 4 starts at the clamp, not at its own block"
