"""GPU: the life of the host layer's device resources -- a create that fails half way, a stream opened again with another
shape, a grid replaced by a larger and a smaller one, a group and its members destroyed in either order, the early returns
of the calibration solve.  Every buffer, stream and event is owned by the field that holds it (csrc/common.hpp), so none of
these paths names what it gives back; the tests pin what the paths compute.  Shapes: N = 200 (two block rows, the second
padded) and N = 128 (one tile exactly), two components, three proposals."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from psoap_amd import synthetic as syn
from psoap_amd._lib import PsoapError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

LNP_RTOL = 1e-10      # tests/test_gpu_parity.py: |dlnp| <= 1e-10 max(1, |lnp|)
C, B = 2, 3


def close(a, b, rtol=LNP_RTOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b))))


def _chunk(N, seed):
    ch = syn.make_chunk(C, 2, N // 2, seed=seed)
    assert ch.N == N
    return ch


def _props(ch, seed):
    gps = syn.make_walkers(C, B, seed=seed)
    return syn.walker_lwls(ch, syn.make_walker_velocities(ch, B, seed=seed + 1)), gps


def _device_total_bytes():
    """torch.cuda.mem_get_info()[1], asked in a child process: torch brings a HIP runtime of its own, which finds no device in
    a process where the library's runtime is already up (any test that ran before this one)"""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.mem_get_info()[1])"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return int(out.stdout.split()[-1])


def test_create_that_fails_gives_everything_back(oracle):
    """max_batch so large that the matrices alone (8 max_batch 128^2 bytes) exceed the device's total memory: the
    allocation is refused whatever else runs on the card, before any pinned memory has been asked for; the two 1 KiB arrays
    allocated ahead of it go back, and the next handle works."""
    from psoap_amd.chunk import ChunkHandle
    ch = _chunk(128, 7301)
    total = _device_total_bytes()
    too_many = total // (8 * 128 * 128) + 1
    with pytest.raises(PsoapError, match="hipMalloc"):
        ChunkHandle(ch.fl, ch.sigma, max_batch=too_many)
    lw, gps = _props(ch, 7302)
    want = np.array([oracle.lnlike(lw[b], ch.fl, ch.sigma, gps[b]) for b in range(B)])
    with ChunkHandle(ch.fl, ch.sigma, max_batch=B) as h:
        got = h.lnlike_batch(lw, gps)
    assert close(got, want), (got, want)


def test_stream_reopened_with_other_lanes_and_schemes():
    """Open, use, close, three times over with other lane counts and schemes; a second close is a no-op; then a batch.
    What tests/test_gpu_stream.py asserts for a single open holds for every reopen: the stream's values agree with the
    handle's batch path to LNP_RTOL and the batch path returns its earlier bits afterwards.  Bit for bit, a reopened stream
    equals the FIRST open of a fresh handle with the same lanes and scheme.  (Stream against batch is not bit-identical, at
    the parent commit either: a lane runs the task list of one matrix, the batch launch a list over all three in sorted
    order, and the sums associate differently -- measured: 1 ulp, 2.2e-16 relative, for schemes 0 and 1; equal for 2.)"""
    from psoap_amd.chunk import ChunkHandle
    ch = _chunk(200, 7311)
    lw, gps = _props(ch, 7312)
    opens = ((2, 0), (3, 1), (3, 2))

    def through_stream(h, lanes, scheme):
        h.stream_open(C, lanes, scheme)
        out = [h.stream_fetch(h.stream_submit(lw[b:b + lanes], gps[b:b + lanes])) for b in range(0, B, lanes)]
        h.stream_close()
        return np.concatenate(out)

    with ChunkHandle(ch.fl, ch.sigma, max_batch=B) as h:
        batch = h.lnlike_batch(lw, gps)
        got = [through_stream(h, lanes, scheme) for lanes, scheme in opens]
        h.stream_close()                       # nothing open: a no-op
        after = h.lnlike_batch(lw, gps)
    assert np.all(np.isfinite(batch)) and np.array_equal(after, batch), (after, batch)
    for (lanes, scheme), g in zip(opens, got):
        with ChunkHandle(ch.fl, ch.sigma, max_batch=B) as fresh:
            first = through_stream(fresh, lanes, scheme)
        print("LIFEROW", lanes, scheme, float(np.max(np.abs(g - batch) / np.maximum(1.0, np.abs(batch)))),
              bool(np.array_equal(g, batch)), bool(np.array_equal(g, first)))
        assert close(g, batch), (lanes, scheme, g, batch)
        assert np.array_equal(g, first), (lanes, scheme, g, first)


def test_grid_replaced_by_a_larger_and_a_smaller_one():
    """set_grid with 4, then 9, then 2 epochs on one handle: the velocity buffers are sized by the call, and each upload
    evaluates what the host forms as lwl + (-v) / c (tests/orbit_cases.py: grids_from_velocities)."""
    from psoap_amd.chunk import ChunkHandle
    ch = _chunk(200, 7321)
    gps = syn.make_walkers(C, B, seed=7322)
    rng = np.random.default_rng(7323)
    with ChunkHandle(ch.fl, ch.sigma, max_batch=B) as h:
        for ne in (4, 9, 2):
            epoch = rng.permutation(ne)[np.arange(ch.N) * ne // ch.N].astype(np.int32)      # runs of pixels, labels shuffled
            vel = rng.uniform(-60.0, 60.0, size=(B, C, ne))
            h.set_grid(ch.lwl, epoch, ne)
            h.upload_velocities(vel, gps)
            h.eval()
            got = h.fetch()
            want = h.lnlike_batch(ch.lwl + (-vel[..., epoch]) / syn.C_KMS, gps)
            assert np.all(np.isfinite(want)) and np.array_equal(got, want), (ne, got, want)


@pytest.mark.parametrize("group_last", [False, True])
def test_group_and_members_destroyed_in_either_order(group_last):
    """the group goes before its members fetch (and they evaluate alone afterwards), or after one member is gone"""
    from psoap_amd.chunk import ChunkGroup, ChunkHandle
    chunks = [_chunk(200, 7331), _chunk(128, 7332)]
    props = [_props(ch, 7333 + k) for k, ch in enumerate(chunks)]
    handles = [ChunkHandle(ch.fl, ch.sigma, max_batch=B) for ch in chunks]
    try:
        own = [h.lnlike_batch(*p) for h, p in zip(handles, props)]
        g = ChunkGroup(handles)
        for h, p in zip(handles, props):
            h.upload(*p)
        g.eval()
        if group_last:
            first = handles[0].fetch()
            handles[0].close()
            g.close()
            grouped = [first, handles[1].fetch()]
            alone = [own[0], handles[1].lnlike_batch(*props[1])]
        else:
            g.close()
            grouped = [h.fetch() for h in handles]
            alone = [h.lnlike_batch(*p) for h, p in zip(handles, props)]
    finally:
        for h in handles:
            h.close()
    for k in range(2):
        assert np.all(np.isfinite(own[k]))
        assert close(grouped[k], own[k]), (k, grouped[k], own[k])
        assert np.array_equal(alone[k], own[k]), (k, alone[k], own[k])


def test_calibration_status_return_then_a_good_call(oracle):
    """B with a negative diagonal entry: status 1 from the first pass, no error; the next, well-posed call is unaffected"""
    from make_golden_host import cal_case
    import calibration_reference as cr
    from test_gpu_calibration import TOL_ORACLE      # against the float64 oracle: (8 + 1) x the float64 evaluation's error
    from psoap_amd import _lib
    from psoap_amd import covariance as cov
    case = cal_case(syn, C, 2, 128, 7341, 0.0, 1.04, limit_array=1)
    M, N, order = case["lwl_cal"].size, case["fl_fixed"].size, 1
    assert (M, N) == (128, 128)
    A, Bm, Cm = oracle.calibration_blocks(case["lwls_cal"], case["sigma_cal"], case["lwls_fixed"], case["sigma_fixed"],
                                          case["gp"])
    bad = np.ascontiguousarray(Bm, dtype=np.float64).copy()
    bad[5, 5] = -1.0
    arrs = [_lib.as_f64(case[k]) for k in ("lwl_cal", "fl_cal", "fl_fixed")] + [_lib.as_f64(A), bad, _lib.as_f64(Cm)]
    fl_cor, X, status = np.empty(M), np.empty(order + 1), ctypes.c_int(-1)
    rc = _lib.load().psoap_calibrate_explicit(_lib.default_device(), M, N, order, float(case["lwl0"]), float(case["lwl1"]),
                                              *[_lib.dptr(a) for a in arrs], 1.0, _lib.dptr(fl_cor), _lib.dptr(X),
                                              ctypes.byref(status))
    assert (rc, status.value) == (0, 1)
    want_fl, want_X = oracle.optimize_calibration(case["lwl0"], case["lwl1"], case["lwl_cal"], case["fl_cal"],
                                                  case["fl_fixed"], A, Bm, Cm, order=order)
    got_fl, got_X = cov.optimize_calibration(case["lwl0"], case["lwl1"], case["lwl_cal"], case["fl_cal"], case["fl_fixed"],
                                             A, Bm, Cm, order=order)
    err = cr.errors((got_fl, got_X), cr.Cal(want_fl, want_X))
    assert all(err[k] <= TOL_ORACLE[k] for k in err), (err, TOL_ORACLE)
