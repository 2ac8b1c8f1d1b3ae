"""The envelopes tests/test_sky_split.py, tests/test_gpu_sky_split.py and tests/golden/make_sky_split_parent.py share: the
three batches of the skyline GPU tests at N = 1250 (padded last tile) and N = 1280 (exact tiles), B = 16, and the headline
batch of bench.py (P = 47, B = 32), and a synthetic band at P = 16."""
import hashlib
import os
import sys

import numpy as np

from test_sky_order import gpu_case, sky_order
from test_sky_plan import plan_dense, plan_sky

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import dag_replay          # noqa: E402

WORKERS = 512
GPU_B = 16
GPU_CASES = [(name, n) for name in ("narrow_odd", "three", "wide") for n in (1250, 1280)]


def gpu_batch(name, n):
    """(fl, sigma, lwl, gps) of one of the three envelope cases at N = n"""
    if name == "narrow_odd":          # the odd walkers' length scales x 0.3: the case with emptied PART ranges
        fl, sigma, lwl, gps = gpu_case(2, 320, N=n)
        gps[1::2, 1::2] *= 0.3
        return fl, sigma, lwl, gps
    if name == "three":
        return gpu_case(3, 308, N=n)
    assert name == "wide"             # length scales x 4: every column on its clamp
    return gpu_case(2, 320, scale=4.0, N=n)


# a band of 14 tiles at P = 16: the smallest shape at which both kinds of split act -- a diagonal tile's pre-accumulation in
# two parts (clipped span >= 12) and strips in up to eight pieces -- and the happens-before checker still takes seconds
MID_B, MID_P = 16, 16
MID_FIRST = [max(j - 13, 0) for j in range(MID_P)]

_envelopes = {}


def envelope(name, n):
    """the union skyline of a case: first (P)"""
    if (name, n) not in _envelopes:
        _, _, lwl, gps = gpu_batch(name, n)
        _envelopes[(name, n)] = [int(v) for v in sky_order(lwl, gps)[0]]
    return _envelopes[(name, n)]


def headline():
    """(first (47), first16 (32, 47)) of the batch bench.py measures"""
    if "headline" not in _envelopes:
        _, lwls, gps = dag_replay.bench_batch(32)
        first, first16 = dag_replay.sky_envelopes(lwls, gps)
        _envelopes["headline"] = ([int(v) for v in first], first16)
    return _envelopes["headline"]


def list_cases():
    """(key, B, P, first) of every skyline list the host test looks at"""
    out = [(f"{name}_{n}", GPU_B, len(envelope(name, n)), envelope(name, n)) for name, n in GPU_CASES]
    out.append(("headline", 32, 47, headline()[0]))
    out.append(("mid_band", MID_B, MID_P, MID_FIRST))
    return out


def digest(plan):
    """sha256 over a plan_sky / plan_dense result: the task records, the counts and the queues' first tickets"""
    tasks, n_slots, n_ctrs, qf = plan
    h = hashlib.sha256(tasks.tobytes())
    h.update(repr((int(n_slots), int(n_ctrs), [int(v) for v in qf])).encode())
    return h.hexdigest()


def parent_digests():
    """what tests/golden/sky_split_parent_v1.json records: per case the envelope and the digests of its skyline list and
    of the dense list of the same (B, P)"""
    out = {}
    for key, B, P, first in list_cases():
        out[key] = {"B": B, "P": P, "first": first, "sky": digest(plan_sky(B, P, first, WORKERS)),
                    "dense": digest(plan_dense(B, P, WORKERS))}
    return out
