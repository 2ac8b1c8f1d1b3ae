"""Device time of psoap_chunk_info_vel -- value, gradient, F and the observed information J from one factorisation -- beside the
two calls an iteration of the scoring fit makes, psoap_chunk_fisher_vel + psoap_chunk_lnlike_grad, on the same chunk in the
same process, and the ``lnprob.epoch_velocities`` fit over the 8 chunks of cfg4 under both methods.

    python tools/vel_newton_bench.py [--shapes sb2 st3] [--repeats 3] [--no-fit]

Shapes and timing as tools/vel_fisher_bench.py: SB2, N = 6000, 20 epochs; ST3, N = 8192, 16 epochs; one warm-up call, then
``--repeats`` calls with the handle's profiling on; the time of a call is psoap_chunk_get_timings' total_ms, the classes the
summed event times per kernel class of the last call (the pair pass is booked under FILL, V = G U and U^T V under GRAD).
One JSON line per measurement on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import vel_fisher_bench as vb  # noqa: E402


def run_shape(name: str, repeats: int) -> dict:
    from psoap_amd import build, synthetic as syn
    from psoap_amd.chunk import ChunkHandle
    ch = syn.make_config_chunk(*vb.SHAPES[name])
    c, E, N = ch.n_components, ch.n_epochs, ch.N
    gp = np.array(syn.GP_BASE[c])
    out = {"shape": name, "N": N, "c": c, "n_epochs": E, "cE": c * E, "library_sha256": build.library_sha256()}
    with ChunkHandle(ch.fl, ch.sigma) as h:
        h.set_profiling(True)
        res = {}
        for what, call in (("info_vel", lambda: h.info_vel(ch.lwls, gp, ch.epoch_index, E)[3]),
                           ("fisher_vel", lambda: h.fisher_vel(ch.lwls, gp, ch.epoch_index, E)),
                           ("lnlike_grad", lambda: h.lnlike_grad(ch.lwls, gp, 1.0)[2])):
            first = call()                                   # warm-up: code objects, the workspace
            ms, classes = [], {}
            for _ in range(repeats):
                again = call()
                t = h.timings()
                ms.append(t["total_ms"])
                classes = {k: round(v["ms"], 3) for k, v in t.items() if isinstance(v, dict) and v["launches"]}
            assert np.array_equal(first, again) and np.all(np.isfinite(first))
            res[what] = (float(np.median(ms)), [round(v, 3) for v in ms], classes)
        old = res["fisher_vel"][0] + res["lnlike_grad"][0]
        for what, (med, all_ms, classes) in res.items():
            out[what + "_device_ms"] = all_ms
            out[what + "_device_ms_median"] = med
            out[what + "_classes_ms_last_call"] = classes
        out["ratio_info_vel_over_the_two_calls"] = res["info_vel"][0] / old
    return out


def run_fits() -> list:
    """vel_fisher_bench.run_fit, once per method (it builds its workers and closes them)"""
    rows = []
    for method in ("scoring", "newton"):
        t0 = time.perf_counter()
        row = vb.run_fit(method)
        row["method"], row["total_s"] = method, round(time.perf_counter() - t0, 1)
        rows.append(row)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", nargs="+", default=["sb2", "st3"], choices=sorted(vb.SHAPES))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-fit", action="store_true")
    args = ap.parse_args(argv)
    for name in args.shapes:
        print(json.dumps(run_shape(name, args.repeats)), flush=True)
    if not args.no_fit:
        for row in run_fits():
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
