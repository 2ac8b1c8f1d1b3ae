"""Plain and marginal Fisher information (T = 8) and leave-one-out at the headline shape -- the benchmark's SB2 chunk, 20
epochs x 300 px (N = 6000), an additive baseline of order 2 -- with the two gradients beside them: the numbers of
profiles/marg_fisher.md.  One process, one handle; every entry ends in a stream synchronisation, so the host clock around a
call is the call.  Repeats are interleaved (one round runs every entry once) and the medians reported; then one profiled call
of each analysis entry gives the library's own per-class split.

    python tools/marg_fisher_latency.py [--reps 7] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from psoap_amd import synthetic as syn
from psoap_amd.chunk import ChunkHandle

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()
REPS = args.reps
ch = syn.make_chunk(2, 20, 300, seed=7)            # SB2, N = 6000: the benchmark's chunk shape
gp = np.array(syn.GP_BASE[2])
N, c, T = ch.N, 2, 8
rng = np.random.default_rng(1)
tan_gp = np.zeros((T, 2 * c))
tan_gp[:4] = np.eye(4)
tan_lwl = np.zeros((T, c, N))
tan_lwl[4:] = rng.standard_normal((4, c, N)) / 2.99792458e5
ep = np.asarray(ch.epoch_index)
out = {"N": N, "epochs": 20, "order": 2, "T": T, "reps": REPS}
with ChunkHandle(ch.fl, ch.sigma) as h:
    h.set_baseline(2, ch.lwl, ep, 20, [0.05, 0.025, 0.0125])
    calls = {
        "fisher": lambda: h.fisher(ch.lwls, gp, tan_gp, tan_lwl),
        "fisher_marg": lambda: h.fisher_marg(ch.lwls, gp, tan_gp, tan_lwl),
        "loo": lambda: h.loo(ch.lwls, gp, 0.9, ep, 20),
        "loo_marg": lambda: h.loo_marg(ch.lwls, gp, 0.9, ep, 20),
        "lnlike_grad": lambda: h.lnlike_grad(ch.lwls, gp, 0.9),
        "lnlike_marg_grad": lambda: h.lnlike_marg_grad(ch.lwls, gp, 0.9),
    }
    for f in calls.values():
        f()                                         # warm-up: allocation, code load
        f()
    times = {k: [] for k in calls}
    for _ in range(REPS):
        for k, f in calls.items():                  # interleaved
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    for k, v in times.items():
        out[k] = {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
    # where the time goes: the library's own per-class timings of one call each
    h.set_profiling(True)
    for k in ("fisher", "fisher_marg", "loo", "loo_marg"):
        calls[k]()
        t = h.timings()
        out[k]["classes_ms"] = {n: round(t[n]["ms"], 3) for n in t if n != "total_ms" and t[n]["launches"]}
        out[k]["total_ms"] = t["total_ms"]
    h.set_profiling(False)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
