"""Time of the predict under the time-variable kernel (psoap_chunk_predict_tv) at the retrieve shape -- ST3, N = 8192, three
components on 1024 points each, one date -- beside the plain psoap_chunk_predict on the same handle in the same process.

    PSOAP_SHARE_POLICY=staged python tools/predict_timevar_bench.py      # the plain call on the staged route: the like-for-like
    python tools/predict_timevar_bench.py --plain-only                   # the plain call on the persistent launch, for scale

Per form one warm-up call, then ``--repeats`` calls; the figures are psoap_chunk_predict_timings' (device_ms: everything on
the device up to mu / Sigma complete; factor_ms: the fill and the sweep; sigma_ms: the mean, the prior fill and the
product; total_ms: the host's wall clock, the Sigma download included), the median of the repeats and their spread
(max - min).  The operation count says predict_tv / plain (staged) = 1: the launches behind the fill are identical.  One JSON
line per form on stdout.  PSOAP_SHARE_POLICY is read once per process: the two regimes are two runs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KEYS = ("device_ms", "factor_ms", "sigma_ms", "download_ms", "total_ms")


def measure(call, timings, repeats):
    call()
    rows = []
    for _ in range(repeats):
        call()
        rows.append(timings())
    out = {}
    for k in KEYS:
        v = sorted(r[k] for r in rows)
        out[k] = round(v[len(v) // 2], 3)
        out[k + "_spread"] = round(v[-1] - v[0], 3)
    out["gflops"] = round(rows[0]["flops"] / (out["device_ms"] * 1e-3) / 1e9, 1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    from psoap_amd import _lib, synthetic as syn
    from psoap_amd.chunk import ChunkHandle
    ch = syn.make_config_chunk(5, 0)                 # ST3: 3 components, 16 epochs x 512 pixels
    c, M = ch.n_components, args.points
    gp = list(syn.GP_BASE[c])
    pred = np.tile(np.linspace(ch.lwls[0].min(), ch.lwls[0].max(), M), (c, 1))
    times = ch.dates[ch.epoch_index] - ch.dates.min()
    span = float(times.max())
    t_pred = np.full(M, 0.4 * span)
    mus = [0.0] * c
    forms = {}
    with ChunkHandle(ch.fl, ch.sigma) as h:
        h.set_times(times)
        forms["plain"] = lambda: h.predict(0, ch.lwls, pred, mus, gp)
        if not args.plain_only:
            forms["tv-finite"] = lambda: h.predict_tv(0, ch.lwls, pred, t_pred, mus, gp, [0.25 * span, np.inf, 2.0 * span])
            forms["tv-inf"] = lambda: h.predict_tv(0, ch.lwls, pred, t_pred, mus, gp, [np.inf] * c)
        for name, call in forms.items():
            row = measure(call, h.predict_timings, args.repeats)
            stats = _lib.share_stats()
            print(json.dumps({"form": name, "N": ch.N, "c": c, "M": M, "policy": os.environ.get("PSOAP_SHARE_POLICY", "default"),
                              "dag_launches": stats["dag_launches"], **row}), flush=True)


if __name__ == "__main__":
    main()
