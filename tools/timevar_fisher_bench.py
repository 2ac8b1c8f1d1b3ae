"""Time of the Fisher information and the leave-one-out under the time-variable kernel (psoap_chunk_fisher_tv,
psoap_chunk_loo_tv) at the benchmark's shape -- SB2, N = 6000 -- beside the static psoap_chunk_fisher and psoap_chunk_loo on the
same handle in the same process.

    python tools/timevar_fisher_bench.py

``fisher`` with T = 4 (the hyper-parameter unit tangents) against ``fisher_tv`` with T = 4 (amp_0, l_0, tau_0 and a velocity
tangent), with a finite tau and with every tau = inf; ``loo`` against ``loo_tv`` with the chunk's 20 epochs.  Per form one
warm-up call, then ``--repeats`` calls: the host's wall clock of the call and the per-bracket device times of
psoap_chunk_get_timings, the median of the repeats and their spread (max - min).  The static call's code is untouched by
the time-variable one, so it is the yardstick: the operation count says the ratio is 1 -- one multiply-add more per element
in one fill and one epilogue, under 4 T N^3 flops of products.  One JSON line per form on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def measure(call, timings, repeats):
    call()
    rows = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        t = timings()
        rows.append({"wall_ms": wall, "device_ms": t["total_ms"], **{k: v["ms"] for k, v in t.items() if isinstance(v, dict) and v["launches"]}})
    out = {}
    for k in rows[0]:
        v = sorted(r[k] for r in rows)
        out[k] = round(v[len(v) // 2], 3)
        out[k + "_spread"] = round(v[-1] - v[0], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--config", type=int, default=3, help="synthetic.CONFIG_SHAPES (3: SB2, N = 6000, 20 epochs)")
    args = ap.parse_args()
    from psoap_amd import synthetic as syn
    from psoap_amd.chunk import ChunkHandle
    ch = syn.make_config_chunk(args.config, 0)
    c, N = ch.n_components, ch.N
    gp = np.array(syn.GP_BASE[c], dtype=np.float64)
    times = ch.dates[ch.epoch_index] - ch.dates.min()
    span = float(times.max())
    finite, inf = np.array([0.25 * span] + [np.inf] * (c - 1)), np.full(c, np.inf)
    T = 4
    tan_gp, tan_tau, tan_lwl = np.zeros((T, 2 * c)), np.zeros((T, c)), np.zeros((T, c, N))
    tan_gp[0, 0] = tan_gp[1, 1] = 1.0
    tan_tau[2, 0] = 1.0
    tan_lwl[3, 0, ch.epoch_index == 0] = -1.0 / syn.C_KMS
    static_gp = np.eye(2 * c)[:T]
    ep, ne = ch.epoch_index, ch.n_epochs
    with ChunkHandle(ch.fl, ch.sigma) as h:
        h.set_times(times)
        h.set_profiling(True)
        forms = {"fisher": lambda: h.fisher(ch.lwls, gp, static_gp),
                 "fisher_tv-finite": lambda: h.fisher_tv(ch.lwls, gp, finite, tan_gp, tan_tau, tan_lwl),
                 "fisher_tv-inf": lambda: h.fisher_tv(ch.lwls, gp, inf, tan_gp, tan_tau, tan_lwl),
                 "fisher-again": lambda: h.fisher(ch.lwls, gp, static_gp),
                 "loo": lambda: h.loo(ch.lwls, gp, 1.0, ep, ne),
                 "loo_tv-finite": lambda: h.loo_tv(ch.lwls, gp, finite, 1.0, ep, ne),
                 "loo_tv-inf": lambda: h.loo_tv(ch.lwls, gp, inf, 1.0, ep, ne),
                 "loo-again": lambda: h.loo(ch.lwls, gp, 1.0, ep, ne)}
        for name, call in forms.items():
            row = measure(call, h.timings, args.repeats)
            print(json.dumps({"form": name, "N": N, "c": c, "T": T if "fisher" in name else None,
                              "epochs": None if "fisher" in name else ne, **row}), flush=True)


if __name__ == "__main__":
    main()
