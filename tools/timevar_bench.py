"""Device time of psoap_chunk_lnlike_tv_grad -- the value and the gradient under the time-variable kernel -- beside
psoap_chunk_lnlike_grad, the static call it extends, on the same handle in the same process.

    python tools/timevar_bench.py [--shapes sb2 st3] [--repeats 3]

Shapes and timing as tools/vel_newton_bench.py: SB2, N = 6000, 20 epochs; ST3, N = 8192, 16 epochs; one warm-up call, then
``--repeats`` calls with the handle's profiling on; the time of a call is psoap_chunk_get_timings' total_ms, the classes the
summed event times per kernel class of every call (and of the last one by itself).  tau = (0.25 x span, inf[, 2 x span]) of the chunk's dates; a third
measurement runs the new call at tau = inf throughout, where its outputs must have the bits of the static call.
One JSON line per shape on stdout.
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

SHAPES = {"sb2": (3, 0), "st3": (5, 0)}      # (cfg, chunk index) of synthetic.make_config_chunk


def run_shape(name: str, repeats: int) -> dict:
    from psoap_amd import build, synthetic as syn
    from psoap_amd.chunk import ChunkHandle
    ch = syn.make_config_chunk(*SHAPES[name])
    c, N = ch.n_components, ch.N
    gp = np.array(syn.GP_BASE[c])
    times = ch.dates[ch.epoch_index] - ch.dates.min()
    span = float(times.max())
    tau = (np.array([0.25, np.inf, 2.0]) * span)[:c]
    inf = np.full(c, np.inf)
    out = {"shape": name, "N": N, "c": c, "n_epochs": ch.n_epochs, "tau_days": [float(v) for v in tau],
           "library_sha256": build.library_sha256()}
    with ChunkHandle(ch.fl, ch.sigma) as h:
        h.set_times(times)
        h.set_profiling(True)
        res, last = {}, {}
        for what, call in (("lnlike_tv_grad", lambda: h.lnlike_tv_grad(ch.lwls, gp, tau, 1.0)),
                           ("lnlike_tv_grad_tau_inf", lambda: h.lnlike_tv_grad(ch.lwls, gp, inf, 1.0)),
                           ("lnlike_tv_value_only", lambda: (h.lnlike_tv(ch.lwls, gp, tau, 1.0),)),
                           ("lnlike_grad", lambda: h.lnlike_grad(ch.lwls, gp, 1.0))):
            first = call()                                   # warm-up: code objects, the workspace
            ms, classes = [], []
            for _ in range(repeats):
                again = call()
                t = h.timings()
                ms.append(t["total_ms"])
                classes.append({k: round(v["ms"], 3) for k, v in t.items() if isinstance(v, dict) and v["launches"]})
            assert all(np.array_equal(a, b) for a, b in zip(first, again)) and np.isfinite(first[0])
            res[what], last[what] = (float(np.median(ms)), [round(v, 3) for v in ms], classes), again
        for what, (med, all_ms, classes) in res.items():
            out[what + "_device_ms"] = all_ms
            out[what + "_device_ms_median"] = med
            out[what + "_classes_ms_last_call"] = classes[-1]
            out[what + "_classes_ms"] = {k: [cl.get(k) for cl in classes] for k in classes[-1]}      # every call's, per class
        out["ratio_tv_grad_over_lnlike_grad"] = res["lnlike_tv_grad"][0] / res["lnlike_grad"][0]
        out["ratio_tv_grad_tau_inf_over_lnlike_grad"] = res["lnlike_tv_grad_tau_inf"][0] / res["lnlike_grad"][0]
        a, b = last["lnlike_tv_grad_tau_inf"], last["lnlike_grad"]
        out["tau_inf_bits_equal_lnlike_grad"] = bool(all(np.array_equal(np.asarray(x), np.asarray(y))
                                                         for x, y in zip((a[0], a[1], a[3], a[4]), b)) and np.all(a[2] == 0.0))
        out["lnp_tv"], out["lnp_static"] = float(last["lnlike_tv_grad"][0]), float(b[0])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", nargs="+", default=["sb2", "st3"], choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args(argv)
    for name in args.shapes:
        print(json.dumps(run_shape(name, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
