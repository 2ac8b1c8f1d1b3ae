"""Device time of psoap_chunk_lnlike_qp_grad -- the value and the gradient under the quasi-periodic kernel -- beside
psoap_chunk_lnlike_tv_grad, the time-variable call it extends and whose code this build leaves as it was, on the same handle
in the same process.

    python tools/quasiperiodic_bench.py [--shapes sb2 st3] [--repeats 3]

Shapes and timing as tools/marg_timevar_bench.py: SB2, N = 6000, 20 epochs; ST3, N = 8192, 16 epochs; one warm-up call, then
``--repeats`` calls with the handle's profiling on; the time of a call is psoap_chunk_get_timings' total_ms, the classes the
summed event times per kernel class of every call.  tau = (0.25 x span, inf[, 2 x span]) of the chunk's dates, Gamma =
(1.5, 0.8[, 2.0]), P = (0.23, 0.04[, 1.7]) x span.  Five measurements: the time-variable call (the yardstick), the new call,
the new call at Gamma = 0 (whose outputs must have the time-variable call's bits), the value-only call, and the time-variable
call once more at the end, so that a drift over the run shows as a difference between two measurements of the same call.

What must hold (``same_launches_hold``): PANEL_UPDATE, POTRF and TRSM are the same launches under both kernels, so the
median of each under the three new calls lies within twice the time-variable call's own spread over its ``--repeats`` calls
(max - min of the first measurement) of the time-variable call's median.  FILL, GRAD and the total are
reported.  One JSON line per shape on stdout; the exit status is 1 where the rule does not hold for a shape.
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
SAME = ("panel_update", "potrf", "trsm")      # the classes whose launches are the same under both kernels
NEW_CALLS = ("lnlike_qp_grad", "lnlike_qp_grad_gamma_0", "lnlike_qp_value_only")


def same_launches(per_call: dict) -> dict:
    """``per_call[measurement][class]``: the class's ms of every call of a measurement -> per class of SAME the time-variable
    call's median and its spread (max - min) over its own calls, the medians of the three new calls, and ``holds``: each of
    them within twice that spread of the time-variable median"""
    out = {}
    for k in SAME:
        ref = per_call["lnlike_tv_grad"][k]
        spread, median = max(ref) - min(ref), float(np.median(ref))
        row = {"tv_median_ms": median, "tv_spread_ms": round(spread, 3)}
        for what in NEW_CALLS:
            row[what + "_median_ms"] = float(np.median(per_call[what][k]))
        row["holds"] = bool(all(abs(row[what + "_median_ms"] - median) <= 2 * spread for what in NEW_CALLS))
        out[k] = row
    return out


def run_shape(name: str, repeats: int) -> dict:
    from psoap_amd import build, synthetic as syn
    from psoap_amd.chunk import ChunkHandle
    ch = syn.make_config_chunk(*SHAPES[name])
    c, N = ch.n_components, ch.N
    gp = np.array(syn.GP_BASE[c])
    times = ch.dates[ch.epoch_index] - ch.dates.min()
    span = float(times.max())
    tau = (np.array([0.25, np.inf, 2.0]) * span)[:c]
    gamma, period, zero = np.array([1.5, 0.8, 2.0])[:c], (np.array([0.23, 0.04, 1.7]) * span)[:c], np.zeros(c)
    out = {"shape": name, "N": N, "c": c, "n_epochs": ch.n_epochs, "tau_days": [float(v) for v in tau],
           "gamma": [float(v) for v in gamma], "period_days": [float(v) for v in period], "library_sha256": build.library_sha256()}
    with ChunkHandle(ch.fl, ch.sigma) as h:
        h.set_times(times)
        h.set_profiling(True)
        res, last = {}, {}
        for what, call in (("lnlike_tv_grad", lambda: h.lnlike_tv_grad(ch.lwls, gp, tau, 1.0)),
                           ("lnlike_qp_grad", lambda: h.lnlike_qp_grad(ch.lwls, gp, tau, gamma, period, 1.0)),
                           ("lnlike_qp_grad_gamma_0", lambda: h.lnlike_qp_grad(ch.lwls, gp, tau, zero, period, 1.0)),
                           ("lnlike_qp_value_only", lambda: (h.lnlike_qp(ch.lwls, gp, tau, gamma, period, 1.0),)),
                           ("lnlike_tv_grad_again", lambda: h.lnlike_tv_grad(ch.lwls, gp, tau, 1.0))):
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
            out[what + "_classes_ms"] = {k: [cl.get(k) for cl in classes] for k in classes[-1]}      # every call's, per class
            out[what + "_classes_ms_median"] = {k: float(np.median([cl.get(k, 0.0) for cl in classes])) for k in classes[-1]}
        tv, qp = res["lnlike_tv_grad"], res["lnlike_qp_grad"]
        out["ratio_qp_grad_over_tv_grad"] = qp[0] / tv[0]
        out["ratio_qp_grad_gamma_0_over_tv_grad"] = res["lnlike_qp_grad_gamma_0"][0] / tv[0]
        out["ratio_tv_grad_again_over_tv_grad"] = res["lnlike_tv_grad_again"][0] / tv[0]
        med = lambda r, k: float(np.median([cl.get(k, 0.0) for cl in r[2]]))      # noqa: E731
        out["class_ratio_qp_over_tv"] = {k: med(qp, k) / med(tv, k) for k in tv[2][-1] if med(tv, k) > 0}
        same = same_launches({what: {k: [cl.get(k, 0.0) for cl in r[2]] for k in SAME} for what, r in res.items()})
        out["same_launches"] = same
        out["same_launches_hold"] = bool(all(v["holds"] for v in same.values()))
        a, b = last["lnlike_qp_grad_gamma_0"], last["lnlike_tv_grad"]
        out["gamma_0_bits_equal_lnlike_tv_grad"] = bool(all(np.array_equal(np.asarray(x), np.asarray(y))
                                                            for x, y in zip((a[0], a[1], a[2], a[5], a[6]), b)) and np.all(a[4] == 0.0))
        out["value_only_bits_equal_the_gradient_calls_lnp"] = bool(last["lnlike_qp_value_only"][0] == last["lnlike_qp_grad"][0])
        out["lnp_qp"], out["lnp_tv"] = float(last["lnlike_qp_grad"][0]), float(b[0])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", nargs="+", default=["sb2", "st3"], choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args(argv)
    hold = True
    for name in args.shapes:
        out = run_shape(name, args.repeats)
        print(json.dumps(out), flush=True)
        hold = hold and out["same_launches_hold"]
    return 0 if hold else 1


if __name__ == "__main__":
    sys.exit(main())
