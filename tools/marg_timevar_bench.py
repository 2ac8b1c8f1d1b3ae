"""Device time of psoap_chunk_lnlike_marg_tv_grad -- the value and the gradient under the time-variable kernel with the
per-epoch continuum integrated out -- beside psoap_chunk_lnlike_marg_grad, the static marginal call it extends, on the same
handle in the same process.

    python tools/marg_timevar_bench.py [--shapes sb2 st3] [--repeats 3]

Shapes and timing as tools/timevar_bench.py: SB2, N = 6000, 20 epochs; ST3, N = 8192, 16 epochs; an order-1 baseline (prior
standard deviations 0.05, 0.025, no weights); one warm-up call, then ``--repeats`` calls with the handle's profiling on; the
time of a call is psoap_chunk_get_timings' total_ms, the classes the summed event times per kernel class of every call.
tau = (0.25 x span, inf[, 2 x span]) of the chunk's dates; a third measurement runs the new call at tau = inf throughout,
where its outputs must have the bits of the static marginal call; a fourth the value-only call; and the static marginal call
once more at the end, so that a drift over the run shows as a difference between two measurements of the same call.  One JSON
line per shape on stdout.
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


def _value_only(h, lwls, gp, tau):
    """psoap_chunk_lnlike_marg_tv_grad with grad_gp == NULL: the gradient entry's value-only call"""
    from psoap_amd._lib import check, dptr
    lw, g, t, lnp = (np.ascontiguousarray(a, dtype=np.float64) for a in (lwls, gp, tau, np.empty(1)))
    check(h._L.psoap_chunk_lnlike_marg_tv_grad(h._h, 1, lw.shape[0], dptr(lw), dptr(g), dptr(t), 1.0, dptr(lnp), None, None, None,
                                               None, None), "psoap_chunk_lnlike_marg_tv_grad")
    return float(lnp[0])


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
        h.set_baseline(1, ch.lwl, ch.epoch_index, ch.n_epochs, [0.05, 0.025])
        h.set_profiling(True)
        res, last = {}, {}
        for what, call in (("lnlike_marg_grad", lambda: h.lnlike_marg_grad(ch.lwls, gp, 1.0)),
                           ("lnlike_marg_tv_grad", lambda: h.lnlike_marg_tv_grad(ch.lwls, gp, tau, 1.0)),
                           ("lnlike_marg_tv_grad_tau_inf", lambda: h.lnlike_marg_tv_grad(ch.lwls, gp, inf, 1.0)),
                           ("lnlike_marg_tv_value_only", lambda: (_value_only(h, ch.lwls, gp, tau),)),
                           ("lnlike_marg_grad_again", lambda: h.lnlike_marg_grad(ch.lwls, gp, 1.0))):
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
        out["ratio_marg_tv_grad_over_marg_grad"] = res["lnlike_marg_tv_grad"][0] / res["lnlike_marg_grad"][0]
        out["ratio_marg_tv_grad_tau_inf_over_marg_grad"] = res["lnlike_marg_tv_grad_tau_inf"][0] / res["lnlike_marg_grad"][0]
        a, b = last["lnlike_marg_tv_grad_tau_inf"], last["lnlike_marg_grad"]
        out["tau_inf_bits_equal_lnlike_marg_grad"] = bool(all(np.array_equal(np.asarray(x), np.asarray(y))
                                                              for x, y in zip((a[0], a[1], a[3], a[4]), b)) and np.all(a[2] == 0.0))
        out["value_only_bits_equal_the_gradient_calls_lnp"] = bool(last["lnlike_marg_tv_value_only"][0] == last["lnlike_marg_tv_grad"][0])
        out["lnp_marg_tv"], out["lnp_marg_static"] = float(last["lnlike_marg_tv_grad"][0]), float(b[0])
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
