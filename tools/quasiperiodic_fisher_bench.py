"""Device time of psoap_chunk_fisher_qp and psoap_chunk_loo_qp -- the Fisher information and the leave-one-out under the
quasi-periodic kernel -- beside psoap_chunk_fisher_tv and psoap_chunk_loo_tv, the time-variable calls they extend and whose
code this build leaves as it was, on the same handle in the same process.

    python tools/quasiperiodic_fisher_bench.py [--shapes sb2 st3] [--repeats 3] [--tangents 4]

Shapes, hyper-parameters and timing as tools/quasiperiodic_bench.py: SB2, N = 6000; ST3, N = 8192; one warm-up call, then
``--repeats`` calls with the handle's profiling on; the time of a call is psoap_chunk_get_timings' total_ms, the classes the
summed event times per kernel class of every call.  T = 4 tangents: an amplitude, a mixed one, pure dGamma, pure dP.  The
measurements: ``fisher_tv`` (the yardstick, the same tangents without their Gamma and period parts), ``fisher_qp``, ``fisher_qp``
at Gamma = 0 (whose F must equal the yardstick's), ``fisher_tv`` once more; then ``loo_tv``, ``loo_qp``, ``loo_tv`` once more.

What must hold (``same_launches_hold``): PANEL_UPDATE, POTRF and TRSM are the same launches under both kernels, so the median
of each under the new calls lies within twice the yardstick's own spread over its ``--repeats`` calls (max - min of the first
measurement) of the yardstick's median.  FILL, GRAD, MISC and the total are reported as ratios to the yardstick, without a
threshold.  One JSON line per shape on stdout; the exit status is 1 where the rule does not hold for a shape.

As measured (profiles/quasiperiodic_fisher.md) the rule does NOT hold and the tool exits 1: PANEL_UPDATE under ``fisher_qp`` at
Gamma > 0 came out 0.26 - 0.35 % below the yardstick's median in three of four measurements, outside twice a spread of 0.016 -
0.041 ms, while at Gamma = 0 -- the yardstick's matrix -- it matched.  The launches are the same; the rule stands as it was set.
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
REPORTED = ("fill", "grad_contract", "misc")


def same_launches(per_call: dict, yardstick: str, new_calls) -> dict:
    """``per_call[measurement][class]``: the class's ms of every call of a measurement -> per class of SAME the yardstick's
    median and its spread (max - min) over its own calls, the medians of the new calls, and ``holds``: each of them within twice
    that spread of the yardstick's median"""
    out = {}
    for k in SAME:
        ref = per_call[yardstick][k]
        spread, median = max(ref) - min(ref), float(np.median(ref))
        row = {"yardstick_median_ms": median, "yardstick_spread_ms": round(spread, 3)}
        for what in new_calls:
            row[what + "_median_ms"] = float(np.median(per_call[what][k]))
        row["holds"] = bool(all(abs(row[what + "_median_ms"] - median) <= 2 * spread for what in new_calls))
        out[k] = row
    return out


def measure(h, calls, repeats):
    """every call of ``calls`` (name, callable, fields to compare between repeats): one warm-up, ``repeats`` timed calls"""
    res, last = {}, {}
    for what, call, same in calls:
        first = call()                                   # warm-up: code objects, the workspace
        ms, classes = [], []
        for _ in range(repeats):
            again = call()
            t = h.timings()
            ms.append(t["total_ms"])
            classes.append({k: round(v["ms"], 3) for k, v in t.items() if isinstance(v, dict) and v["launches"]})
        assert same(first, again)
        res[what], last[what] = (float(np.median(ms)), [round(v, 3) for v in ms], classes), again
    return res, last


def report(out, res, yardstick, new_calls):
    for what, (med, all_ms, classes) in res.items():
        out[what + "_device_ms"] = all_ms
        out[what + "_device_ms_median"] = med
        out[what + "_classes_ms_median"] = {k: float(np.median([cl.get(k, 0.0) for cl in classes])) for k in classes[-1]}
    med = lambda r, k: float(np.median([cl.get(k, 0.0) for cl in r[2]]))      # noqa: E731
    y = res[yardstick]
    for what in list(new_calls) + [yardstick + "_again"]:
        out[f"ratio_{what}_over_{yardstick}"] = res[what][0] / y[0]
        out[f"class_ratio_{what}_over_{yardstick}"] = {k: med(res[what], k) / med(y, k) for k in y[2][-1] if med(y, k) > 0}
    same = same_launches({what: {k: [cl.get(k, 0.0) for cl in r[2]] for k in SAME} for what, r in res.items()}, yardstick, new_calls)
    out["same_launches_" + yardstick] = same
    return bool(all(v["holds"] for v in same.values()))


def run_shape(name: str, repeats: int, T: int) -> dict:
    from psoap_amd import build, synthetic as syn
    from psoap_amd.chunk import ChunkHandle
    ch = syn.make_config_chunk(*SHAPES[name])
    c, N = ch.n_components, ch.N
    gp = np.array(syn.GP_BASE[c])
    times = ch.dates[ch.epoch_index] - ch.dates.min()
    span = float(times.max())
    tau = (np.array([0.25, np.inf, 2.0]) * span)[:c]
    gamma, period, zero = np.array([1.5, 0.8, 2.0])[:c], (np.array([0.23, 0.04, 1.7]) * span)[:c], np.zeros(c)
    tan_gp, tan_tau, tan_gamma, tan_period = np.zeros((T, 2 * c)), np.zeros((T, c)), np.zeros((T, c)), np.zeros((T, c))
    for t in range(T):
        kind = t % 4
        if kind == 0:
            tan_gp[t, 0] = 1.0
        elif kind == 1:
            tan_gp[t], tan_tau[t, 0], tan_gamma[t], tan_period[t] = 0.1 * gp, 0.1 * tau[0], 0.2, 0.05 * period
        elif kind == 2:
            tan_gamma[t, 0] = 1.0
        else:
            tan_period[t, 0] = 1.0
    ep = np.ascontiguousarray(ch.epoch_index, dtype=np.int32)
    out = {"shape": name, "N": N, "c": c, "T": T, "n_epochs": ch.n_epochs, "tau_days": [float(v) for v in tau],
           "gamma": [float(v) for v in gamma], "period_days": [float(v) for v in period], "library_sha256": build.library_sha256()}
    eq = lambda a, b: np.array_equal(np.asarray(a), np.asarray(b)) and bool(np.all(np.isfinite(a)))      # noqa: E731
    loo_eq = lambda a, b: a.lnp == b.lnp and np.array_equal(a.pix_logp, b.pix_logp) and np.isfinite(a.lnp)      # noqa: E731
    with ChunkHandle(ch.fl, ch.sigma) as h:
        h.set_times(times)
        h.set_profiling(True)
        tv = lambda: h.fisher_tv(ch.lwls, gp, tau, tan_gp, tan_tau)      # noqa: E731
        res, last = measure(h, (("fisher_tv", tv, eq),
                                ("fisher_qp", lambda: h.fisher_qp(ch.lwls, gp, tau, gamma, period, tan_gp, tan_tau, tan_gamma, tan_period), eq),
                                ("fisher_qp_gamma_0", lambda: h.fisher_qp(ch.lwls, gp, tau, zero, period, tan_gp, tan_tau, None, tan_period), eq),
                                ("fisher_tv_again", tv, eq)), repeats)
        hold = report(out, res, "fisher_tv", ("fisher_qp", "fisher_qp_gamma_0"))
        out["gamma_0_equals_fisher_tv"] = bool(np.array_equal(last["fisher_qp_gamma_0"], last["fisher_tv"]))
        h.fisher_release()
        ltv = lambda: h.loo_tv(ch.lwls, gp, tau, 1.0, ep, ch.n_epochs)      # noqa: E731
        res, last = measure(h, (("loo_tv", ltv, loo_eq),
                                ("loo_qp", lambda: h.loo_qp(ch.lwls, gp, tau, gamma, period, 1.0, ep, ch.n_epochs), loo_eq),
                                ("loo_tv_again", ltv, loo_eq)), repeats)
        hold = report(out, res, "loo_tv", ("loo_qp",)) and hold
    out["same_launches_hold"] = hold
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", nargs="+", default=["sb2", "st3"], choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tangents", type=int, default=4)
    args = ap.parse_args(argv)
    hold = True
    for name in args.shapes:
        out = run_shape(name, args.repeats, args.tangents)
        print(json.dumps(out), flush=True)
        hold = hold and out["same_launches_hold"]
    return 0 if hold else 1


if __name__ == "__main__":
    sys.exit(main())
