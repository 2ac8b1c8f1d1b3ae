"""Timings of the time scales at the ``lnprob(p)`` boundary on one MI355X (profiles/timevar_sampling.md).

Two shapes: SB2 N = 6000 with B = 32 proposals, ST3 N = 8192 with B = 16.  Per shape, one warm-up call of every route and then
three timed calls of each, the routes alternating inside one process in an order that rotates from round to round; a call is timed by a host clock around work that ends in
``fetch`` (a device synchronisation).  Medians and the spread (max - min) of the three are printed, one JSON line per shape:

1. ``tv``      upload_orbits + set_tau + eval + fetch on a ``ChunkWorker(timevar=...)`` at finite time scales;
   ``static``  the same upload without time scales under ``set_mode("staged")``, same build; ``ratio_tv_static`` their medians;
   ``tv_dag``  the ``tv`` call with the handle in the persistent mode (not what a timevar worker does: its handle is in staged
   mode), where the upload also queues the skyline's sort and envelope kernels that a staged evaluation never reads;
2. ``host_tv`` what was the only way to these values before: ``lnlike_tv`` (psoap_chunk_lnlike_tv_grad, value only) on grids
   shifted on the host, the velocities from ``orbit.velocities`` -- the whole call, shift included; evals/s per proposal of
   both routes and their ratio.

    python tools/timevar_sampling_bench.py [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from psoap_amd import synthetic as syn  # noqa: E402
from psoap_amd.lnprob import ChunkWorker  # noqa: E402

SHAPES = (("SB2", 3, 32), ("ST3", 5, 16))          # (model, synthetic config, B)
REPEATS = 3


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def measure(model, cfg, B, only=None):
    ch = syn.make_config_chunk(cfg)
    c = ch.n_components
    dates = np.asarray(ch.dates, dtype=np.float64)
    span = float(dates.max() - dates.min())
    p_orb = syn.make_orbit_proposals(model, B, seed=100 + cfg)
    gp = syn.make_walkers(c, B, seed=200 + cfg)
    tau = span * (0.3 + 0.05 * np.arange(B)[:, None] + 0.2 * np.arange(c)[None, :])
    tv = ChunkWorker(model, ch.lwl, ch.fl, ch.sigma, ch.epoch_index, dates, max_batch=B,
                     timevar={"fit": [True] * c, "tau": [np.inf] * c})
    static = ChunkWorker(model, ch.lwl, ch.fl, ch.sigma, ch.epoch_index, dates, max_batch=B)
    static.handle.set_mode("staged")

    def route_tv():
        tv.upload_orbits(p_orb, gp, 1.0, tau)
        tv.handle.eval()
        return tv.handle.fetch()

    def route_static():
        static.upload_orbits(p_orb, gp, 1.0)
        static.handle.eval()
        return static.handle.fetch()

    def route_host_tv():
        lwls, fast = tv.shifted_grids(p_orb)
        out = tv.handle.lnlike_tv(lwls, gp, tau, 1.0)
        out[fast] = -np.inf
        return out

    def route_tv_dag():          # the same call with the handle left in the persistent mode: the upload then queues the skyline kernels
        tv.handle.set_mode("dag")
        try:
            return route_tv()
        finally:
            tv.handle.set_mode("staged")

    routes = {"tv": route_tv, "static": route_static, "tv_dag": route_tv_dag, "host_tv": route_host_tv}
    if only:
        routes = {k: routes[k] for k in only}
    try:
        values = {k: fn() for k, fn in routes.items()}          # warm-up: one call of every route
        ms = {k: [] for k in routes}
        names = list(routes)
        for r in range(REPEATS):
            # (the order rotates: what a call follows -- the 0.7 s host_tv call above all -- is shared out among the routes)
            for k in names[r % len(names):] + names[:r % len(names)]:
                ms[k].append(timed(routes[k])[0])
    finally:
        tv.close()
        static.close()
    row = {"model": model, "N": int(ch.N), "B": B}
    if "tv" in values and "host_tv" in values:
        row["tv_vs_host_tv_max_rel"] = float(np.max(np.abs(values["tv"] - values["host_tv"]) /
                                                    np.maximum(1.0, np.abs(values["host_tv"]))))
    for k, v in ms.items():
        row[k + "_ms"] = {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "calls": [round(x, 3) for x in v]}
    if "tv" in ms and "static" in ms:
        row["ratio_tv_static"] = row["tv_ms"]["median"] / row["static_ms"]["median"]
    if "tv" in ms and "host_tv" in ms:
        row["evals_per_s_per_proposal"] = {k: B / (row[k + "_ms"]["median"] * 1e-3) for k in ("tv", "host_tv")}
        row["speedup_over_host_tv"] = row["host_tv_ms"]["median"] / row["tv_ms"]["median"]
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--routes", default=None, help="comma-separated subset of tv,static,tv_dag,host_tv (a kernel trace of two)")
    args = ap.parse_args(argv)
    for model, cfg, B in SHAPES:
        line = json.dumps(measure(model, cfg, B, args.routes.split(",") if args.routes else None))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
