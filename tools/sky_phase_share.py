"""Where the worker time of the headline skyline launch goes, from the persistent kernel's per-task stamps, on the batch
bench.py measures (make_config_chunk(3), 32 walkers, seeds 3500 / 3501, both proposal sets): worker time by phase, the
dependency waits apart from the K-loops, idle worker time split into ramp, steady state and tail, and the same per block row.
Fits the cost constants of the host replay (tools/dag_replay.py) to the stamps, replays the same list and prints how far
the replayed span and phase shares lie from the measured ones.  tools/dag_phase_share.py is the same account for
replicated grids and dense lists.

    python tools/sky_phase_share.py [--out DIR]      (needs the GPU; DIR gets costs.json and the raw stamps of set 0)"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dag_replay as rp          # noqa: E402  (puts the repository root on sys.path)
from psoap_amd.chunk import ChunkHandle          # noqa: E402

PART, DIAG, OFF = rp.PART, rp.DIAG, rp.OFF


def stamps(h, lwls, gps):
    """one warm launch's list and stamps: (tasks, log (n, 8) in ticks of 10 ns)"""
    h.lnlike_batch(lwls, gps)
    h.lnlike_batch(lwls, gps)
    n = ctypes.c_longlong(0)
    h._L.psoap_chunk_dag_tasks(h._h, None, 0, ctypes.byref(n))
    nt = n.value
    tasks = np.zeros(nt, dtype=rp.TASK)
    h._L.psoap_chunk_dag_tasks(h._h, tasks.ctypes.data_as(ctypes.c_void_p), nt, ctypes.byref(n))
    log = np.zeros(nt * 8, dtype=np.uint64)
    h._L.psoap_chunk_dag_tasklog(h._h, log.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), nt)
    return tasks, log.reshape(nt, 8)


def account(tasks, log, workers):
    """the measured launch: phases in us of worker time, idle split, per block row"""
    ty = tasks["type"] & rp.TYPE_MASK
    us = log.astype(np.float64) / 100.0
    w7 = log[:, 7]
    waits = (w7 >> np.uint64(40)).astype(np.float64) / 100.0          # both waits of dag_update, added up
    ran = (log[:, 0] > 0) & (log[:, 3] > 0)
    t0 = us[ran, 0].min()
    s, e = us[:, 0] - t0, us[:, 3] - t0
    span = e[ran].max()
    part, diag, off = ran & (ty == PART), ran & (ty == DIAG), ran & (ty == OFF)
    fin = diag | off
    ph = {
        "kloop": (us[:, 5] - us[:, 0] - waits)[ran].sum(),
        "wait_operands": waits[ran].sum(),
        "wait_partials": (us[:, 6] - us[:, 5])[ran].sum(),
        "store_final": (us[:, 1] - us[:, 6])[fin].sum(),           # fold + covariance + stores + drain
        "store_part": (us[:, 3] - us[:, 6])[part].sum(),           # fold + stores + drain + publish
        "wait_potrf": (us[:, 2] - us[:, 1])[off].sum(),
        "solve": (us[:, 3] - us[:, 2])[off].sum(),
        "potrf": (us[:, 3] - us[:, 1])[diag].sum(),                # the wait for row q - 3 + in-block Cholesky + publish
    }
    task_time = (e - s)[ran].sum()
    idle = workers * span - task_time
    # tasks in flight over time -> ramp: until 90 % of the workers hold a task; tail: after the last such moment
    ev = np.concatenate([np.stack([s[ran], np.ones(ran.sum())], 1), np.stack([e[ran], -np.ones(ran.sum())], 1)])
    ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
    infl = np.cumsum(ev[:, 1])
    full = np.flatnonzero(infl >= 0.9 * workers)
    t_ramp, t_tail = (ev[full[0], 0], ev[full[-1], 0]) if len(full) else (span, span)

    def idle_in(a, b):
        if b <= a:
            return 0.0
        busy = (np.clip(e[ran], a, b) - np.clip(s[ran], a, b)).sum()
        return workers * (b - a) - busy

    # (a diagonal tile's tasks belong to the block row whose strip solve continues into them)
    row = np.where((tasks["q"] == tasks["j"]) & (tasks["q"] > 0), tasks["q"].astype(int) - 1, tasks["q"].astype(int))
    P = int(tasks["q"].max()) + 1
    starts = [float(np.median(s[ran & (row == q)])) if (ran & (row == q)).any() else span for q in range(P)] + [span]
    rows = []
    for q in range(P):
        m = ran & (row == q)
        rows.append({"q": q, "tasks": int(m.sum()), "parts": int((m & (ty == PART)).sum()),
                     "t_ms": starts[q] / 1e3, "task_ms": float((e - s)[m].sum() / 1e3),
                     "wait_ms": float((waits + (us[:, 6] - us[:, 5]) + np.where(ty == OFF, us[:, 2] - us[:, 1], 0.0))[m].sum() / 1e3),
                     "idle_ms": idle_in(starts[q], max(starts[q + 1], starts[q])) / 1e3})
    return {"span": span, "task_time": task_time, "idle": idle, "phases": ph,
            "idle_split": {"ramp": idle_in(0.0, t_ramp), "steady": idle_in(t_ramp, t_tail), "tail": idle_in(t_tail, span)},
            "t_ramp": t_ramp, "t_tail": t_tail, "rows": rows, "ran": ran, "s": s, "e": e, "us": us, "waits": waits}


def fit_costs(tasks, acc, first16):
    """the replay's constants from the stamps (medians: robust against the tasks that were descheduled)"""
    ty = tasks["type"] & rp.TYPE_MASK
    us, ran, waits = acc["us"], acc["ran"], acc["waits"]
    head, last = rp.task_stages(tasks, first16)
    stages = (head + last).astype(np.float64)
    kl = us[:, 5] - us[:, 0] - waits
    m = ran & (stages >= 16)
    # kloop = task + stage x stages: least squares over the tasks with a K-loop
    A = np.stack([np.ones(m.sum()), stages[m]], 1)
    fixed, stage = np.linalg.lstsq(A, kl[m], rcond=None)[0]
    S = tasks["S"].astype(int)
    fin, part, off, diag = ran & (ty != PART), ran & (ty == PART), ran & (ty == OFF), ran & (ty == DIAG)
    store1 = float(np.median((us[:, 1] - us[:, 6])[fin & (S == 1)])) if (fin & (S == 1)).any() else 30.0
    folds = fin & (S > 1)
    fold = float(np.median(((us[:, 1] - us[:, 6])[folds] - store1) / (S[folds] - 1))) if folds.any() else 5.5
    return {"stage": float(stage), "task": float(max(fixed, 0.0)), "fold": max(fold, 0.0), "store_final": store1,
            "store_part": float(np.median((us[:, 3] - us[:, 6])[part])) if part.any() else 12.0,
            "solve": float(np.median((us[:, 3] - us[:, 2])[off])), "potrf": float(np.median((us[:, 3] - us[:, 1])[diag])),
            "poll": rp.DEFAULT_COSTS["poll"]}


def worker_gaps(log, acc):
    """time between a worker's tasks (the ticket draw): workers told apart by XCD and HW_ID's low 16 bits"""
    ran = acc["ran"]
    key = ((log[:, 7] >> np.uint64(32)) & np.uint64(0xFF)) << np.uint64(16) | (log[:, 7] & np.uint64(0xFFFF))
    idx = np.flatnonzero(ran)
    order = idx[np.lexsort((acc["s"][idx], key[idx]))]
    same = key[order][1:] == key[order][:-1]
    gaps = (acc["s"][order][1:] - acc["e"][order][:-1])[same]
    return len(np.unique(key[idx])), gaps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--walkers", type=int, default=32)
    args = ap.parse_args()
    B = args.walkers
    ch, lwls_a, gps_a = rp.bench_batch(B)
    sets = [(lwls_a, gps_a), (np.roll(lwls_a, 1, axis=0).copy(), np.roll(gps_a, 1, axis=0).copy())]
    workers = 512
    with ChunkHandle(ch.fl, ch.sigma, max_batch=B) as h:
        h._L.psoap_chunk_dag_tasklog(h._h, None, 0)
        runs = [stamps(h, *s) for s in sets]
        stats = h.sky_stats()
    print("sky_stats:", json.dumps({k: (int(v) if isinstance(v, (int, np.integer)) else v) for k, v in stats.items()}, default=str))
    costs0 = None
    for k, (tasks, log) in enumerate(runs):
        first, first16 = rp.sky_envelopes(*sets[k])
        acc = account(tasks, log, workers)
        ty = tasks["type"] & rp.TYPE_MASK
        total = workers * acc["span"]
        print(f"\n== proposal set {k}: span {acc['span'] / 1e3:.3f} ms, {len(tasks)} tasks, {(ty == PART).sum()} PARTs, "
              f"{int((ty != PART).sum())} tiles; {workers} x span = {total / 1e3:.0f} ms of worker time")
        for name, v in acc["phases"].items():
            print(f"  {name:15s} {v / 1e3:9.1f} ms  {100 * v / total:5.1f} %")
        print(f"  {'no task held':15s} {acc['idle'] / 1e3:9.1f} ms  {100 * acc['idle'] / total:5.1f} %   "
              + "  ".join(f"{n} {v / 1e3:.1f} ms" for n, v in acc["idle_split"].items())
              + f"   (90 % of the workers hold a task from {acc['t_ramp'] / 1e3:.2f} to {acc['t_tail'] / 1e3:.2f} ms)")
        nw, gaps = worker_gaps(log, acc)
        if len(gaps):
            print(f"  {nw} workers seen; between two tasks of a worker: median {np.median(gaps):.1f} us, mean {gaps.mean():.1f} us, "
                  f"sum {gaps.sum() / 1e3:.1f} ms")
        print("  per block row: q tasks parts start_ms task_ms waits_ms idle_ms")
        for r in acc["rows"]:
            print(f"    {r['q']:3d} {r['tasks']:5d} {r['parts']:5d} {r['t_ms']:8.3f} {r['task_ms']:8.1f} {r['wait_ms']:8.1f} {r['idle_ms']:8.1f}")
        costs = fit_costs(tasks, acc, first16)
        print("  fitted costs (us):", json.dumps({n: round(v, 3) for n, v in costs.items()}))
        host_tasks, _, _, qf = rp.plan_sky(B, len(first), first, workers)
        same = host_tasks.tobytes() == tasks.tobytes()
        print(f"  the host's list for the host twin's envelope is the device's: {same}")
        sim = rp.Replay(tasks, qf, costs, workers, first16).run()
        rep = sim.report()
        print(f"  replay: span {rep['span_ms']:.3f} ms against {acc['span'] / 1e3:.3f} measured ({100 * (rep['span_ms'] * 1e3 / acc['span'] - 1):+.1f} %)")
        meas = {"kloop": acc["phases"]["kloop"], "wait_operands": acc["phases"]["wait_operands"],
                "wait_partials": acc["phases"]["wait_partials"], "wait_potrf": acc["phases"]["wait_potrf"],
                "solve": acc["phases"]["solve"], "potrf": acc["phases"]["potrf"], "store_part": acc["phases"]["store_part"],
                "store_final+fold": acc["phases"]["store_final"]}
        simv = {n: rep[n + "_pct"] for n in ("kloop", "wait_operands", "wait_partials", "wait_potrf", "solve", "store_part")}
        simv["potrf"] = rep["potrf_pct"] + rep["wait_rows_pct"]
        simv["store_final+fold"] = rep["store_final_pct"] + rep["fold_pct"]
        for n, v in meas.items():
            print(f"    {n:18s} measured {100 * v / total:5.1f} %   replayed {simv[n]:5.1f} %")
        print(f"    {'tail':18s} measured {100 * acc['idle_split']['tail'] / total:5.1f} %   replayed {rep['tail_pct']:5.1f} %")
        if k == 0:
            costs0 = costs
            if args.out:
                os.makedirs(args.out, exist_ok=True)
                json.dump(costs, open(os.path.join(args.out, "costs.json"), "w"), indent=1)
                np.savez_compressed(os.path.join(args.out, "stamps_set0.npz"), tasks=tasks, log=log, first=first, first16=first16,
                                    queue_first=np.array(qf))
    return costs0


if __name__ == "__main__":
    main()
