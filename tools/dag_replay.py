"""Host replay of one launch of the persistent Cholesky kernel's throughput form (k_chol_dag, scheme 0) from its task
list: no GPU.  The list is psoap_dag_plan_sky's; the waits are the ones the kernel performs on that list (the edge rules of
tests/protocol_model.py's Model01, scheme 0); the costs come from a handful of constants fitted to the kernel's own per-task
stamps (tools/sky_phase_share.py prints them).

    python tools/dag_replay.py [--costs costs.json] [--workers 512] [--env NAME=VALUE ...]

replays the list of the headline batch (bench.py's: make_config_chunk(3), 32 walkers, seeds 3500 / 3501) and prints the
makespan, the worker time by phase and the idle share by cause.  --env builds the list in a child process under those
variables (the planner reads its experiment knobs once per process).

The simulation: every queue hands its tickets out in list order to whoever asks first; a queue's 64 home workers ask their
own queue until it is dry and then the others, starting at the queue their index picks, as k_chol_dag does.  A task holds
its worker from the draw to its end, its waits included.  A record flagged "owned" (the diagonal task behind the strip
solve of tile (q, q+1)) is run by the worker that ran that strip solve and skipped by whoever draws its ticket.  Every wait
targets a smaller ticket of the same queue, so a task's whole timeline is known when it is drawn.

What the model does not know: the two workgroups of a compute unit share one MFMA pipe, so a K-loop stage costs more
beside a K-loop than beside a strip solve or a wait -- `stage` is the fitted average of the measured launch; HBM and L2
contention of the partial tiles; clock and power.  profiles/sky_sched.md states how far the replayed span and phase shares
of the measured list lie from the measurement: a candidate's predicted gain counts only beyond that."""
from __future__ import annotations

import argparse
import ctypes
import heapq
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TASK = np.dtype([("type", "u1"), ("q", "u1"), ("j", "u1"), ("S", "u1"), ("b", "<u2"), ("pa", "u1"), ("pb", "u1"),
                 ("slot", "<u4"), ("ctr", "<u4")])
PART, DIAG, OFF = 0, 1, 2
TYPE_MASK, CHAIN, NOSOLVE, WAITNEXT, FUSED = 0x0F, 0x10, 0x20, 0x40, 0x80
CTR_MASK = 0x00FFFFFF
N_QUEUES = 8
GPT = 8          # 16-row stages per 128-row panel

# microseconds; the defaults are the fit of profiles/sky_sched.md (headline list, 512 workgroups)
DEFAULT_COSTS = {
    "stage": 3.54,        # one 16-row stage of a K-loop (16 x 128 x 128 MFMA work, staging included)
    "task": 0.0,          # fixed per task ahead of the K-loop (the fit's intercept)
    "fold": 11.1,         # per partial tile folded into the accumulators
    "store_final": 27.6,  # covariance on the fly + stores + drain of a final
    "store_part": 6.5,    # stores + drain + publish of a PART
    "solve": 30.0,        # strip solve + publish
    "potrf": 95.2,        # in-block Cholesky + publish
    "poll": 2.0,          # a waiter notices a publication this much after it (not fitted)
}
PHASES = ("kloop", "fold", "store_final", "store_part", "solve", "potrf", "task")
WAITS = ("wait_operands", "wait_partials", "wait_potrf", "wait_rows")


def plan_sky(B, P, first, workers=512, env=None):
    """psoap_dag_plan_sky's list: (tasks, n_slots, n_ctrs, queue_first).  env: built in a child process under these variables"""
    if env:
        code = ("import sys, json, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
                "import dag_replay as r\n"
                "t, s, c, qf = r.plan_sky(%d, %d, %r, %d)\n"
                "sys.stdout.buffer.write(json.dumps([s, c, qf]).encode() + b'\\n' + t.tobytes())\n"
                % (ROOT, os.path.dirname(os.path.abspath(__file__)), B, P, [int(v) for v in first], workers))
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, check=True).stdout
        head, _, body = out.partition(b"\n")
        s, c, qf = json.loads(head)
        return np.frombuffer(body, dtype=TASK).copy(), s, c, qf
    from psoap_amd import _lib
    L = _lib.load()
    f = (ctypes.c_int * P)(*[int(v) for v in first])
    n, slots, ctrs = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
    qf = (ctypes.c_uint32 * 9)()
    assert L.psoap_dag_plan_sky(B, P, f, workers, None, 0, ctypes.byref(n), ctypes.byref(slots), ctypes.byref(ctrs), qf) == 0
    tasks = np.zeros(n.value, dtype=TASK)
    assert L.psoap_dag_plan_sky(B, P, f, workers, tasks.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n),
                                ctypes.byref(slots), ctypes.byref(ctrs), qf) == 0
    return tasks, slots.value, ctrs.value, list(qf)


def bench_batch(B=32):
    """the headline batch of bench.py on one GPU: (chunk, lwls (B, c, N), gps (B, 2c))"""
    from psoap_amd import synthetic as syn
    ch = syn.make_config_chunk(3)
    gps = syn.make_walkers(ch.n_components, B, seed=3500)
    vels = syn.make_walker_velocities(ch, B, seed=3501)
    return ch, syn.walker_lwls(ch, vels), gps


def sky_envelopes(lwls, gps):
    """the host twins of the upload-side kernels: the union skyline first (P) of the winning order and every walker's own
    first 16-row group per column tile, first16 (B, P)"""
    from psoap_amd import _lib
    L = _lib.load()
    lwls = np.ascontiguousarray(lwls, dtype=np.float64)
    gps = np.ascontiguousarray(gps, dtype=np.float64)
    B, c, N = lwls.shape
    P = (N + 127) // 128
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    first = np.zeros(P, dtype=np.int32)
    assert L.psoap_sky_order(c, N, B, lwls.ctypes.data_as(dp), gps.ctypes.data_as(dp), first.ctypes.data_as(ip), None, None) == 0
    first16 = np.zeros((B, P), dtype=np.int32)
    assert L.psoap_sky_clip16(c, N, B, lwls.ctypes.data_as(dp), gps.ctypes.data_as(dp), first16.ctypes.data_as(ip), None, None) == 0
    return first, first16


def task_stages(tasks, first16=None):
    """16-row stages every task's K-loops run (dag_update: the panels before the last from max(128 pa, 16 ka16) on, the last
    panel whole or not at all); first16 None: nothing clipped"""
    pa, pb = tasks["pa"].astype(np.int64), tasks["pb"].astype(np.int64)
    ka = np.zeros(len(tasks), dtype=np.int64) if first16 is None else first16[tasks["b"], tasks["j"]].astype(np.int64)
    r0 = np.maximum(pa * GPT, ka)
    head = np.where(pb - pa > 1, np.maximum((pb - 1) * GPT - r0, 0), 0)
    last = np.where((pb > pa) & (r0 < pb * GPT), GPT, 0)
    return head, last


class Replay:
    """One simulated launch.  After run(): span, start / end per ticket (us), busy[phase], waited[cause], tail (worker time
    between a worker's last task and the end of the launch), workers."""

    def __init__(self, tasks, queue_first, costs=None, workers=512, first16=None):
        self.tasks, self.qf = tasks, [int(v) for v in queue_first]
        self.c = dict(DEFAULT_COSTS)
        self.c.update(costs or {})
        self.workers = workers
        self.head, self.last = task_stages(tasks, first16)
        self.kind = tasks["type"] & TYPE_MASK
        # PARTs per counter (a final gathers S - 1 of them), by queue: a counter index is the launch's
        self.part_tickets = {}
        for t in np.flatnonzero(self.kind == PART):
            self.part_tickets.setdefault(int(tasks["ctr"][t]), []).append(int(t))

    def run(self):
        tasks, c, kind = self.tasks, self.c, self.kind
        n = len(tasks)
        self.start, self.end = np.full(n, np.nan), np.full(n, np.nan)
        self.busy = {k: 0.0 for k in PHASES}
        self.waited = {k: 0.0 for k in WAITS}
        self.checked_waits = 0
        rvrow = {}           # (b, column tile, value) -> time the progress word reaches value
        potrf = {}           # (b, q) -> time potrf_done reaches q + 1
        row_left, row_done = {}, {}     # (b, q) -> finals still to count / time rows_done reaches q + 1
        P = int(tasks["q"].max()) + 1 if n else 0
        for t in np.flatnonzero(kind != PART):
            key = (int(tasks["b"][t]), int(tasks["q"][t]))
            row_left[key] = row_left.get(key, 0) + 1
        nxt = [0] * N_QUEUES
        size = [self.qf[g + 1] - self.qf[g] for g in range(N_QUEUES)]
        nonempty = [g for g in range(N_QUEUES) if size[g] > 0]
        # worker w: home queue w mod 8 (one per XCD), steals from the non-empty queue its index picks on
        heap = [(0.0, w) for w in range(self.workers)]
        heapq.heapify(heap)
        probe = [0] * self.workers
        dry = [0] * self.workers
        self.worker_end = [0.0] * self.workers

        def wait(now, t_flag, cause):
            """a wait whose publication comes at t_flag (a smaller ticket's: known)"""
            assert t_flag == t_flag, "a task waits for a ticket that has not been drawn"
            self.checked_waits += 1
            if t_flag <= now:
                return now
            self.waited[cause] += t_flag + c["poll"] - now
            return t_flag + c["poll"]

        def spend(now, phase, us):
            self.busy[phase] += us
            return now + us

        def run_task(t, now):
            k = tasks[t]
            b, q, j, pa, pb, S = int(k["b"]), int(k["q"]), int(k["j"]), int(k["pa"]), int(k["pb"]), int(k["S"])
            ty = int(kind[t])
            self.start[t] = now
            now = spend(now, "task", c["task"])
            if pb > pa:
                if pb - pa > 1:
                    now = wait(now, max(rvrow[(b, q, pb - 1)], rvrow[(b, j, pb - 1)]), "wait_operands")
                    now = spend(now, "kloop", c["stage"] * int(self.head[t]))
                now = wait(now, max(rvrow[(b, q, pb)], rvrow[(b, j, pb)]), "wait_operands")
                now = spend(now, "kloop", c["stage"] * int(self.last[t]))
            if ty == PART:
                now = spend(now, "store_part", c["store_part"])
                self.end[t] = now
                return now
            if S > 1:
                parts = self.part_tickets[int(k["ctr"]) & CTR_MASK]
                assert len(parts) == S - 1
                now = wait(now, max(self.end[p] for p in parts), "wait_partials")
                now = spend(now, "fold", c["fold"] * (S - 1))
            now = spend(now, "store_final", c["store_final"])
            if ty == DIAG:
                if q >= 3:
                    now = wait(now, row_done[(b, q - 3)], "wait_rows")
                now = spend(now, "potrf", c["potrf"])
                if q > 0:
                    now = max(now, potrf[(b, q - 1)])          # (published in order)
                potrf[(b, q)] = now
            else:
                now = wait(now, potrf[(b, q)], "wait_potrf")
                now = spend(now, "solve", c["solve"])
                rvrow[(b, j, q + 1)] = now
            self.end[t] = now
            row_left[(b, q)] -= 1
            if row_left[(b, q)] == 0:
                row_done[(b, q)] = max(now, row_done.get((b, q - 1), 0.0))
            return now

        while heap:
            now, w = heapq.heappop(heap)
            if dry[w] == (1 << N_QUEUES) - 1:
                self.worker_end[w] = now
                continue
            home = w % N_QUEUES
            g = home if probe[w] == 0 else (nonempty[w % len(nonempty)] + probe[w] - 1) % N_QUEUES if nonempty else home
            if dry[w] & (1 << g):
                probe[w] += 1
                heapq.heappush(heap, (now, w))
                continue
            if nxt[g] >= size[g]:
                dry[w] |= 1 << g
                probe[w] += 1
                heapq.heappush(heap, (now, w))
                continue
            t = self.qf[g] + nxt[g]
            nxt[g] += 1
            if kind[t] == DIAG and (tasks["type"][t] & NOSOLVE):
                heapq.heappush(heap, (now, w))               # owned: skipped by whoever draws its ticket
                continue
            now = run_task(t, now)
            if kind[t] == OFF and (tasks["type"][t] & FUSED):
                now = run_task(t + 1, now)                    # ... and run by the worker of the strip solve in front of it
            heapq.heappush(heap, (now, w))
        self.span = float(np.nanmax(self.end)) if n else 0.0
        self.tail = sum(self.span - e for e in self.worker_end)
        assert not np.isnan(self.end).any(), "a task never ran"
        return self

    def report(self):
        total = self.workers * self.span
        out = {"span_ms": self.span / 1e3, "tasks": int(len(self.tasks)), "parts": int((self.kind == PART).sum()),
               "stages": int(self.head.sum() + self.last.sum()), "workers": self.workers}
        for k, v in list(self.busy.items()) + list(self.waited.items()) + [("tail", self.tail)]:
            out[k + "_pct"] = 100.0 * v / total if total else 0.0
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--costs", help="JSON file of cost constants (tools/sky_phase_share.py writes one)")
    ap.add_argument("--workers", type=int, default=512)
    ap.add_argument("--walkers", type=int, default=32)
    ap.add_argument("--env", action="append", default=[], help="NAME=VALUE for the planner (repeatable)")
    args = ap.parse_args()
    costs = json.load(open(args.costs)) if args.costs else None
    ch, lwls, gps = bench_batch(args.walkers)
    first, first16 = sky_envelopes(lwls, gps)
    env = dict(kv.split("=", 1) for kv in args.env)
    tasks, _, _, qf = plan_sky(args.walkers, len(first), first, args.workers, env or None)
    print(json.dumps(Replay(tasks, qf, costs, args.workers, first16).run().report()))


if __name__ == "__main__":
    main()
