"""Latency of the likelihood's gradient beside the likelihood itself (psoap_chunk_lnlike_grad against psoap_lnlike).

    python tools/grad_latency.py [--sizes 2000 4096 6000] [--reps 20] [--markdown profiles/grad_latency.md]

Per N (c = 2, B = 1, the benchmark hyper-parameters): ms per call of both entry points, timed in the same process
(host clock around the whole call, median of ``--reps`` after warm-up), the gradient's per-kernel split from the handle's
profiling mode (HIP events around every launch, a run of its own: profiling serialises nothing here, the gradient is one
stream, but the events cost a little), and the achieved fp64 rate against F_grad(N) = N^3 -- factorisation, triangular
solve and contraction at N^3/3 each."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from psoap_amd import synthetic as syn  # noqa: E402
from psoap_amd.chunk import ChunkHandle  # noqa: E402

PEAK_TFLOPS = 78.6          # MI355X fp64 matrix peak, as bench.py states it


def _chunk(N):
    for ne in (10, 16, 20, 25, 32):
        if N % ne == 0:
            return syn.make_chunk(2, ne, N // ne, seed=8000 + N)
    raise SystemExit(f"N = {N}: no epoch count among 10, 16, 20, 25, 32 divides it")


def _median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def measure(N, reps):
    ch, gp = _chunk(N), np.array(syn.GP_BASE[2])
    with ChunkHandle(ch.fl, ch.sigma) as h:
        ms_val = _median_ms(lambda: h.lnlike(ch.lwls, gp), reps)
        ms_grad = _median_ms(lambda: h.lnlike_grad(ch.lwls, gp), reps)
        h.set_mode("staged")
        ms_staged = _median_ms(lambda: h.lnlike(ch.lwls, gp), reps)
        h.set_mode("dag")
        h.set_profiling(True)
        h.lnlike_grad(ch.lwls, gp)
        split = h.timings()
        h.set_profiling(False)
    return {"N": N, "lnlike_ms": ms_val, "staged_ms": ms_staged, "grad_ms": ms_grad, "split": split,
            "tflops": N ** 3 / (ms_grad * 1e-3) / 1e12}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 4096, 6000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--markdown", help="write the table to this file as well")
    a = ap.parse_args()
    rows = [measure(N, a.reps) for N in a.sizes]
    names = ("fill", "panel_update", "potrf", "trsm", "grad_contract", "misc")
    out = ["| N | psoap_lnlike (persistent) ms | psoap_lnlike (staged) ms | gradient ms | gradient / persistent | gradient / staged | "
           "TFLOP/s at N^3 | of 78.6 |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['N']} | {r['lnlike_ms']:.2f} | {r['staged_ms']:.2f} | {r['grad_ms']:.2f} | {r['grad_ms'] / r['lnlike_ms']:.2f} | "
                   f"{r['grad_ms'] / r['staged_ms']:.2f} | {r['tflops']:.1f} | {r['tflops'] / PEAK_TFLOPS:.3f} |")
    out += ["", "Per-kernel split of one profiled gradient call (ms; launches; TFLOP/s of the executed MFMA flops):", "",
            "| N | " + " | ".join(names) + " | sum of kernels | first to last event |", "|---|" + "---|" * (len(names) + 2)]
    for r in rows:
        cells = []
        for k in names:
            s = r["split"][k]
            rate = f", {s['flops'] / (s['ms'] * 1e-3) / 1e12:.1f}" if s["flops"] > 0 and s["ms"] > 0 else ""
            cells.append(f"{s['ms']:.3f} ({s['launches']}{rate})")
        out.append(f"| {r['N']} | " + " | ".join(cells) + f" | {sum(r['split'][k]['ms'] for k in names):.3f} | {r['split']['total_ms']:.3f} |")
    text = "\n".join(out)
    print(text)
    if a.markdown:
        with open(a.markdown, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
