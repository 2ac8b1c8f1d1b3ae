"""Latency of the continuum-marginalised likelihood beside the likelihood's gradient (psoap_chunk_lnlike_marg against
psoap_chunk_lnlike_grad), its nearest staged neighbour: the gradient carries N appended columns through the factorisation,
the marginal likelihood q = n_epochs (order + 1).

    python tools/marg_latency.py [--sizes 2000 6000] [--orders 1 3] [--batches 1 8] [--reps 10] [--markdown profiles/x.md]

Per (N, order, B) with c = 2 and 20 epochs, the benchmark hyper-parameters and an additive baseline: ms per EVALUATION
(per call / B) of both entry points on the same handle in the same process -- host clock around the whole call, median of
``--reps`` after warm-up -- their ratio, and the per-kernel split of one profiled marginal call (HIP events around every
launch, a run of its own)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from psoap_amd import build, synthetic as syn  # noqa: E402
from psoap_amd.chunk import ChunkHandle  # noqa: E402

N_EPOCHS = 20


def _median_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def measure(N, orders, batches, reps):
    if N % N_EPOCHS:
        raise SystemExit(f"N = {N} is not a multiple of {N_EPOCHS} epochs")
    ch = syn.make_chunk(2, N_EPOCHS, N // N_EPOCHS, seed=8000 + N)
    gp = np.array(syn.GP_BASE[2])
    rows = []
    with ChunkHandle(ch.fl, ch.sigma, max_batch=max(batches)) as h:
        for B in batches:
            lw, gps = np.stack([ch.lwls] * B), np.stack([gp] * B)
            ms_grad = _median_ms(lambda: h.lnlike_grad(lw, gps), reps) / B
            for order in orders:
                h.set_baseline(order, ch.lwl, ch.epoch_index, N_EPOCHS, 0.05 * 0.5 ** np.arange(order + 1))
                ms_marg = _median_ms(lambda: h.lnlike_marg(lw, gps), reps) / B
                ms_all = _median_ms(lambda: h.lnlike_marg(lw, gps, want_beta=True, want_cov=True, want_flux=True), reps) / B
                h.set_profiling(True)
                h.lnlike_marg(lw, gps)
                split = h.timings()
                h.set_profiling(False)
                rows.append({"N": N, "order": order, "B": B, "grad_ms": ms_grad, "marg_ms": ms_marg, "marg_all_ms": ms_all,
                             "split": split})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 6000])
    ap.add_argument("--orders", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--markdown", help="write the table to this file as well")
    a = ap.parse_args()
    rows = [r for N in a.sizes for r in measure(N, a.orders, a.batches, a.reps)]
    names = ("fill", "panel_update", "potrf", "trsm", "grad_contract", "misc")
    out = [f"library sha256 {build.library_sha256()}", "",
           "| N | order | q | B | lnlike_grad ms / evaluation | lnlike_marg ms / evaluation | marg / grad | with beta, covariance and "
           "flux ms / evaluation |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['N']} | {r['order']} | {N_EPOCHS * (r['order'] + 1)} | {r['B']} | {r['grad_ms']:.2f} | {r['marg_ms']:.2f} | "
                   f"{r['marg_ms'] / r['grad_ms']:.2f} | {r['marg_all_ms']:.2f} |")
    out += ["", "Per-kernel split of one profiled marginal call (ms for the whole batch; launches; TFLOP/s of the executed MFMA "
            "flops; grad_contract is the Gram kernel):", "",
            "| N | order | B | " + " | ".join(names) + " | sum of kernels | first to last event |", "|---|---|---|" + "---|" * (len(names) + 2)]
    for r in rows:
        cells = []
        for k in names:
            s = r["split"][k]
            rate = f", {s['flops'] / (s['ms'] * 1e-3) / 1e12:.1f}" if s["flops"] > 0 and s["ms"] > 0 else ""
            cells.append(f"{s['ms']:.3f} ({s['launches']}{rate})")
        out.append(f"| {r['N']} | {r['order']} | {r['B']} | " + " | ".join(cells) +
                   f" | {sum(r['split'][k]['ms'] for k in names):.3f} | {r['split']['total_ms']:.3f} |")
    text = "\n".join(out)
    print(text)
    if a.markdown:
        with open(a.markdown, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
