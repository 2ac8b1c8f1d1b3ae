"""Latency of the gradient of the continuum-marginalised likelihood (psoap_chunk_lnlike_marg_grad) beside its two parents,
the plain gradient (psoap_chunk_lnlike_grad) and the marginal likelihood (psoap_chunk_lnlike_marg), and beside a plain
staged evaluation of the likelihood.

    python tools/marg_grad_latency.py [--sizes 2000 4096 6000] [--order 2] [--batches 1 8] [--reps 10] [--markdown profiles/x.md]

Per (N, B) with c = 2, 20 epochs and an additive baseline of the given order: ms per EVALUATION (per call / B) of the four on
the same handle in the same process -- host clock around the whole call, median of ``--reps`` after warm-up -- the ratios, and
the per-kernel split of one profiled call of the new entry (HIP events around every launch, a run of its own).  N is rounded
down to a multiple of the 20 epochs."""
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


def measure(N, order, batches, reps):
    N -= N % N_EPOCHS
    ch = syn.make_chunk(2, N_EPOCHS, N // N_EPOCHS, seed=8000 + N)
    gp = np.array(syn.GP_BASE[2])
    rows = []
    with ChunkHandle(ch.fl, ch.sigma, max_batch=max(batches)) as h:
        h.set_baseline(order, ch.lwl, ch.epoch_index, N_EPOCHS, 0.05 * 0.5 ** np.arange(order + 1))
        h.set_mode(0)          # the staged path for the plain evaluation
        for B in batches:
            lw, gps = np.stack([ch.lwls] * B), np.stack([gp] * B)
            ms = {"staged": _median_ms(lambda: h.lnlike_batch(lw, gps), reps) / B,
                  "grad": _median_ms(lambda: h.lnlike_grad(lw, gps), reps) / B,
                  "marg": _median_ms(lambda: h.lnlike_marg(lw, gps), reps) / B,
                  "marg_grad": _median_ms(lambda: h.lnlike_marg_grad(lw, gps), reps) / B}
            h.set_profiling(True)
            h.lnlike_marg_grad(lw, gps)
            split = h.timings()
            h.set_profiling(False)
            rows.append({"N": N, "B": B, "ms": ms, "split": split})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 4096, 6000])
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--markdown", help="write the table to this file as well")
    a = ap.parse_args()
    rows = [r for N in a.sizes for r in measure(N, a.order, a.batches, a.reps)]
    names = ("fill", "panel_update", "potrf", "trsm", "grad_contract", "misc")
    out = [f"library sha256 {build.library_sha256()}", "", f"order {a.order}, q = {N_EPOCHS * (a.order + 1)}, c = 2; ms per evaluation", "",
           "| N | B | staged lnlike | lnlike_grad | lnlike_marg | lnlike_marg_grad | marg_grad / grad | marg / staged |",
           "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        m = r["ms"]
        out.append(f"| {r['N']} | {r['B']} | {m['staged']:.2f} | {m['grad']:.2f} | {m['marg']:.2f} | {m['marg_grad']:.2f} | "
                   f"{m['marg_grad'] / m['grad']:.2f} | {m['marg'] / m['staged']:.2f} |")
    out += ["", "Per-kernel split of one profiled lnlike_marg_grad call (ms for the whole batch; launches; TFLOP/s of the executed MFMA "
            "flops; grad_contract is k_marg_gram + k_marg_grad_cross and k_marg_grad_contract; panel_update, potrf and trsm cover "
            "both [K | I | Ht] and [M | Xt]):", "",
            "| N | B | " + " | ".join(names) + " | sum of kernels | first to last event |", "|---|---|" + "---|" * (len(names) + 2)]
    for r in rows:
        cells = []
        for k in names:
            s = r["split"][k]
            rate = f", {s['flops'] / (s['ms'] * 1e-3) / 1e12:.1f}" if s["flops"] > 0 and s["ms"] > 0 else ""
            cells.append(f"{s['ms']:.3f} ({s['launches']}{rate})")
        out.append(f"| {r['N']} | {r['B']} | " + " | ".join(cells) +
                   f" | {sum(r['split'][k]['ms'] for k in names):.3f} | {r['split']['total_ms']:.3f} |")
    text = "\n".join(out)
    print(text)
    if a.markdown:
        with open(a.markdown, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
