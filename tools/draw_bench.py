"""What posterior draws cost on the device against NumPy on the host: the numbers of profiles/predict_draw.md.

    python tools/draw_bench.py [--rounds 5] [--no-host] [--out FILE]

At the retrieve shape (ST3, N = 8192, 3 x 1024 prediction pixels, R = 3072) and at SB2 with R = 2 x 600 (N = 6000), for
D in {5, 32, 1024}: after one ``ChunkHandle.predict`` with Sigma, ``predict_draw(D, seed)`` with the library's profiling on --
device ms of copy + factorisation (classes fill, panel_update, potrf, trsm), of the normals (misc) and of the triangular
product (grad_contract), median of the rounds after two warm-up calls, and the wall clock of the whole call; then the wall
clock of ``np.random.multivariate_normal(mu, Sigma, size=D)`` on the downloaded Sigma on the same machine (one call: its SVD
takes seconds).  One JSON line per (shape, D).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from psoap_amd import build, synthetic as syn  # noqa: E402
from psoap_amd.chunk import ChunkHandle  # noqa: E402

SHAPES = {"ST3 N=8192 R=3x1024": (5, 1024), "SB2 N=6000 R=2x600": (3, 600)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [json.dumps({"library_sha256": build.library_sha256()})]
    for name, (cfg, M) in SHAPES.items():
        ch = syn.make_config_chunk(cfg)
        c = ch.n_components
        pred = np.linspace(np.min(ch.lwls[0]), np.max(ch.lwls[0]), num=M)
        with ChunkHandle(ch.fl, ch.sigma, max_batch=1) as h:
            mu, Sigma = h.predict(0, ch.lwls, np.stack([pred] * c), np.zeros(c), syn.GP_BASE[c])
            h.set_profiling(True)
            for D in (5, 32, 1024):
                rows, wall = [], []
                for r in range(a.rounds + 2):
                    t0 = time.perf_counter()
                    h.predict_draw(D, seed=r)
                    t1 = time.perf_counter()
                    t = h.timings()
                    if r >= 2:
                        rows.append(t)
                        wall.append(1e3 * (t1 - t0))
                med = lambda f: float(np.median([f(t) for t in rows]))      # noqa: E731
                rec = {"shape": name, "R": int(mu.shape[0]), "D": D, "rounds": a.rounds,
                       "copy_factor_ms": med(lambda t: sum(t[k]["ms"] for k in ("fill", "panel_update", "potrf", "trsm"))),
                       "copy_ms": med(lambda t: t["fill"]["ms"]), "normals_ms": med(lambda t: t["misc"]["ms"]),
                       "product_ms": med(lambda t: t["grad_contract"]["ms"]), "device_total_ms": med(lambda t: t["total_ms"]),
                       "call_wall_ms": float(np.median(wall))}
                if not a.no_host:
                    t0 = time.perf_counter()
                    np.random.default_rng(0).multivariate_normal(mu, Sigma, size=D)
                    rec["numpy_host_ms"] = 1e3 * (time.perf_counter() - t0)
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
            h.set_profiling(False)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
