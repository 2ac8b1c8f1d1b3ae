"""Device time of leave-one-out cross-validation (psoap_chunk_loo) on the cfg3 chunk (SB2, 20 epochs) at N = 6000 and 2000.

    python tools/loo_bench.py [--sizes 6000 2000] [--repeats 3]

Per size: one warm-up call, then ``--repeats`` calls of ``ChunkHandle.loo`` with the epoch index and the handle's profiling
on.  The time of a call is the device time between the first and the last kernel of psoap_chunk_loo by HIP events on the
handle's stream (psoap_chunk_get_timings: total_ms); the host's layout of the packed blocks and the copies in front are not in
it.  Beside it, in the same process on the same chunk: one psoap_chunk_lnlike_grad call, which shares the factorisation of
[K | I] -- class by class, so that what the call costs beyond the shared factorisation can be read off (the packed blocks go
through the same panel_update / potrf / trsm classes) -- and the band kernel's executed tile flops over its event time (class
``grad_contract``, which holds nothing else in a loo call).  One JSON line per size on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FP64_TFLOPS = 78.6
NB = 128


def band_tiles(epoch_index, N):
    """the tile list of psoap_amd/csrc/loo_plan.hpp: (all upper tiles, band tiles)"""
    P = (N + NB - 1) // NB
    ep = np.asarray(epoch_index)
    tiles = set()
    for e in np.unique(ep):
        idx = np.flatnonzero(ep == e)
        t0, t1 = idx[0] // NB, idx[-1] // NB
        tiles |= {(ti, tj) for ti in range(t0, t1 + 1) for tj in range(ti, t1 + 1)}
    return P * (P + 1) // 2, len(tiles)


def classes(t):
    return {k: round(v["ms"], 3) for k, v in t.items() if isinstance(v, dict) and v["launches"]}


def run_size(N: int, repeats: int) -> dict:
    from psoap_amd import build, synthetic as syn
    from psoap_amd.chunk import ChunkHandle
    c, n_epochs, _ = syn.CONFIG_SHAPES[3]
    ch = syn.make_chunk(c, n_epochs, N // n_epochs, seed=3000)
    assert ch.N == N
    gp = np.array(syn.GP_BASE[c])
    ep = ch.epoch_index
    upper, band = band_tiles(ep, N)
    out = {"N": N, "c": c, "n_epochs": n_epochs, "pixels_per_epoch": N // n_epochs, "upper_tiles": upper, "band_tiles": band,
           "library_sha256": build.library_sha256()}
    with ChunkHandle(ch.fl, ch.sigma) as h:
        h.set_profiling(True)
        first = h.loo(ch.lwls, gp, 1.0, ep, n_epochs)                  # warm-up: code objects, the workspace
        calls, wall, band_ms, band_flops = [], [], [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            again = h.loo(ch.lwls, gp, 1.0, ep, n_epochs)
            wall.append(time.perf_counter() - t0)
            t = h.timings()
            calls.append(t["total_ms"])
            band_ms.append(t["grad_contract"]["ms"])
            band_flops.append(t["grad_contract"]["flops"])
            loo_classes = classes(t)
        same = all(np.array_equal(getattr(first, f), getattr(again, f))
                   for f in ("pix_mean", "pix_var", "pix_logp", "ep_resid", "ep_chi2", "ep_logp", "ep_npix"))
        h.lnlike_grad(ch.lwls, gp, 1.0)
        lnp = h.lnlike_grad(ch.lwls, gp, 1.0)[0]
        g = h.timings()
        grad_classes = classes(g)
        t0 = time.perf_counter()
        pixels = h.loo(ch.lwls, gp, 1.0)
        pix_wall = time.perf_counter() - t0
        pix_ms = h.timings()["total_ms"]
    shared = sum(grad_classes.get(k, 0.0) for k in ("fill", "panel_update", "potrf", "trsm"))
    out.update(device_ms=[round(v, 3) for v in calls], device_ms_median=float(np.median(calls)),
               host_wall_ms=[round(1e3 * v, 1) for v in wall], classes_ms_last_call=loo_classes,
               lnlike_grad_device_ms=round(g["total_ms"], 3), lnlike_grad_classes_ms=grad_classes,
               shared_factorisation_ms=round(shared, 3), beyond_shared_factorisation_ms=round(float(np.median(calls)) - shared, 3),
               blocks_ms={k: round(loo_classes.get(k, 0.0) - grad_classes.get(k, 0.0), 3) for k in ("panel_update", "potrf", "trsm")},
               band_ms=float(np.median(band_ms)), band_flops=float(np.median(band_flops)),
               band_tflops=float(np.median(band_flops) / (np.median(band_ms) * 1e-3) / 1e12),
               pixels_only_device_ms=round(pix_ms, 3), pixels_only_wall_ms=round(1e3 * pix_wall, 1),
               bits_repeat=bool(same), lnp_is_lnlike_grads=bool(first.lnp == lnp),
               pixel_bits_without_epochs=bool(np.array_equal(first.pix_logp, pixels.pix_logp)),
               max_abs_pix_z=float(np.max(np.abs(first.pix_z))), loo_logp=first.loo_logp, lnp=first.lnp)
    out["band_share_of_fp64_peak"] = out["band_tflops"] / PEAK_FP64_TFLOPS
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[6000, 2000])
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args(argv)
    for N in args.sizes:
        print(json.dumps(run_size(N, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
