"""Device time of the epoch-velocity Fisher information (psoap_chunk_fisher_vel) beside the generic psoap_chunk_fisher with 32
epoch-velocity tangents -- the most the generic call takes -- on the same chunk in the same process, and one
``lnprob.epoch_velocities`` fit over the 8 chunks of cfg4.

    python tools/vel_fisher_bench.py [--shapes sb2 st3] [--repeats 3] [--no-fit]

Shapes: SB2, N = 6000, 20 epochs (c E = 40); ST3, N = 8192, 16 epochs (c E = 48).  Per shape: one warm-up call, then
``--repeats`` calls with the handle's profiling on.  The time of a call is the device time between its first and its last
kernel by HIP events on the handle's stream (psoap_chunk_get_timings: total_ms), the classes are the summed event times per
kernel class.  The rate is the algorithmic (1 + 2 c + c (c + 1)) N^3 -- the factorisation of [K | I] and K^-1, N^3, and the
products (psoap_amd/csrc/vel_fisher_kernels.hpp) -- over that time; the generic call's is (1 + 4 T) N^3.  Also: how many
128 x 128 tiles of Dv_c are exactly zero (what a later pull request could skip).
The fit: 8 chunks of the cfg4 shape with shared dates and velocities, the flux of each drawn from the model itself, started
1 km/s off the truth; iterations and wall time.  One JSON line per measurement on stdout.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PEAK_FP64_TFLOPS = 78.6
SHAPES = {"sb2": (3, 0), "st3": (5, 0)}      # (cfg, chunk index) of synthetic.make_config_chunk


def zero_tiles(ch, gp):
    """(exactly-zero tiles, all tiles) of Dv_c summed over the components: a tile is zero when every pair (m, n) in it is of
    one epoch or has exp(p_c d^2) = +0 (p_c d^2 <= -746)"""
    NB = 128
    N, ep = ch.N, ch.epoch_index
    P = (N + NB - 1) // NB
    zero = 0
    for k in range(ch.n_components):
        p = -0.5 * 2.99792458e5 ** 2 / gp[2 * k + 1] ** 2
        x = ch.lwls[k]
        for ti in range(P):
            xi, ei = x[ti * NB:(ti + 1) * NB], ep[ti * NB:(ti + 1) * NB]
            for tj in range(P):
                xj, ej = x[tj * NB:(tj + 1) * NB], ep[tj * NB:(tj + 1) * NB]
                d = xj[None, :] - xi[:, None]
                live = (ei[:, None] != ej[None, :]) & (p * d * d > -746.0)
                zero += not live.any()
    return zero, ch.n_components * P * P


def run_shape(name: str, repeats: int) -> dict:
    import vel_fisher_reference as vr
    from psoap_amd import build, synthetic as syn
    from psoap_amd.chunk import ChunkHandle
    ch = syn.make_config_chunk(*SHAPES[name])
    c, E, N = ch.n_components, ch.n_epochs, ch.N
    gp = np.array(syn.GP_BASE[c])
    tan_lwl, tan_gp = vr.epoch_tangents(c, N, ch.epoch_index, E)
    out = {"shape": name, "N": N, "c": c, "n_epochs": E, "cE": c * E, "library_sha256": build.library_sha256()}
    with ChunkHandle(ch.fl, ch.sigma) as h:
        h.set_profiling(True)
        res = {}
        for what, call in (("vel", lambda: h.fisher_vel(ch.lwls, gp, ch.epoch_index, E)),
                           ("generic32", lambda: h.fisher(ch.lwls, gp, tan_gp[:32], tan_lwl[:32]))):
            F = call()                                       # warm-up: code objects, the workspace
            ms, classes = [], {}
            for _ in range(repeats):
                again = call()
                t = h.timings()
                ms.append(t["total_ms"])
                classes = {k: round(v["ms"], 3) for k, v in t.items() if isinstance(v, dict) and v["launches"]}
            assert np.array_equal(F, again) and np.array_equal(F, F.T) and np.all(np.isfinite(F))
            res[what] = (F, float(np.median(ms)), [round(v, 3) for v in ms], classes)
        Fv, Fg = res["vel"][0], res["generic32"][0]
        d = np.sqrt(np.diag(Fv)[:32])
        flops_vel = (1.0 + 2 * c + c * (c + 1)) * float(N) ** 3
        flops_gen = (1.0 + 4 * 32) * float(N) ** 3
        z, n = zero_tiles(ch, gp)
        out.update(vel_device_ms=res["vel"][2], vel_device_ms_median=res["vel"][1], vel_classes_ms_last_call=res["vel"][3],
                   generic32_device_ms=res["generic32"][2], generic32_device_ms_median=res["generic32"][1],
                   generic32_classes_ms_last_call=res["generic32"][3], ratio_generic32_over_vel=res["generic32"][1] / res["vel"][1],
                   vel_tflops=flops_vel / (res["vel"][1] * 1e-3) / 1e12, generic32_tflops=flops_gen / (res["generic32"][1] * 1e-3) / 1e12,
                   vel_vs_generic32_rel=float(np.max(np.abs(Fv[:32, :32] - Fg) / np.outer(d, d))),
                   dv_zero_tiles=z, dv_tiles=n)
        out["vel_share_of_fp64_peak"] = out["vel_tflops"] / PEAK_FP64_TFLOPS
    return out


def run_fit(method: str = "scoring") -> dict:
    """the 8-chunk cfg4 fit; ``method`` goes to lnprob.epoch_velocities (tools/vel_newton_bench.py runs both)"""
    import oracle
    from psoap_amd import lnprob, synthetic as syn
    from psoap_amd.utils import registered_params
    gp = np.array(syn.GP_BASE[2])
    first = syn.make_config_chunk(4, 0)
    full = dict(zip(registered_params["SB2"], list(syn.ORBIT_BASE["SB2"]) + list(gp)))
    workers = []
    t0 = time.perf_counter()
    for k in range(8):
        ch = syn.make_config_chunk(4, k)
        lwls = syn.replicate_wls(ch.lwl, first.velocities, ch.mask)
        K = np.empty((ch.N, ch.N))
        oracle.fill_sym(K, np.ascontiguousarray(lwls), gp)
        K[np.diag_indices_from(K)] += ch.sigma ** 2
        fl = 1.0 + np.linalg.cholesky(K) @ np.random.default_rng(4100 + k).standard_normal(ch.N)
        ch = dataclasses.replace(ch, fl=fl)
        workers.append(lnprob.ChunkWorker("SB2", ch.lwl, ch.fl, ch.sigma, ch.epoch_index, first.dates, defaults=full))
    setup = time.perf_counter() - t0
    d = np.random.default_rng(4200).standard_normal(first.velocities.shape)
    d -= d.mean(axis=1, keepdims=True)
    d /= np.max(np.abs(d))
    p = np.array([full[n] for n in registered_params["SB2"]])
    try:
        t0 = time.perf_counter()
        res = lnprob.epoch_velocities(workers, p, vel0=first.velocities + d, method=method)
        wall = time.perf_counter() - t0
    finally:
        for w in workers:
            w.close()
    return {"fit": "cfg4, 8 chunks, N = 6000 each, 20 epochs", "host_setup_s": round(setup, 1), "wall_s": round(wall, 2),
            "n_iter": res.n_iter, "converged": bool(res.converged), "decrement": res.decrement, "lnp_start": res.lnp_start,
            "lnp": res.lnp, "sigma_kms_min_max": [float(np.nanmin(res.sigma)), float(np.nanmax(res.sigma))],
            "max_abs_v_minus_truth_over_sigma": float(np.nanmax(np.abs(res.vel - first.velocities) / res.sigma))}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", nargs="+", default=["sb2", "st3"], choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-fit", action="store_true")
    args = ap.parse_args(argv)
    for name in args.shapes:
        print(json.dumps(run_shape(name, args.repeats)), flush=True)
    if not args.no_fit:
        print(json.dumps(run_fit()), flush=True)


if __name__ == "__main__":
    main()
