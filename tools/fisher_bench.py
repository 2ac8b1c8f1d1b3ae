"""Device time of the Fisher information (psoap_chunk_fisher) for SB2 with all 11 parameters as tangents.

    python tools/fisher_bench.py [--sizes 6000 2000] [--repeats 3] [--no-scipy]

Per size: one warm-up call, then ``--repeats`` calls of ``ChunkWorker.fisher_orbits`` with the handle's profiling on.  The
time of a call is the device time between the first and the last kernel of psoap_chunk_fisher by HIP events on the handle's
stream (psoap_chunk_get_timings: total_ms); the host's assembly of the (T, c, N) tangents and the copies in front are not in
it.  The rate is the algorithmic F_fisher(N, T) = (1 + 4 T) N^3 (psoap_amd/csrc/fisher_kernels.hpp) over that time, against the
78.6 TFLOP/s fp64 matrix peak of the MI355X.  Beside it: the rate of the three MFMA kernels alone (executed tile flops over
their summed event time, class ``grad_contract``), the same for k_grad_contract in one psoap_chunk_lnlike_grad call on the
same chunk, and at N = 2000 the float64 SciPy evaluation of tests/fisher_reference.py on this host's CPU.
One JSON line per size on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PEAK_FP64_TFLOPS = 78.6


def fisher_flops(N: int, T: int) -> float:
    return (1.0 + 4.0 * T) * float(N) ** 3


def run_size(N: int, repeats: int, scipy_too: bool) -> dict:
    from psoap_amd import build, synthetic as syn
    from psoap_amd.lnprob import ChunkWorker
    n_epochs = 10
    ch = syn.make_chunk(2, n_epochs, N // n_epochs, seed=8800 + N)
    assert ch.N == N
    p_orb, gp = np.array(syn.ORBIT_BASE["SB2"]), np.array(syn.GP_BASE[2])
    T = p_orb.shape[0] + gp.shape[0]
    w = ChunkWorker("SB2", ch.lwl, ch.fl, ch.sigma, ch.epoch_index, ch.dates)
    out = {"N": N, "T": T, "c": 2, "library_sha256": build.library_sha256()}
    try:
        h = w.handle
        h.set_profiling(True)
        F = w.fisher_orbits(p_orb, gp)                      # warm-up: code objects, the workspace
        calls, mfma_ms, mfma_flops, wall = [], [], [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            again = w.fisher_orbits(p_orb, gp)
            wall.append(time.perf_counter() - t0)
            t = h.timings()
            calls.append(t["total_ms"])
            mfma_ms.append(t["grad_contract"]["ms"])
            mfma_flops.append(t["grad_contract"]["flops"])
            classes = {k: round(v["ms"], 3) for k, v in t.items() if isinstance(v, dict) and v["launches"]}
        assert np.array_equal(F, again) and np.array_equal(F, F.T)
        keep = [i for i in range(T) if i != 6]              # gamma moves every grid alike: its row of F is zero up to rounding
        live = F[np.ix_(keep, keep)]
        out.update(device_ms=[round(v, 3) for v in calls], device_ms_median=float(np.median(calls)),
                   host_wall_ms=[round(1e3 * v, 1) for v in wall], classes_ms_last_call=classes,
                   flops_algorithmic=fisher_flops(N, T),
                   tflops=fisher_flops(N, T) / (np.median(calls) * 1e-3) / 1e12,
                   mfma_kernels_tflops=float(np.median(mfma_flops) / (np.median(mfma_ms) * 1e-3) / 1e12),
                   finite=bool(np.all(np.isfinite(F))), gamma_row_over_max_diag=float(np.max(np.abs(F[6])) / np.max(np.diag(F))),
                   min_eig_over_max_diag=float(np.min(np.linalg.eigvalsh(live)) / np.max(np.diag(live))))
        out["share_of_fp64_peak"] = out["tflops"] / PEAK_FP64_TFLOPS
        # the gradient's fused contraction on the same chunk: what the tile engine reaches in k_grad_contract
        vel = syn.make_walker_velocities(ch, 1, seed=8801)
        lw = syn.walker_lwls(ch, vel)
        h.lnlike_grad(lw[0], gp, 1.0)
        h.lnlike_grad(lw[0], gp, 1.0)
        g = h.timings()["grad_contract"]
        out["k_grad_contract_tflops"] = g["flops"] / (g["ms"] * 1e-3) / 1e12
        if scipy_too:
            import fisher_reference as fr
            from psoap_amd.orbit import velocity_jacobian
            vel, jac = velocity_jacobian("SB2", p_orb[None], ch.dates)
            ep = ch.epoch_index
            lwls = ch.lwl[None, :] + (-vel[0][:, ep]) / fr.C_KMS
            tan_lwl = np.zeros((T, 2, N))
            tan_lwl[:7] = -np.moveaxis(jac[0], 2, 0)[:, :, ep] / fr.C_KMS
            tan_gp = np.zeros((T, 4))
            tan_gp[7:] = np.eye(4)
            t0 = time.perf_counter()
            F64, _ = fr.fisher_f64(lwls, ch.sigma, gp, tan_lwl, tan_gp)
            out["scipy_f64_wall_ms"] = 1e3 * (time.perf_counter() - t0)
            out["scipy_cpus"] = len(os.sched_getaffinity(0))
            d = np.sqrt(np.diag(F64)[[i for i in range(T) if i != 6]])
            keep = [i for i in range(T) if i != 6]
            out["device_vs_scipy_rel"] = float(np.max(np.abs(F - F64)[np.ix_(keep, keep)] / np.outer(d, d)))
    finally:
        w.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[6000, 2000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args(argv)
    for N in args.sizes:
        print(json.dumps(run_size(N, args.repeats, (not args.no_scipy) and N <= 2000)), flush=True)


if __name__ == "__main__":
    main()
