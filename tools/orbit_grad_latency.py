"""Latency of the gradient of lnprob(p) on the device beside the same gradient assembled on the host.

    python tools/orbit_grad_latency.py [--sizes 2000 6000] [--batches 1 8] [--reps 20] [--markdown profiles/orbit_grad_latency.md]

Per N (SB2, c = 2, 20 epochs, the benchmark hyper-parameters) and batch size B, ms per call (host clock around the whole
call, median of ``--reps`` after 3 warm-up calls, same process, same handle):

* device: ``ChunkWorker.lnprob_grad_batch`` -- psoap_chunk_lnprob_grad: the orbit Jacobian, the Doppler shift, the
  likelihood's gradient, the epoch fold and the chain on the device; n_orb + 2c doubles up, 1 + n_orb + 2c + 1 down;
* host composition: what the same gradient took before that entry point existed -- ``orbit.velocities``
  (psoap_orbit_velocities), the host shift, ``ChunkHandle.lnlike_grad`` with the (B, c, N) ``grad_lwl`` downloaded,
  ``covariance.velocity_gradient`` and a NumPy Jacobian (the float64 formulas of tests/orbit_grad_reference.py).

``--profile-one`` runs ONE device call at N = --sizes[0], B = --batches[0] and nothing else: the process to put under
``rocprofv3 --kernel-trace --stats`` for the per-kernel split."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from psoap_amd import covariance, orbit, synthetic as syn  # noqa: E402
from psoap_amd.lnprob import ChunkWorker  # noqa: E402

MODEL, N_EPOCHS = "SB2", 20


def _median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def _setup(N, B):
    ch = syn.make_chunk(2, N_EPOCHS, N // N_EPOCHS, seed=8100 + N)
    P = syn.make_orbit_proposals(MODEL, B, seed=8200 + N)
    gps = syn.make_walkers(2, B, seed=8300 + N)
    return ch, np.concatenate([P, gps], axis=1)


def _host_composition(w, ch, ps):
    from orbit_grad_reference import jacobian_f64
    P, gps = ps[:, :7], ps[:, 7:]
    vel = orbit.velocities(MODEL, P, ch.dates)
    lw = ch.lwl + (-vel[:, :, ch.epoch_index]) / syn.C_KMS
    lnp, g_gp, g_lwl, _ = w.handle.lnlike_grad(lw, gps)
    g_v = covariance.velocity_gradient(g_lwl, ch.epoch_index, N_EPOCHS)
    g_orb = np.stack([np.einsum("ce,cek->k", g_v[b], np.asarray(jacobian_f64(MODEL, P[b], ch.dates)[0])) for b in range(len(P))])
    return lnp, np.concatenate([g_orb, g_gp], axis=1)


def measure(N, B, reps):
    ch, ps = _setup(N, B)
    w = ChunkWorker(MODEL, ch.lwl, ch.fl, ch.sigma, ch.epoch_index, ch.dates)
    try:
        dev = w.lnprob_grad_batch(ps)
        host = _host_composition(w, ch, ps)
        ms_dev = _median_ms(lambda: w.lnprob_grad_batch(ps), reps)
        ms_host = _median_ms(lambda: _host_composition(w, ch, ps), reps)
    finally:
        w.close()
    return {"N": N, "B": B, "device_ms": ms_dev, "host_ms": ms_host,
            "max_rel_diff": float(np.max(np.abs(dev[1] - host[1]) / np.max(np.abs(host[1]), axis=1, keepdims=True)))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 6000])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--markdown", help="write the table to this file as well")
    ap.add_argument("--profile-one", action="store_true")
    a = ap.parse_args()
    if a.profile_one:
        ch, ps = _setup(a.sizes[0], a.batches[0])
        w = ChunkWorker(MODEL, ch.lwl, ch.fl, ch.sigma, ch.epoch_index, ch.dates)
        print(w.lnprob_grad_batch(ps)[0])
        w.close()
        return
    out = ["| N | B | device: lnprob_grad_batch ms | host composition ms | host / device | largest difference of the two gradients / largest entry |",
           "|---|---|---|---|---|---|"]
    for N in a.sizes:
        for B in a.batches:
            r = measure(N, B, a.reps)
            out.append(f"| {N} | {B} | {r['device_ms']:.2f} | {r['host_ms']:.2f} | {r['host_ms'] / r['device_ms']:.2f} | {r['max_rel_diff']:.1e} |")
    text = "\n".join(out)
    print(text)
    if a.markdown:
        with open(a.markdown, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
