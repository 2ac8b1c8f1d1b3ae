"""What marginalising the component spectra over chain samples costs on the device against the route a user had before:
the numbers of profiles/predict_mixture.md.

    python tools/mix_latency.py [--rounds 3] [--samples 64] [--out FILE]

At the retrieve shape (ST3, N = 8192, 3 x 1024 prediction pixels, R = 3072), S samples with the benchmark hyper-parameters
jittered by 3 % and the velocities by 0.2 km/s.  Every round runs both routes one after the other on one handle:

* device: ``mix_begin``, S x ``mix_add``, ``mix_finish`` -- per add the wall clock, the plain predict's own ``device_ms``
  (``predict_timings``) and, with the library's profiling on, the device time of the fold beyond it (class fill: Sbar += w Sigma
  and the row store); the finish's wall clock and its device time (misc: mean and centring; grad_contract: the rank-S product);
* host: S x ``predict`` with ``Sigma`` downloaded, ``Sbar += w Sigma`` and the means stacked in NumPy as they arrive, then the
  moments (a NumPy GEMM for the between term).

One warm-up round, then the median and the range over the rounds; one JSON line per route and one with the largest
difference between the two results."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from psoap_amd import build, synthetic as syn  # noqa: E402
from psoap_amd.chunk import ChunkHandle  # noqa: E402


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--pixels", type=int, default=1024)
    ap.add_argument("--config", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S, M = a.samples, a.pixels
    ch = syn.make_config_chunk(a.config)
    c = ch.n_components
    rng = np.random.default_rng(5)
    lwls = syn.walker_lwls(ch, syn.make_walker_velocities(ch, S, seed=6))
    gps = np.array(syn.GP_BASE[c]) * (1.0 + 0.03 * rng.standard_normal((S, 2 * c)))
    w = rng.uniform(0.5, 2.0, S)
    pred = np.stack([np.linspace(np.min(ch.lwls[0]), np.max(ch.lwls[0]), num=M)] * c)
    mus = np.zeros(c)
    R = c * M
    lines = [json.dumps({"library_sha256": build.library_sha256(), "N": ch.N, "c": c, "M": M, "R": R, "S": S, "rounds": a.rounds})]
    dev, host = [], []
    with ChunkHandle(ch.fl, ch.sigma, max_batch=1) as h:
        for r in range(a.rounds + 1):
            # ---- device route
            h.set_profiling(True)
            t0 = time.perf_counter()
            h.mix_begin(0, pred, mus, S)
            t_begin = time.perf_counter() - t0
            add_wall, fold_ms, pred_ms = [], [], []
            for s in range(S):
                t0 = time.perf_counter()
                h.mix_add(lwls[s], gps[s], w[s])
                add_wall.append(1e3 * (time.perf_counter() - t0))
                fold_ms.append(h.timings()["fill"]["ms"])
                pred_ms.append(h.predict_timings()["device_ms"])
            t0 = time.perf_counter()
            got = h.mix_finish()
            fin_wall = 1e3 * (time.perf_counter() - t0)
            t = h.timings()
            h.set_profiling(False)
            rec_d = {"begin_ms": 1e3 * t_begin, "add_wall_ms": float(np.median(add_wall)), "add_fold_device_ms": float(np.median(fold_ms)),
                     "add_predict_device_ms": float(np.median(pred_ms)), "adds_wall_ms": float(np.sum(add_wall)), "finish_wall_ms": fin_wall,
                     "finish_center_device_ms": t["misc"]["ms"], "finish_syrk_device_ms": t["grad_contract"]["ms"],
                     "total_wall_ms": 1e3 * t_begin + float(np.sum(add_wall)) + fin_wall}
            # ---- host route: what a user could do before
            t_all = time.perf_counter()
            Sbar, Mu = np.zeros((R, R)), np.empty((S, R))
            call_wall, dl_ms = [], []
            for s in range(S):
                t0 = time.perf_counter()
                mu_s, Sig_s = h.predict(0, lwls[s], pred, mus, gps[s])
                call_wall.append(1e3 * (time.perf_counter() - t0))
                dl_ms.append(h.predict_timings()["download_ms"])
                Sbar += w[s] * Sig_s
                Mu[s] = mu_s
            t0 = time.perf_counter()
            W = w.sum()
            mu = (w[:, None] * Mu).sum(axis=0) / W
            D = np.sqrt(w / W)[:, None] * (Mu - mu)
            Sigma = Sbar / W + D.T @ D
            mom_ms = 1e3 * (time.perf_counter() - t0)
            rec_h = {"predict_call_wall_ms": float(np.median(call_wall)), "predict_download_ms": float(np.median(dl_ms)),
                     "predicts_wall_ms": float(np.sum(call_wall)), "moments_ms": mom_ms, "total_wall_ms": 1e3 * (time.perf_counter() - t_all)}
            if r >= 1:
                dev.append(rec_d)
                host.append(rec_h)
            diff = {"max_abs_diff_Sigma": float(np.max(np.abs(Sigma - got["Sigma"]))), "max_abs_diff_mu": float(np.max(np.abs(mu - got["mu"]))),
                    "median_var_within": float(np.median(got["var_within"])), "median_var_between": float(np.median(got["var_between"]))}
        for name, recs in (("device", dev), ("host", host)):
            lines.append(json.dumps({"route": name, **{k: stats([x[k] for x in recs]) for k in recs[0]}}))
            print(lines[-1], flush=True)
        lines.append(json.dumps({"agreement": diff}))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
