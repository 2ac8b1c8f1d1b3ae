"""predict_marg against the plain predict at the retrieve shape (ST3, N = 8192, 3 x 1024 prediction pixels), on one handle
in one process: the numbers of profiles/marg_predict.md.

    python tools/marg_predict_bench.py [--rounds 9] [--order 3] [--out FILE]

Per round, alternating: the plain ``ChunkHandle.predict`` as it runs by default (persistent launch, Sigma fused), the plain
predict with the separate Sigma product (PSOAP_PREDICT_FUSED=0, read by the library at every call), ``predict_marg`` with
Sigma, ``predict_marg`` with the variances only.  ``predict_timings`` of every call; medians and ranges as one JSON line,
with the library's per-class split of one further profiled ``predict_marg`` call.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from psoap_amd import synthetic as syn  # noqa: E402
from psoap_amd.chunk import ChunkHandle  # noqa: E402

KEYS = ("device_ms", "factor_ms", "sigma_ms", "download_ms", "total_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ch = syn.make_config_chunk(5)
    M = 2 * ch.n_pix
    pred = np.linspace(np.min(ch.lwls[0]), np.max(ch.lwls[0]), num=M)
    args = (0, ch.lwls, np.stack([pred] * 3), np.zeros(3), syn.GP_BASE[3])
    sd = 0.05 * 0.5 ** np.arange(a.order + 1)
    h = ChunkHandle(ch.fl, ch.sigma, max_batch=1)
    h.set_baseline(a.order, ch.lwl, ch.epoch_index, ch.n_epochs, sd)

    def plain():
        os.environ.pop("PSOAP_PREDICT_FUSED", None)
        return h.predict(*args)

    def separate():
        os.environ["PSOAP_PREDICT_FUSED"] = "0"
        try:
            return h.predict(*args)
        finally:
            os.environ.pop("PSOAP_PREDICT_FUSED", None)

    forms = {"plain": plain, "plain_separate_sigma": separate, "marg": lambda: h.predict_marg(*args),
             "marg_var": lambda: h.predict_marg(*args, want_sigma="diag")}
    last, times = {}, {k: [] for k in forms}
    for name, f in forms.items():          # warm-up: every shape the timed rounds use (workspaces, code objects, task list)
        f()
        f()
    for _ in range(a.rounds):
        for name, f in forms.items():
            last[name] = f()
            times[name].append(h.predict_timings())
    # the results the timed calls gave: the two plain forms agree, the marginal covariance only adds to the plain one
    (mu_p, S_p), (mu_s, S_s), (mu_m, S_m), (mu_v, var) = (last[k] for k in forms)
    unit = float(np.max(np.asarray(syn.GP_BASE[3])[0::2] ** 2))          # the largest prior variance
    checks = {"plain_forms_max_diff": float(np.max(np.abs(S_p - S_s))), "marg_symmetric": bool(np.array_equal(S_m, S_m.T)),
              "marg_mu_same_bits": bool(np.array_equal(mu_m, mu_v)), "marg_var_vs_diag": float(np.max(np.abs(var - np.diag(S_m)))),
              "min_var_gain": float(np.min(var - np.diag(S_p))), "max_var_gain": float(np.max(var - np.diag(S_p))),
              "finite": bool(np.all(np.isfinite(S_m)) and np.all(np.isfinite(mu_m))), "unit": unit}
    out = {"shape": {"N": int(ch.N), "c": 3, "M": int(M), "R": int(3 * M), "n_epochs": int(ch.n_epochs), "order": a.order,
                     "q": int(ch.n_epochs * (a.order + 1))}, "rounds": a.rounds, "checks": checks}
    for name, ts in times.items():
        out[name] = {k: {"median": float(np.median([t[k] for t in ts])), "min": float(min(t[k] for t in ts)),
                         "max": float(max(t[k] for t in ts))} for k in KEYS}
        out[name]["flops"] = ts[-1]["flops"]
    # the library's own split of one more call (HIP events around every launch group: not part of the timed rounds)
    h.set_profiling(True)
    h.predict_marg(*args)
    split = h.timings()
    h.set_profiling(False)
    out["marg_split_ms"] = {k: (v if k == "total_ms" else {"ms": v["ms"], "launches": v["launches"]}) for k, v in split.items()}
    h.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
