#!/usr/bin/env python3
"""Every analysis entry of the C ABI once, for comparing two builds of the library: a change to the host layer that should move
nothing must leave this tool's first output identical line for line.

    python tools/analysis_ab.py [--tree DIRECTORY] [--out FILE] [--ms-out FILE] [--repeats R] [--sizes N ...]

``--tree``: the checkout whose ``psoap_amd`` (and built library) is loaded -- this one by default, an older one to get the
other side of the comparison.  Only what old checkouts have is imported from the package; an entry the loaded ``ChunkHandle``
lacks is reported as ``absent``.

``--out`` (default: standard output): for N = 129 (P = 2, the smallest size with an off-diagonal tile) and N = 257, c = 2,
baseline of order 1 where one applies, profiling on, one fresh handle per call -- the SHA-256 of every output array and, per
kernel class, ``launches``, ``flops`` and ``bytes`` of ``ChunkHandle.timings()`` (host-computed).  ``--ms-out``: the device
milliseconds per class of ``--repeats`` further runs of each call on the same handle (measurements: they differ run to run).
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ap.add_argument("--ms-out", default=None)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--sizes", type=int, nargs="+", default=[129, 257], help="N of the chunks (for --ms-out: a larger one)")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

from psoap_amd import synthetic as syn  # noqa: E402
from psoap_amd._lib import K_NAMES, check, dptr  # noqa: E402
from psoap_amd.chunk import ChunkHandle  # noqa: E402
from psoap_amd.utils import MODEL_ID  # noqa: E402

C, B, EPOCHS, MU = 2, 3, 3, 1.0
PRIOR_SD = (0.05, 0.02)          # order 1: offset and slope of the continuum of every epoch
BOOK = ("launches", "flops", "bytes")


def chunk(N):
    """c = 2, three epochs, the last one cut so that the chunk has N pixels (every epoch one contiguous run)"""
    ch = syn.make_chunk(C, EPOCHS, -(-N // EPOCHS), seed=4200 + N)
    return {"fl": ch.fl[:N], "sigma": ch.sigma[:N], "lwl": ch.lwl[:N], "lwls": np.ascontiguousarray(ch.lwls[:, :N]),
            "epoch": ch.epoch_index[:N].astype(np.int32), "dates": ch.dates}


def proposals(ch, seed):
    return np.stack([ch["lwls"] + 1e-6 * k for k in range(B)]), syn.make_walkers(C, B, seed=seed)


def handle(ch, baseline=False, grid=False, times=False, **kw):
    h = ChunkHandle(ch["fl"], ch["sigma"], **kw)
    h.set_profiling(True)
    if grid:
        h.set_grid(ch["lwl"], ch["epoch"], EPOCHS)
        check(h._L.psoap_chunk_set_dates(h._h, dptr(ch["dates"]), EPOCHS), "psoap_chunk_set_dates")
    if times:
        t = ch["dates"][ch["epoch"]]
        h.set_times(t - t.min())
    if baseline:
        h.set_baseline(1, ch["lwl"], ch["epoch"], EPOCHS, PRIOR_SD)
    return h


def fields(r, names):
    return {k: getattr(r, k) for k in names if getattr(r, k, None) is not None}


def tup(names, r):
    return dict(zip(names, r if isinstance(r, tuple) else (r,)))


def calls(ch, N):
    """name -> (handle options, entry name, call(h) -> {output: array})"""
    lw, gps = proposals(ch, 7100 + N)
    gp = gps[0]
    orb = syn.make_orbit_proposals("SB2", B, seed=7200 + N)
    tau = np.array([[40.0, 90.0], [np.inf, 25.0], [60.0, 60.0]])
    rng = np.random.default_rng(7300 + N)
    tan_gp, tan_lwl = rng.standard_normal((2, 2 * C)), 1e-5 * rng.standard_normal((2, C, N))
    tan_tau = np.array([[7.0, -3.0], [0.0, 11.0]])      # fisher_tv and loo_tv run at tau[0]: both finite
    ep = ch["epoch"]
    GRAD, ORB = ("lnp", "grad_gp", "grad_lwl", "grad_mu"), ("lnp", "grad_orb", "grad_gp", "grad_mu", "grad_vel")
    LOO = ("lnp", "loo_logp", "pix_mean", "pix_var", "pix_logp", "ep_resid", "ep_chi2", "ep_logp", "ep_npix")
    MARG = ("lnp", "parts", "beta", "beta_cov", "fl_cor")
    INFO = ("lnp", "grad", "F", "J")
    return {
        "lnlike_grad": ({}, "lnlike_grad", lambda h: tup(GRAD, h.lnlike_grad(lw, gps, MU))),
        "lnprob_grad": ({"grid": True}, "lnprob_grad",
                        lambda h: tup(ORB, h.lnprob_grad(MODEL_ID["SB2"], orb, gps, MU, want_vel=True))),
        "lnlike_tv-value-only": ({"times": True}, "lnlike_tv", lambda h: tup(("lnp",), h.lnlike_tv(lw, gps, tau, MU))),
        "lnlike_tv_grad": ({"times": True}, "lnlike_tv_grad",
                           lambda h: tup(("lnp", "grad_gp", "grad_tau", "grad_lwl", "grad_mu"), h.lnlike_tv_grad(lw, gps, tau, MU))),
        "fisher": ({}, "fisher", lambda h: tup(("F", "F_mu"), h.fisher(ch["lwls"], gp, tan_gp, tan_lwl, want_mu=True))),
        "fisher_tv": ({"times": True}, "fisher_tv",
                      lambda h: tup(("F", "F_mu"), h.fisher_tv(ch["lwls"], gp, tau[0], tan_gp, tan_tau, tan_lwl, want_mu=True))),
        "fisher_marg": ({"baseline": True}, "fisher_marg",
                        lambda h: tup(("F", "F_mu"), h.fisher_marg(ch["lwls"], gp, tan_gp, tan_lwl, want_mu=True))),
        "fisher_vel": ({}, "fisher_vel", lambda h: tup(("F",), h.fisher_vel(ch["lwls"], gp, ep, EPOCHS))),
        "info_vel": ({}, "info_vel", lambda h: tup(INFO, h.info_vel(ch["lwls"], gp, ep, EPOCHS, MU))),
        "info_vel-marg": ({"baseline": True}, "info_vel", lambda h: tup(INFO, h.info_vel(ch["lwls"], gp, ep, EPOCHS, MU, marg=True))),
        "loo": ({}, "loo", lambda h: fields(h.loo(ch["lwls"], gp, MU, ep, EPOCHS), LOO)),
        "loo_tv": ({"times": True}, "loo_tv", lambda h: fields(h.loo_tv(ch["lwls"], gp, tau[0], MU, ep, EPOCHS), LOO)),
        "loo_marg": ({"baseline": True}, "loo_marg", lambda h: fields(h.loo_marg(ch["lwls"], gp, MU, ep, EPOCHS), LOO)),
        "lnlike_marg": ({"baseline": True, "max_batch": B}, "lnlike_marg", lambda h: tup(("lnp",), h.lnlike_marg(lw, gps, MU))),
        "lnlike_marg-want_cov": ({"baseline": True, "max_batch": B}, "lnlike_marg",
                                 lambda h: fields(h.lnlike_marg(lw, gps, MU, want_beta=True, want_cov=True, want_flux=True), MARG)),
        "lnlike_marg_grad": ({"baseline": True}, "lnlike_marg_grad", lambda h: tup(GRAD, h.lnlike_marg_grad(lw, gps, MU))),
        "lnprob_marg_grad": ({"baseline": True, "grid": True}, "lnprob_marg_grad",
                             lambda h: tup(ORB, h.lnprob_marg_grad(MODEL_ID["SB2"], orb, gps, MU, want_vel=True))),
    }


def sha(a):
    a = np.ascontiguousarray(np.atleast_1d(np.asarray(a)))
    return f"{a.dtype.str}{list(a.shape)} sha256={hashlib.sha256(a.tobytes()).hexdigest()}"


def main():
    out = open(args.out, "w") if args.out else sys.stdout
    ms_out = open(args.ms_out, "w") if args.ms_out else None
    for N in args.sizes:
        ch = chunk(N)
        assert ch["fl"].shape == (N,)
        for name, (opts, entry, call) in calls(ch, N).items():
            if getattr(ChunkHandle, entry, None) is None:
                print(f"N={N} {name}: absent", file=out, flush=True)
                continue
            h = handle(ch, **opts)
            try:
                got = call(h)
                t = h.timings()
                for k, v in got.items():
                    print(f"N={N} {name} {k} {sha(v)}", file=out)
                for f in BOOK:
                    print(f"N={N} {name} {f} " + " ".join(f"{n}={float(t[n][f])!r}" for n in K_NAMES), file=out, flush=True)
                if ms_out:
                    for r in range(args.repeats):
                        call(h)
                        t = h.timings()
                        print(f"N={N} {name} run{r} " + " ".join(f"{n}={float(t[n]['ms']):.4f}" for n in K_NAMES),
                              file=ms_out, flush=True)
            finally:
                h.close()


if __name__ == "__main__":
    main()
