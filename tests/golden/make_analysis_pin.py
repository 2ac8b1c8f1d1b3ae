#!/usr/bin/env python3
"""The exact pin of the analysis paths behind the C ABI (gradient, orbit gradient, Fisher information, leave-one-out, continuum
marginalisation and its gradients, the time-variable kernel's gradient and Fisher information, the staged likelihood, the
predict family): for every call of ``CALLS`` the int64 bit pattern of every output
array and, from ``ChunkHandle.timings()``, the per-class ``launches``, ``flops`` and ``bytes`` -- host-computed integers held in
doubles.  ``ms`` and ``total_ms`` are measurements and are not recorded.  A predict call also records ``predict_timings()["flops"]`` (host-computed; no ``*_ms``
field).  tests/test_gpu_analysis_pin.py replays ``CALLS``
through ``run`` and compares with ``==``.

Needs the device: every call runs twice, with profiling on, on a fresh handle, and an output whose bits (or a bookkeeping
field whose value) differ between the two runs is refused, not recorded.

    python tests/golden/make_analysis_pin.py [--out DIRECTORY] [--commit ID]

The calls are spread over the files of ``PIN_FILES`` by the prefix of their names, so that no fixture outgrows what the
repository takes for one file; ``load_pin`` reads them back as one.

The fixture pins the library as it is when this runs: generate it BEFORE a change that has to keep the bits, never after.
``--commit`` is stored in the file as ``generated_at``.  The shapes are those of the reference modules of tests/: the
smallest at which each path differs (a second tile row, two groups of proposals, an empty epoch, a Gram matrix that crosses
a block row).
"""
import contextlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (ROOT, TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fisher_reference as fr  # noqa: E402
import grad_reference as gr  # noqa: E402
import marg_fisher_reference as mf  # noqa: E402
import marg_predict_reference as mp  # noqa: E402
import marg_reference as mr  # noqa: E402
import orbit_grad_reference as ogr  # noqa: E402
import timevar_fisher_reference as tf  # noqa: E402
from psoap_amd import synthetic as syn  # noqa: E402
from psoap_amd import _lib  # noqa: E402
from psoap_amd._lib import K_NAMES, dptr  # noqa: E402
from psoap_amd.utils import MODEL_ID  # noqa: E402

# prefix of a call's name -> its file, the first that matches (the plain predict calls and the draws share one)
PIN_FILES = (("predict_marg", "predict_marg_pin_v1.npz"), ("predict", "predict_pin_v1.npz"), ("", "analysis_pin_v1.npz"))
BOOK_FIELDS = ("launches", "flops", "bytes")
ORBIT_BASELINE = {"order": 1, "sd": list(mr.PLANT_SD), "weight": "one"}
FAST_K = 4.0e6                  # km/s: thirteen times the speed of light (tests/test_gpu_marg_grad.py)


# ---- set-ups -----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _handle(ch, baseline=None, **kw):
    """a fresh handle on the chunk's data, profiling on; ``baseline = (case, kind)`` sets that case's baseline"""
    from psoap_amd.chunk import ChunkHandle
    with ChunkHandle(ch.fl, ch.sigma, **kw) as h:
        h.set_profiling(True)
        if baseline is not None:
            case, kind = baseline
            h.set_baseline(ch.order, ch.x, ch.epoch_index, ch.n_epochs, mr.prior_sd(ch.order), mr.case_weight(case, kind))
        yield h


@contextlib.contextmanager
def _orbit_worker(baseline):
    """the SB2 chunk of the orbit-gradient tests at N = 129 (two tile rows), profiling on"""
    from psoap_amd.lnprob import ChunkWorker
    ch = ogr.CHAIN_CASES[0].chunk
    w = ChunkWorker("SB2", ch.lwl, ch.fl, ch.sigma, ch.epoch_index, ch.dates, baseline=baseline)
    try:
        w.handle.set_profiling(True)
        yield w.handle
    finally:
        w.close()


def _batch(case, B, seed, negative=None):
    """B proposals around a case of marg_reference: grids a few 1e-6 apart, seeded hyper-parameters (the case's own first);
    ``negative``: the proposal whose second hyper-parameter changes sign"""
    ch, c = mr.case_chunk(case), case[2]
    gps = syn.make_walkers(c, B, seed=seed)
    gps[0] = mr.case_gp(case)
    if negative is not None:
        gps[negative, 1] = -gps[negative, 1]
    return np.stack([ch.lwls + 1e-6 * k for k in range(B)]), gps


def _orbit_batch():
    """three SB2 orbits, the one in the middle faster than light"""
    P = syn.make_orbit_proposals("SB2", 3, seed=920)
    P[1, 1] = FAST_K
    return P, syn.make_walkers(2, 3, seed=921)


def _named(names, values):
    return dict(zip(names, values))


GRAD_OUT = ("lnp", "grad_gp", "grad_lwl", "grad_mu")
TV_GRAD_OUT = ("lnp", "grad_gp", "grad_tau", "grad_lwl", "grad_mu")
ORBIT_OUT = ("lnp", "grad_orb", "grad_gp", "grad_mu", "grad_vel")
LOO_OUT = ("lnp", "loo_logp", "pix_mean", "pix_var", "pix_logp", "ep_resid", "ep_chi2", "ep_logp", "ep_npix")
MARG_OUT = ("lnp", "parts", "beta", "beta_cov", "fl_cor")


# ---- the calls: name -> a context manager that yields (handle, call); call() -> {output: array} ------------------------------
@contextlib.contextmanager
def _lnlike_grad(B):
    case = mr.case_named("c")
    ch = mr.case_chunk(case)
    lw, gps = (ch.lwls, mr.case_gp(case)) if B == 1 else _batch(case, B, 9701, negative=4)
    with _handle(ch) as h:
        yield h, lambda: _named(GRAD_OUT, h.lnlike_grad(lw, gps, mr.MU_GP))


@contextlib.contextmanager
def _lnprob_grad(marg):
    P, gps = _orbit_batch()
    with _orbit_worker(ORBIT_BASELINE if marg else None) as h:
        entry = h.lnprob_marg_grad if marg else h.lnprob_grad
        yield h, lambda: _named(ORBIT_OUT, entry(MODEL_ID["SB2"], P, gps, gr.MU_GP, want_vel=True))


@contextlib.contextmanager
def _fisher(grid_tangents):
    case = fr.CASES[2]                      # N = 129, c = 2
    assert case[:2] == (129, 2)
    ch, gp, c = fr.case_chunk(case), fr.case_gp(case), case[1]
    tan_lwl, tan_gp = fr.case_tangents(case)
    pick = [1, 2 * c] if grid_tangents else [0, 1]          # a hyper-parameter and a velocity tangent / two hyper-parameters
    with _handle(ch) as h:
        yield h, lambda: _named(("F", "F_mu"), h.fisher(ch.lwls, gp, tan_gp[pick], tan_lwl[pick] if grid_tangents else None,
                                                        want_mu=True))


@contextlib.contextmanager
def _fisher_tv():
    """N = 129, c = 2 (an off-diagonal tile, a diagonal tile with masked rows, 127 padded rows), tau = (2 span, inf): an
    amplitude, a length-scale, a time-scale (of the finite tau) and a grid tangent"""
    case = next(k for k in tf.CASES if tf.case_id(k) == "N129-c2")
    d = tf.case_data(case)
    assert np.isfinite(d.tau[0]) and np.isinf(d.tau[1])
    tan_lwl, tan_gp, tan_tau = tf.case_tangents(case)
    pick = [0, 1, 4, 6]
    assert all(np.any(a[pick]) for a in (tan_lwl, tan_gp[:, 0::2], tan_gp[:, 1::2], tan_tau))
    with _handle(d) as h:
        h.set_times(d.times)
        yield h, lambda: _named(("F", "F_mu"), h.fisher_tv(d.lwls, d.gp, d.tau, tan_gp[pick], tan_tau[pick], tan_lwl[pick],
                                                           want_mu=True))


@contextlib.contextmanager
def _lnlike_tv_grad():
    """the batch of ``_lnlike_grad`` cut to one group of three, the epochs 30 days apart, one tau finite and one infinite in
    every proposal"""
    case = mr.case_named("c")
    ch = mr.case_chunk(case)
    lw, gps = _batch(case, 3, 9703)
    tau = np.array([[40.0, np.inf], [np.inf, 25.0], [70.0, np.inf]])
    with _handle(ch) as h:
        h.set_times(30.0 * ch.epoch_index)
        yield h, lambda: _named(TV_GRAD_OUT, h.lnlike_tv_grad(lw, gps, tau, mr.MU_GP))


@contextlib.contextmanager
def _fisher_marg(name, kind, grid_tangents, negative=False):
    """as ``_fisher`` under the case's baseline; ``negative``: the second hyper-parameter changes sign"""
    case = mr.case_named(name)
    ch, gp, c = mr.case_chunk(case), mr.case_gp(case), case[2]
    if negative:
        gp[1] = -gp[1]
    tan_lwl, tan_gp = mf.case_tangents(case)
    pick = [1, 2 * c] if grid_tangents else [0, 1]
    with _handle(ch, baseline=(case, kind)) as h:
        yield h, lambda: _named(("F", "F_mu"), h.fisher_marg(ch.lwls, gp, tan_gp[pick], tan_lwl[pick] if grid_tangents else None,
                                                             want_mu=True))


@contextlib.contextmanager
def _loo(name, epochs, kind=None):
    """``kind``: under the case's baseline with that weight (``loo_marg``)"""
    case = mr.case_named(name)
    ch, gp = mr.case_chunk(case), mr.case_gp(case)
    with _handle(ch, baseline=None if kind is None else (case, kind)) as h:
        def call():
            r = (h.loo if kind is None else h.loo_marg)(ch.lwls, gp, mr.MU_GP, *((ch.epoch_index, ch.n_epochs) if epochs else ()))
            return {k: getattr(r, k) for k in LOO_OUT if getattr(r, k) is not None}
        yield h, call


@contextlib.contextmanager
def _lnlike_marg(name, kind, B, more):
    case = mr.case_named(name)
    ch = mr.case_chunk(case)
    lw, gps = (ch.lwls, mr.case_gp(case)) if B == 1 else _batch(case, B, 9702)
    with _handle(ch, baseline=(case, kind), max_batch=B) as h:
        def call():
            r = h.lnlike_marg(lw, gps, mr.MU_GP, want_beta=more, want_cov=more, want_flux=more)
            return {k: getattr(r, k) for k in MARG_OUT} if more else {"lnp": r}
        yield h, call


@contextlib.contextmanager
def _lnlike_marg_grad():
    case = mr.case_named("f")
    lw, gps = _batch(case, 10, 9801)
    with _handle(mr.case_chunk(case), baseline=(case, "flux")) as h:
        yield h, lambda: _named(GRAD_OUT, h.lnlike_marg_grad(lw, gps, mr.MU_GP))


@contextlib.contextmanager
def _lnlike_marg_grad_parts():
    """one group of three, the one in the middle refused; ``parts`` asked for, which ``ChunkHandle.lnlike_marg_grad`` does not"""
    case = mr.case_named("c")
    lw, gps = _batch(case, 3, 9802, negative=1)
    with _handle(mr.case_chunk(case), baseline=(case, "one")) as h:
        def call():
            parts = np.empty((3, 4))
            got = h._lnlike_grad("psoap_chunk_lnlike_marg_grad", lw, gps, mr.MU_GP, dptr(parts))
            return dict(_named(GRAD_OUT, got), parts=parts)
        yield h, call


@contextlib.contextmanager
def _staged_lnlike():
    case = mr.case_named("c")
    lw, gps = _batch(case, 3, 9703)
    with _handle(mr.case_chunk(case), max_batch=3) as h:
        h.set_mode("staged")
        yield h, lambda: {"lnp": h.lnlike_batch(lw, gps, mr.MU_GP)}


# ---- the predict family ------------------------------------------------------------------------------------------------------
FORMS = {"full": True, "diag": "diag", "mean": False}       # want_sigma of ChunkHandle.predict / predict_marg
PRED_OUT = {"full": ("mu", "Sigma"), "diag": ("mu", "var"), "mean": ("mu",)}
STAGED_ENV = {"PSOAP_SHARE_PROCS": "9", "PSOAP_QUIET": "1"}       # nine processes: more than PSOAP_SHARE_DAG_MAX's 8


@contextlib.contextmanager
def _environ(**kw):
    """the variables set for the duration of a call (the library reads them per call), the old values back afterwards"""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _pcase(name, mode):
    """the case of marg_predict_reference.PCASES on chunk ``name`` in ``mode`` -> (case, chunk, (mode, lwls, pred, mus, gp))"""
    pc, = [p for p in mp.PCASES if p[:2] == (name, mode)]
    case = mr.case_named(name)
    ch = mr.case_chunk(case)
    return case, ch, (mode, ch.lwls, mp.pcase_pred(pc), mp.pcase_mus(pc), mr.case_gp(case))


def _predicted(h, entry, args, form):
    """one predict call in ``form`` -> its arrays and the host-computed flop count of ``predict_timings()``"""
    got = entry(*args, want_sigma=FORMS[form])
    out = _named(PRED_OUT[form], got if isinstance(got, tuple) else (got,))
    out["predict_flops"] = h.predict_timings()["flops"]
    return out


@contextlib.contextmanager
def _predict(name, mode, form, env=None, staged=False):
    """plain ``predict`` of a case; ``env``: variables around the call; ``staged``: the call has to take the staged branch,
    which the library's own count of such calls says -- the pin cannot silently record the persistent one"""
    _, ch, args = _pcase(name, mode)
    with _handle(ch) as h:
        def call():
            before = _lib.share_stats()["staged_policy"]
            with _environ(**(env or {})):
                out = _predicted(h, h.predict, args, form)
            assert not staged or _lib.share_stats()["staged_policy"] > before, "the call did not take the staged branch"
            return out
        yield h, call


@contextlib.contextmanager
def _predict_transposed():
    """predict_f_g_h_sum (mode 1, c = 3, M == N = 129): the transposed mean on a prediction grid of its own, always staged"""
    ch = syn.make_chunk(3, 3, 43, seed=9901)
    assert ch.N == 129
    pred = np.stack([np.linspace(w.min(), w.max(), ch.N) for w in ch.lwls])
    with _handle(ch) as h:
        yield h, lambda: _predicted(h, h.predict, (1, ch.lwls, pred, [1.07], syn.GP_BASE[3]), "full")


@contextlib.contextmanager
def _predict_marg(name, mode, kind, form):
    case, ch, args = _pcase(name, mode)
    with _handle(ch, baseline=(case, kind)) as h:
        yield h, lambda: _predicted(h, h.predict_marg, args, form)


@contextlib.contextmanager
def _predict_draw(name, kind, D, seed=None, z_seed=None):
    """``D`` draws after ``predict`` (``kind`` None) or ``predict_marg`` of a case; ``z_seed``: the normals handed in"""
    case, ch, args = _pcase(name, 0)
    R = args[2].size                    # mode 0: c M rows
    z = None if z_seed is None else np.random.default_rng(z_seed).standard_normal((D, R))
    with _handle(ch, baseline=None if kind is None else (case, kind)) as h:
        (h.predict if kind is None else h.predict_marg)(*args)
        yield h, lambda: {"draws": h.predict_draw(D, seed=seed, z=z)}


def _predict_calls():
    calls = {}
    for form in FORMS:
        calls[f"predict-c-mode0-M65-{form}"] = lambda form=form: _predict("c", 0, form)       # two block rows, two prediction tile columns
        calls[f"predict-a-mode1-M130-{form}"] = lambda form=form: _predict("a", 1, form)      # the 1e-8 nugget
        calls[f"predict-b-mode2-M128-{form}"] = lambda form=form: _predict("b", 2, form)
        calls[f"predict_marg-c-one-mode0-M65-{form}"] = lambda form=form: _predict_marg("c", 0, "one", form)
        calls[f"predict_marg-f-flux-mode0-M100-{form}"] = lambda form=form: _predict_marg("f", 0, "flux", form)   # Q = 2
        calls[f"predict_marg-a-one-mode1-M130-{form}"] = lambda form=form: _predict_marg("a", 1, "one", form)
        calls[f"predict_marg-b-one-mode2-M128-{form}"] = lambda form=form: _predict_marg("b", 2, "one", form)
    calls["predict-c-mode0-M65-full-unfused"] = lambda: _predict("c", 0, "full", env={"PSOAP_PREDICT_FUSED": "0"})
    calls["predict-mode1-c3-N129-transposed-mean"] = _predict_transposed
    calls["predict-c-mode0-M65-full-staged"] = lambda: _predict("c", 0, "full", env=STAGED_ENV, staged=True)
    calls["predict-b-mode2-M128-full-staged"] = lambda: _predict("b", 2, "full", env=STAGED_ENV, staged=True)
    calls["predict_draw-c-plain-seed-D3"] = lambda: _predict_draw("c", None, 3, seed=20261)        # R = 130: two tile rows
    calls["predict_draw-c-plain-z-D2"] = lambda: _predict_draw("c", None, 2, z_seed=20262)
    calls["predict_draw-f-flux-seed-D3"] = lambda: _predict_draw("f", "flux", 3, seed=20263)
    return calls


CALLS = {
    "lnlike_grad-c-B1": lambda: _lnlike_grad(1),
    "lnlike_grad-c-B10-negative": lambda: _lnlike_grad(10),               # two groups, 8 + 2
    "lnprob_grad-SB2-N129-B3-fast": lambda: _lnprob_grad(False),
    "fisher-N129-T2-no-grid-tangents": lambda: _fisher(False),
    "fisher-N129-T2-grid-tangents": lambda: _fisher(True),
    "loo-e-epochs": lambda: _loo("e", True),                              # an empty epoch, runs not in id order
    "loo-c-pixels-only": lambda: _loo("c", False),
    "lnlike_marg-c-B1": lambda: _lnlike_marg("c", "one", 1, False),
    "lnlike_marg-c-B1-beta-cov-flux": lambda: _lnlike_marg("c", "one", 1, True),
    "lnlike_marg-f-B3": lambda: _lnlike_marg("f", "flux", 3, False),       # Q = 2: M crosses a block row
    "lnlike_marg-f-B3-beta-cov-flux": lambda: _lnlike_marg("f", "flux", 3, True),      # the [M | I] sweep
    "lnlike_marg_grad-f-flux-B10": _lnlike_marg_grad,
    "lnprob_marg_grad-SB2-N129-B3-fast": lambda: _lnprob_grad(True),
    "staged-lnlike_batch-c-B3": _staged_lnlike,
    "fisher_marg-c-one-T2-no-grid-tangents": lambda: _fisher_marg("c", "one", False),      # N = 129, Q = 1
    "fisher_marg-f-flux-T2-grid-tangents": lambda: _fisher_marg("f", "flux", True),        # Q = 2: the second K loop spans two slots
    "loo_marg-e-flux-epochs": lambda: _loo("e", True, "flux"),
    "loo_marg-f-one-pixels-only": lambda: _loo("f", False, "one"),
    "fisher_marg-c-one-negative": lambda: _fisher_marg("c", "one", False, negative=True),      # the NaN convention
    "lnlike_marg_grad-c-one-B3-negative": _lnlike_marg_grad_parts,          # one group, a refusal: parts, the poisoned gradient
    "fisher_tv-N129-T4-finite-tau": _fisher_tv,
    "lnlike_tv_grad-c-B3-finite-tau": _lnlike_tv_grad,
    **_predict_calls(),
}


# ---- running and comparing -------------------------------------------------------------------------------------------------
def bits(a):
    """the int64 bit pattern of a float64 array (or scalar); integer arrays as int64 values"""
    a = np.atleast_1d(np.asarray(a))
    if a.dtype.kind in "iu":
        return a.astype(np.int64)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).copy()


def book(timings):
    """(3, classes): launches, flops and bytes per kernel class, in the order of ``K_NAMES``"""
    return np.array([[float(timings[name][f]) for name in K_NAMES] for f in BOOK_FIELDS])


def run(name, repeats=1):
    """``repeats`` runs of the call on ONE fresh handle -> [({output: bits}, book), ...]"""
    out = []
    with CALLS[name]() as (h, call):
        for _ in range(repeats):
            got = call()
            out.append(({k: bits(v) for k, v in got.items()}, book(h.timings())))
    return out


def pin_file(name):
    return next(f for prefix, f in PIN_FILES if name.startswith(prefix))


def load_pin(directory=HERE):
    """every fixture file as one dict: "<call>/<output>" -> array, and "generated_at", which all of them share"""
    pin = {}
    for _, fname in PIN_FILES:
        with np.load(os.path.join(directory, fname)) as f:
            assert pin.get("generated_at", f["generated_at"]) == f["generated_at"], "the fixture files are of different commits"
            pin.update({k: f[k] for k in f.files})
    return pin


def write_pin(pin, directory):
    for _, fname in PIN_FILES:
        path = os.path.join(directory, fname)
        np.savez_compressed(path, generated_at=pin["generated_at"],
                            **{k: v for k, v in pin.items() if "/" in k and pin_file(k.rsplit("/", 1)[0]) == fname})
        print("wrote", path, os.path.getsize(path))


def main(argv):
    directory = argv[argv.index("--out") + 1] if "--out" in argv else HERE
    commit = argv[argv.index("--commit") + 1] if "--commit" in argv else "unknown"
    pin, refused = {"generated_at": np.array(commit)}, []
    for name in CALLS:
        (first, book1), (second, book2) = run(name, repeats=2)
        for k in first:
            if not np.array_equal(first[k], second[k]):
                refused.append(f"{name}/{k}")
            pin[f"{name}/{k}"] = first[k]
        if not np.array_equal(book1, book2):
            refused.append(f"{name}/book")
        pin[f"{name}/book"] = book1
        print(f"{name}: {', '.join(f'{k}{list(v.shape)}' for k, v in first.items())}; launches "
              f"{dict(zip(K_NAMES, (int(v) for v in book1[0])))}")
    if refused:
        raise SystemExit("two runs on one handle differ, nothing written: " + ", ".join(refused))
    write_pin(pin, directory)


if __name__ == "__main__":
    main(sys.argv[1:])
