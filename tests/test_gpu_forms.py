"""GPU: every (form, scheme) cell of the persistent Cholesky kernel against a plain high-precision reference.

dag_launch<AUG, STREAM> (psoap_amd/csrc/dag_launch.hpp) dispatches over 24 built forms -- the likelihood and predict with
C in 1..3 x {throughput, LAT, LAT wide}, the resident stream with C x {throughput, LAT} -- and the LAT and wide forms run
under two task-list schemes (1 latency, 2 following).  Each case of tests/gpu_form_cases.py declares the cell it means to
reach; here it runs, and asserts

* the launch counters (psoap_dag_form_launches) moved for exactly the declared form, and the scheme is the declared one
  (the likelihood's task list, the stream's stats, the environment predict reads);
* every output agrees with the LAPACK oracle within the contract, and with the long-double value (oracle.lnlike_ext /
  predict_ext, N <= 1300) within 1e-11 of the likelihood's scale (max(1, |lnp|, and the terms lnp is the difference of:
  gpu_form_cases.lnlike_refs));
* a second call gives the same bits.

The module ends with the coverage check: all 39 cells ran."""
import ctypes
import json

import numpy as np
import pytest

import gpu_form_cases as fc

pytestmark = pytest.mark.gpu

TASK = np.dtype([("type", "u1"), ("q", "u1"), ("j", "u1"), ("S", "u1"), ("b", "<u2"), ("pa", "u1"), ("pb", "u1"),
                 ("slot", "<u4"), ("ctr", "<u4")])
PART, OFF = 0, 2
TYPE_MASK, WAITNEXT = 0x0F, 0x40

_RAN = {}           # cell -> names of the cases that reached it
_SPLIT = set()      # likelihood forms seen with a split tile in their task list


def _counts():
    from psoap_amd import _lib
    return _lib.dag_form_launches()


def _ran(before):
    after = _counts()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def _assert_form(case, moved):
    form = case.cell[0]
    assert set(moved) == {form} and moved[form] >= 1, f"{case.name}: declared {form}, the counters moved {moved}"


def _task_list(h):
    n = ctypes.c_longlong()
    assert h._L.psoap_chunk_dag_tasks(h._h, None, 0, ctypes.byref(n)) == 0
    tasks = np.zeros(n.value, dtype=TASK)
    assert h._L.psoap_chunk_dag_tasks(h._h, tasks.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)) == 0
    return tasks


def _scheme_of(tasks, lat):
    """0 for the throughput forms; under LAT: 2 when every strip solve follows the factorisation (DAG_WAITNEXT on the
    OFF finals), 1 when none does"""
    if not lat:
        return 0
    ty = tasks["type"] & TYPE_MASK
    follows = (tasks["type"][ty == OFF] & WAITNEXT) != 0
    assert follows.size, "no off-diagonal tile: the scheme cannot be read"
    assert follows.all() or not follows.any()
    return 2 if follows.all() else 1


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(b)
    return float(np.max(np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin])), initial=0.0))


def _record(case, **row):
    _RAN.setdefault(case.cell, []).append(case.name)
    print("FORMROW " + json.dumps({"cell": f"{case.cell[0]} s{case.cell[1]}", "case": case.name, **row}))


def _check_lnp(case, got, lap, ext, rej):
    ld, scale = ext if ext is not None else (None, None)
    if rej is not None:
        assert got[rej] == -np.inf, (case.name, got[rej])
    ok = [b for b in range(case.B) if b != rej]
    assert np.all(np.isfinite(got[ok])), (case.name, got)
    for b in ok:
        assert abs(got[b] - lap[b]) <= fc.LNP_RTOL * max(1.0, abs(lap[b])), (case.name, b, got[b], lap[b])
        if ld is not None:
            assert abs(got[b] - ld[b]) <= fc.LNP_EXT_RTOL * scale[b], (case.name, b, got[b], ld[b], scale[b])
    return {"B": case.B, "d_lap": _rel(got[ok], lap[ok]),
            "d_ext": None if ld is None else _rel(got[ok], ld[ok]),
            "lapack_vs_ext": None if ld is None else _rel(lap[ok], ld[ok]),
            "terms_over_lnp": None if ld is None else float(np.max(scale[ok] / np.maximum(1.0, np.abs(ld[ok]))))}


LNLIKE = [c for c in fc.CASES if c.kind == "lnlike"]
STREAM = [c for c in fc.CASES if c.kind == "stream"]
PREDICT = [c for c in fc.CASES if c.kind == "predict"]


@pytest.mark.parametrize("case", LNLIKE, ids=[c.name for c in LNLIKE])
def test_lnlike_form(case, monkeypatch):
    from psoap_amd.chunk import ChunkHandle
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    if not case.env:
        monkeypatch.delenv("PSOAP_DAG_SCHEME", raising=False)
        monkeypatch.delenv("PSOAP_DAG_WIDE", raising=False)
    ch, lw, gps, rej = fc.lnlike_inputs(case)
    lap, ext = fc.lnlike_refs(case, ch, lw, gps, rej)
    with ChunkHandle(ch.fl, ch.sigma, max_batch=case.B) as h:
        before = _counts()
        got = h.lnlike_batch(lw, gps, case.mu)
        moved = _ran(before)
        tasks = _task_list(h)
        again = h.lnlike_batch(lw, gps, case.mu)
    _assert_form(case, moved)
    assert _scheme_of(tasks, case.form != "TP") == case.scheme, case.name
    finals = (tasks["type"] & TYPE_MASK) != PART
    split = bool(np.any(tasks["S"][finals] >= 2))
    if case.split:
        assert split, f"{case.name}: no split tile in the task list"
    if split:
        _SPLIT.add(case.cell[0])
    row = _check_lnp(case, got, lap, ext, rej)
    assert np.array_equal(got, again), case.name
    row["N"] = ch.N
    _record(case, split=split, **row)


@pytest.mark.parametrize("case", STREAM, ids=[c.name for c in STREAM])
def test_stream_form(case, monkeypatch):
    from psoap_amd.chunk import ChunkHandle
    monkeypatch.delenv("PSOAP_DAG_SCHEME", raising=False)
    ch, lw, gps, rej = fc.lnlike_inputs(case)
    lap, ext = fc.lnlike_refs(case, ch, lw, gps, rej)
    with ChunkHandle(ch.fl, ch.sigma, max_batch=case.B) as h:
        before = _counts()
        h.stream_open(case.c, case.B, case.scheme)
        got = h.stream_fetch(h.stream_submit(lw, gps, case.mu))
        again = h.stream_fetch(h.stream_submit(lw, gps, case.mu))
        st = h.stream_stats()
        h.stream_close()
        moved = _ran(before)
    _assert_form(case, moved)
    assert st["scheme"] == case.scheme, (case.name, st)
    row = _check_lnp(case, got, lap, ext, rej)
    assert np.array_equal(got, again), case.name
    row["N"] = ch.N
    _record(case, **row)


@pytest.mark.parametrize("case", PREDICT, ids=[c.name for c in PREDICT])
def test_predict_form(case, monkeypatch):
    import oracle
    from psoap_amd import covariance as cov
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    ch, pred, mus = fc.predict_inputs(case)
    gp = case.gp()
    lw = np.stack(ch.lwls)
    before = _counts()
    if case.mode == 2:
        mu, Sig = cov.predict_f(lw[0], ch.fl, ch.sigma, pred[0], gp[0], gp[1], mus[0])
    else:
        mu, Sig = cov._predict(case.mode, lw, ch.fl, ch.sigma, pred, mus, gp)
    mu_d, var = cov._predict(case.mode, lw, ch.fl, ch.sigma, pred, mus, gp, want_sigma="diag")
    mu2, Sig2 = cov._predict(case.mode, lw, ch.fl, ch.sigma, pred, mus, gp)
    moved = _ran(before)
    _assert_form(case, moved)
    assert dict(case.env)["PSOAP_DAG_SCHEME"] == str(case.scheme)       # the scheme predict's plan is built with
    mu_l, Sig_l = fc.predict_lapack(case.mode, lw, ch.fl, ch.sigma, pred, mus, gp)
    assert np.max(np.abs(mu - mu_l)) <= fc.MU_ATOL, case.name
    assert np.max(np.abs(Sig - Sig_l)) <= fc.SIGMA_ATOL, case.name
    assert np.max(np.abs(mu_d - mu_l)) <= fc.MU_ATOL and np.max(np.abs(var - np.diag(Sig_l))) <= fc.SIGMA_ATOL, case.name
    row = {"N": ch.N, "mu_lap": float(np.max(np.abs(mu - mu_l))), "Sigma_lap": float(np.max(np.abs(Sig - Sig_l)))}
    if ch.N <= fc.EXT_MAX_N:
        mu_x, Sig_x = oracle.predict_ext(case.mode, lw, ch.fl, ch.sigma, pred, mus, gp)
        mu_x, Sig_x = mu_x.astype(np.float64), Sig_x.astype(np.float64)
        assert np.max(np.abs(mu - mu_x)) <= fc.MU_ATOL and np.max(np.abs(Sig - Sig_x)) <= fc.SIGMA_ATOL, case.name
        row.update(mu_ext=float(np.max(np.abs(mu - mu_x))), Sigma_ext=float(np.max(np.abs(Sig - Sig_x))),
                   lapack_mu_vs_ext=float(np.max(np.abs(mu_l - mu_x))))
    assert np.array_equal(mu, mu2) and np.array_equal(Sig, Sig2), case.name
    _record(case, mode=case.mode, mu=case.mu, **row)


def test_every_form_and_scheme_ran(request):
    """the 39 cells (tests/gpu_form_cases.py: CELLS) were all reached by a case above; every likelihood form also with a
    split tile in its task list"""
    from psoap_amd import covariance
    covariance.release_handles()
    missing = sorted(set(fc.CELLS) - set(_RAN))
    if missing and request.config.getoption("keyword"):
        pytest.skip(f"cases deselected with -k: {len(missing)} of {len(fc.CELLS)} cells not run")
    print("FORMCELLS " + json.dumps({f"{f} s{s}": len(_RAN.get((f, s), [])) for f, s in fc.CELLS}))
    assert not missing, f"cells no case reached: {missing}"
    lnlike_forms = {f for f, _ in fc.CELLS if f.startswith("lnlike/")}
    assert lnlike_forms <= _SPLIT, f"likelihood forms never run with a split tile: {sorted(lnlike_forms - _SPLIT)}"
