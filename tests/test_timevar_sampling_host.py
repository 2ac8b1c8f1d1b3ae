"""The pure-host argument checks of the time scales on the batch route (psoap_amd/csrc/marg_grad_plan.hpp: batch_tau_check, what
psoap_batch_set_tau asks before any work; lnprob_tv_check, what psoap_chunk_lnprob_tv_grad and psoap_chunk_lnprob_marg_tv_grad ask
before the orbits are looked at) built by a host compiler alone into tests/host/timevar_sampling_host_check.cpp, with
AddressSanitizer and UBSan, and run as a child process: a clean run -- the program checks the order of the refusals and their
words itself -- and every line it prints reproduced by the restatement below.  Then the boundary: the three entries declared,
bound and reachable from Python."""
import ctypes
import os
import subprocess

import pytest

from test_plan_host import FLAGS, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "timevar_sampling_host_check.cpp")

GOOD = dict(array=True, B=9, c=2, pending=True, pend_B=9, pend_c=2, have_times=True, open_stream=False, have_baseline=False)
LGOOD = dict(arrays=True, grad_gp=True, grad_orb=True, grad_tau=True, grad_rest=True, B=3, have_grid=True, have_times=True,
             open_stream=False)
TIMES = "call psoap_chunk_set_times first"
STREAM = "the handle has an open stream (psoap_stream_close first)"
BASELINE = ("the handle has a baseline (psoap_chunk_set_baseline): the value under a baseline goes through "
            "psoap_chunk_lnlike_marg_tv")


def check(**change):
    """batch_tau_check restated: -> the refusal, or "ok" """
    a = dict(GOOD, **change)
    if not a["array"]:
        return "bad arguments"
    if not 1 <= a["c"] <= 3:
        return "number of components must be 1, 2 or 3"
    if a["B"] < 1:
        return "B must be at least 1"
    if not a["have_times"]:
        return TIMES
    if a["open_stream"]:
        return STREAM
    if a["have_baseline"]:
        return BASELINE
    if not a["pending"]:
        return "no upload is pending (psoap_batch_upload, psoap_batch_upload_velocities or psoap_batch_upload_orbits first)"
    if (a["B"], a["c"]) != (a["pend_B"], a["pend_c"]):
        return "B and c must be those of the pending upload"
    return "ok"


def lcheck(**change):
    """lnprob_tv_check restated"""
    a = dict(LGOOD, **change)
    if not a["arrays"]:
        return "bad arguments"
    if not a["grad_gp"] and (a["grad_orb"] or a["grad_tau"] or a["grad_rest"]):
        return "grad_gp == NULL asks for the value only: grad_orb, grad_tau, grad_vel and grad_mu must be NULL too"
    if a["grad_gp"] and not (a["grad_orb"] and a["grad_tau"]):
        return "grad_orb and grad_tau go with grad_gp"
    if a["B"] < 1:
        return "B must be at least 1"
    if not a["have_grid"]:
        return "call psoap_chunk_set_grid and psoap_chunk_set_dates first"
    if not a["have_times"]:
        return TIMES
    if a["open_stream"]:
        return STREAM
    return "ok"


def expected():
    tau = [("ok", {}), ("ok-B1-c1", dict(B=1, pend_B=1, c=1, pend_c=1)), ("ok-c3", dict(c=3, pend_c=3)),
           ("no-array", dict(array=False)), ("c0", dict(c=0)), ("c4", dict(c=4)), ("B0", dict(B=0)),
           ("no-pending", dict(pending=False, pend_B=0, pend_c=0)), ("B-mismatch", dict(B=8)), ("c-mismatch", dict(c=3)),
           ("no-times", dict(have_times=False)), ("open-stream", dict(open_stream=True)), ("baseline", dict(have_baseline=True))]
    none = dict(grad_gp=False, grad_orb=False, grad_tau=False)
    lnp = [("ok", {}), ("ok-no-rest", dict(grad_rest=False)), ("value-only", dict(none, grad_rest=False)),
           ("no-arrays", dict(arrays=False)), ("orb-and-tau-without-gp", dict(grad_gp=False)), ("rest-without-gp", none),
           ("gp-without-tau", dict(grad_tau=False)), ("gp-without-orb", dict(grad_orb=False)), ("B0", dict(B=0)),
           ("no-grid", dict(have_grid=False)), ("no-times", dict(have_times=False)), ("open-stream", dict(open_stream=True))]
    return [f"set_tau {n} : {check(**c)}" for n, c in tau] + [f"lnprob {n} : {lcheck(**c)}" for n, c in lnp]


def test_ctypes_declarations_and_python_layers():
    from psoap_amd import _lib
    from psoap_amd.chunk import ChunkHandle
    dp = _lib._dp
    res, args = _lib.SIGNATURES["psoap_batch_set_tau"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, dp]
    base = _lib.SIGNATURES["psoap_chunk_lnprob_grad"][1]
    for name in ("psoap_chunk_lnprob_tv_grad", "psoap_chunk_lnprob_marg_tv_grad"):
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(base) + 2 and args.count(dp) == base.count(dp) + 2
        assert args[6] is ctypes.c_double
    header = open(os.path.join(ROOT, "include", "psoap_gp.h")).read()
    for entry in ("psoap_batch_set_tau", "psoap_chunk_lnprob_tv_grad", "psoap_chunk_lnprob_marg_tv_grad"):
        assert f"int {entry}(" in header
    assert all(callable(getattr(ChunkHandle, n)) for n in ("set_tau", "lnprob_tv_grad", "lnprob_marg_tv_grad"))


def test_checks_run_clean_under_sanitizers_and_match_the_restatement(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    exe = str(tmp_path / "timevar_sampling_host_check")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True,
                        cwd=str(tmp_path))
    assert cc.returncode == 0, cc.stderr
    if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        assert cc.stderr == "", cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    assert run.stdout.splitlines() == expected()
