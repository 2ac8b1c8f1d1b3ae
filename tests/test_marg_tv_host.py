"""The pure-host argument check of the time-variable kernel under the marginalised continuum (psoap_amd/csrc/marg_grad_plan.hpp:
marg_tv_check, what psoap_chunk_lnlike_marg_tv, psoap_chunk_lnlike_marg_tv_grad and psoap_chunk_fisher_marg_tv ask before any
work) built by a host compiler alone into tests/host/marg_tv_host_check.cpp, with AddressSanitizer and UBSan, and run as a
child process: a clean run -- the program checks the order of the refusals and their words itself -- and every line it prints
reproduced by the restatement below."""
import os
import subprocess

import pytest

from test_plan_host import FLAGS, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "marg_tv_host_check.cpp")

GOOD = dict(arrays=True, grad_gp=True, grad_tau=True, grad_rest=True, B=3, c=2, T=9, max_batch=4, max_T=32, have_times=True,
            open_stream=False, have_baseline=True, stale_weight=False)
STALE = "psoap_chunk_set_data changed the data the baseline's weights were given for (psoap_chunk_set_baseline again)"


def check(entry, **change):
    """marg_tv_check restated: -> the refusal, or "ok" """
    a = dict(GOOD, **change)
    if not a["arrays"]:
        return "bad arguments"
    if entry == "grad":
        if not a["grad_gp"] and (a["grad_tau"] or a["grad_rest"]):
            return "grad_gp == NULL asks for the value only: grad_tau, grad_lwl and grad_mu must be NULL too"
        if a["grad_gp"] and not a["grad_tau"]:
            return "grad_tau goes with grad_gp"
    if not 1 <= a["c"] <= 3:
        return "number of components must be 1, 2 or 3"
    if entry == "value" and not 1 <= a["B"] <= a["max_batch"]:
        return "batch size outside [1, max_batch]"
    if entry == "grad" and a["B"] < 1:
        return "B must be at least 1"
    if entry == "fisher" and not 1 <= a["T"] <= a["max_T"]:
        return "the number of tangents must be between 1 and 32"
    if not a["have_times"]:
        return "call psoap_chunk_set_times first"
    if a["open_stream"]:
        return "the handle has an open stream (psoap_stream_close first)"
    if not a["have_baseline"]:
        return "call psoap_chunk_set_baseline first"
    if a["stale_weight"]:
        return STALE
    return "ok"


def expected():
    lines = []
    common = [("ok", {}), ("no-arrays", dict(arrays=False)), ("c0", dict(c=0)), ("c4", dict(c=4)), ("c1", dict(c=1)),
              ("c3", dict(c=3)), ("no-times", dict(have_times=False)), ("open-stream", dict(open_stream=True)),
              ("no-baseline", dict(have_baseline=False)), ("stale", dict(stale_weight=True))]
    for entry in ("value", "grad", "fisher"):
        lines += [(entry, name, change) for name, change in common]
    lines += [("value", "B0", dict(B=0)), ("grad", "B0", dict(B=0)), ("fisher", "B0", dict(B=0)), ("value", "Bmax", dict(B=4)),
              ("value", "Bmax+1", dict(B=5)), ("grad", "Bmax+1", dict(B=5)), ("value", "B1", dict(B=1)),
              ("fisher", "T0", dict(T=0)), ("value", "T0", dict(T=0)), ("fisher", "T1", dict(T=1)), ("fisher", "T32", dict(T=32)),
              ("fisher", "T33", dict(T=33)),
              ("grad", "value-only", dict(grad_gp=False, grad_tau=False, grad_rest=False)),
              ("grad", "tau-without-gp", dict(grad_gp=False)), ("grad", "rest-without-gp", dict(grad_gp=False, grad_tau=False)),
              ("grad", "gp-without-tau", dict(grad_tau=False)), ("grad", "gp-and-tau", dict(grad_rest=False)),
              ("value", "grad-flags-ignored", dict(grad_gp=False))]
    return [f"{entry} {name} : {check(entry, **change)}" for entry, name, change in lines]


def test_restatement_by_hand():
    """the accepted corners and one refusal of each kind, written out"""
    assert check("value") == check("grad") == check("fisher") == "ok"
    assert check("value", B=4) == "ok" and check("value", B=5) == "batch size outside [1, max_batch]" and check("grad", B=5) == "ok"
    assert check("fisher", T=32) == "ok" and check("fisher", T=33) == "the number of tangents must be between 1 and 32"
    assert check("fisher", B=0) == "ok" and check("value", T=0) == "ok"
    assert check("grad", grad_gp=False, grad_tau=False, grad_rest=False) == "ok"
    assert check("grad", grad_gp=False).startswith("grad_gp == NULL") and check("grad", grad_tau=False) == "grad_tau goes with grad_gp"
    # the order: arguments, NULL rules, c, B or T, times, stream, baseline, stale
    assert check("grad", arrays=False, grad_gp=False) == "bad arguments"
    assert check("grad", grad_gp=False, c=0).startswith("grad_gp == NULL")
    assert check("value", c=0, B=0) == "number of components must be 1, 2 or 3"
    assert check("value", B=0, have_times=False) == "batch size outside [1, max_batch]"
    assert check("fisher", have_times=False, open_stream=True) == "call psoap_chunk_set_times first"
    assert check("fisher", open_stream=True, have_baseline=False) == "the handle has an open stream (psoap_stream_close first)"
    assert check("fisher", have_baseline=False, stale_weight=True) == "call psoap_chunk_set_baseline first"


def test_the_messages_are_those_of_the_entries_it_combines():
    """times and stream in the words of the time-variable checks, the baseline in those of psoap_chunk_lnlike_marg; the
    time-variable entries keep the refusal of a handle with a baseline that existing tests pin"""
    plan = open(os.path.join(ROOT, "psoap_amd", "csrc", "predict_plan.hpp")).read()
    assert '"call psoap_chunk_set_times first"' in plan and '"the handle has an open stream (psoap_stream_close first)"' in plan
    assert plan.count("is not built yet") == 2
    src = open(os.path.join(ROOT, "psoap_amd", "csrc", "psoap_gp.hip")).read()
    assert 'FAIL("psoap_chunk_lnlike_marg: call psoap_chunk_set_baseline first")' in src
    assert STALE in src.replace('"\n             "', "")
    assert src.count("marginalised continuum is not built yet") == 1
    for entry in ("psoap_chunk_lnlike_marg_tv", "psoap_chunk_lnlike_marg_tv_grad", "psoap_chunk_fisher_marg_tv"):
        assert f'extern "C" int {entry}(' in src and f'std::string("{entry}: ") + why' in src


def test_ctypes_declarations_and_python_layers():
    import ctypes
    import inspect
    from psoap_amd import _lib, covariance
    from psoap_amd.chunk import ChunkHandle
    res, args = _lib.SIGNATURES["psoap_chunk_lnlike_marg_tv"]
    assert res is ctypes.c_int and len(args) == 12 and args[6] is ctypes.c_double and args.count(_lib._dp) == 8
    res, args = _lib.SIGNATURES["psoap_chunk_lnlike_marg_tv_grad"]
    assert res is ctypes.c_int and len(args) == 13 and args[6] is ctypes.c_double and args.count(_lib._dp) == 9
    res, args = _lib.SIGNATURES["psoap_chunk_fisher_marg_tv"]
    assert (res, args) == _lib.SIGNATURES["psoap_chunk_fisher_tv"]
    header = open(os.path.join(ROOT, "include", "psoap_gp.h")).read()
    for entry in ("psoap_chunk_lnlike_marg_tv", "psoap_chunk_lnlike_marg_tv_grad", "psoap_chunk_fisher_marg_tv"):
        assert f"int {entry}(" in header
    assert all(callable(getattr(ChunkHandle, n)) for n in ("lnlike_marg_tv", "lnlike_marg_tv_grad", "fisher_marg_tv"))
    for name in ("lnlike_timevar_grad", "fisher_information_timevar", "timevar_laplace"):
        assert inspect.signature(getattr(covariance, name)).parameters["baseline"].default is None, name
    # the two whose parameter lists are fixed have a marginal twin that takes the baseline after ``times``
    assert list(inspect.signature(covariance.lnlike_timevar_marginal).parameters) == [
        "lwls", "fl", "sigma", "gp", "tau", "times", "baseline", "mu_GP"]
    assert list(inspect.signature(covariance.optimize_GP_timevar_marginal).parameters) == [
        "lwls", "fl", "sigma", "gp0", "tau0", "times", "baseline", "free_tau", "mu_GP", "ftol", "full_output"]
    for name in ("lnlike_timevar", "optimize_GP_timevar", "loo_timevar", "predict_timevar"):
        assert "baseline" not in inspect.signature(getattr(covariance, name)).parameters, name
    with pytest.raises(ValueError, match="baseline needs"):
        covariance.lnlike_timevar_marginal(np_zeros(1, 4), np_zeros(4), np_zeros(4) + 1.0, [1.0, 1.0], [1.0], np_zeros(4), {"order": 1})
    with pytest.raises(ValueError, match="baseline needs"):
        covariance.optimize_GP_timevar_marginal(np_zeros(1, 4), np_zeros(4), np_zeros(4) + 1.0, [1.0, 1.0], [1.0], np_zeros(4),
                                                {"order": 1})


def np_zeros(*shape):
    import numpy as np
    return np.zeros(shape)


def test_marg_tv_check_runs_clean_under_sanitizers_and_matches_the_restatement(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    exe = str(tmp_path / "marg_tv_host_check")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True,
                        cwd=str(tmp_path))
    assert cc.returncode == 0, cc.stderr
    if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        assert cc.stderr == "", cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    assert run.stdout.splitlines() == expected()
