"""The pure-host part of the quasi-periodic entry (psoap_amd/csrc/qp_plan.hpp: ``qp_check``, the refusals of
psoap_chunk_lnlike_qp_grad, and ``qp_refused``, the values of Gamma and P that are no proposal) built by a host compiler alone
into tests/host/qp_host_check.cpp, with AddressSanitizer and UBSan, and run as a child process, the way
tests/test_share_host.py runs its program.  The program checks the invariants; this file checks that it leaves clean and what
it says: every refusal in the words of psoap_chunk_lnlike_tv_grad.  No GPU."""
import os
import subprocess

import pytest

from test_plan_host import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "qp_host_check.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

VALUE_ONLY = "grad_gp == NULL asks for the value only: grad_tau, grad_gamma, grad_period, grad_lwl and grad_mu must be NULL too"
GO_WITH = "grad_tau, grad_gamma and grad_period go with grad_gp"
EXPECTED = {
    "full": "ok",
    "no-optional": "ok",
    "value-only": "ok",
    "no-arrays": "bad arguments",
    "value-with-temporal": VALUE_ONLY,
    "value-with-rest": VALUE_ONLY,
    "no-grad-tau": GO_WITH,
    "no-grad-gamma": GO_WITH,
    "no-grad-period": GO_WITH,
    "B0": "B must be at least 1",
    "c0": "number of components must be 1, 2 or 3",
    "c4": "number of components must be 1, 2 or 3",
    "no-times": "call psoap_chunk_set_times first",
    "open-stream": "the handle has an open stream (psoap_stream_close first; psoap_chunk_set_times refuses one too)",
    "baseline": "the handle has a baseline (psoap_chunk_set_baseline): the quasi-periodic kernel under the marginalised continuum "
                "is not built",
}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    where = tmp_path_factory.mktemp("qp_host")
    exe = str(where / "qp_host_check")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True,
                        cwd=str(where))
    assert cc.returncode == 0, cc.stderr
    if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        assert cc.stderr == "", cc.stderr
    return exe


def test_refusals_and_invalid_values_on_the_host_under_sanitizers(program, tmp_path):
    run = subprocess.run([program], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    said = dict(line.split(" : ", 1) for line in run.stdout.splitlines())
    assert said == EXPECTED


def test_the_words_are_those_of_the_time_variable_entry_and_the_library_uses_the_check():
    """the refusals a time-variable call shares are spelled as psoap_chunk_lnlike_tv_grad spells them, and the entry in
    psoap_gp.hip goes through qp_check and grad_run, with qp_refused deciding -inf in analysis_host.hpp"""
    csrc = os.path.join(ROOT, "psoap_amd", "csrc")
    with open(os.path.join(csrc, "psoap_gp.hip")) as fh:
        hip = fh.read()
    with open(os.path.join(csrc, "analysis_host.hpp")) as fh:
        runs = fh.read()
    with open(os.path.join(csrc, "qp_plan.hpp")) as fh:
        plan = fh.read()
    for name in ("B0", "no-times", "open-stream"):
        assert f'"psoap_chunk_lnlike_tv_grad: {EXPECTED[name]}' in hip, name
    entry = hip[hip.index('extern "C" int psoap_chunk_lnlike_qp_grad'):]
    entry = entry[:entry.index("\n}\n")]
    assert "qp_check(call)" in entry and "grad_run(" in entry and "&qp)" in entry
    assert "qp_refused(qp->gamma, qp->period, c, b)" in runs
    assert "hip/" not in plan and "hip_runtime" not in plan
