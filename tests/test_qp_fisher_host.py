"""The pure-host part of psoap_chunk_fisher_qp and psoap_chunk_loo_qp (psoap_amd/csrc/qp_plan.hpp: ``fisher_qp_check``,
``loo_qp_check`` and the workspace arithmetic ``fisher_qp_sizes``) built by a host compiler alone into
tests/host/qp_fisher_host_check.cpp, with AddressSanitizer and UBSan, and run as a child process, the way tests/test_qp_host.py
runs its program.  The program checks the invariants -- among them that every refusal but the baseline's is the time-variable
twin's word for word; this file checks that it leaves clean and what it says.  No GPU."""
import os
import subprocess

import pytest

from test_plan_host import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "qp_fisher_host_check.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

BAD, COMPONENTS = "bad arguments", "number of components must be 1, 2 or 3"
TANGENTS, TIMES = "the number of tangents must be between 1 and 32", "call psoap_chunk_set_times first"
STREAM = "the handle has an open stream (psoap_stream_close first)"
BASELINE = ("the handle has a baseline (psoap_chunk_set_baseline): the quasi-periodic kernel under the marginalised continuum is "
            "not built")
EXPECTED = {
    "fisher-good": "ok", "fisher-T1": "ok", "fisher-T32": "ok",
    "fisher-no-arrays": BAD, "fisher-c0": COMPONENTS, "fisher-c4": COMPONENTS, "fisher-T0": TANGENTS, "fisher-T33": TANGENTS,
    "fisher-no-times": TIMES, "fisher-open-stream": STREAM, "fisher-baseline": BASELINE,
    "fisher-order-c-before-T": COMPONENTS, "fisher-order-T-before-times": TANGENTS, "fisher-order-times-before-stream": TIMES,
    "fisher-order-stream-before-baseline": STREAM,
    "loo-good": "ok", "loo-no-arrays": BAD, "loo-c0": COMPONENTS, "loo-c4": COMPONENTS, "loo-no-times": TIMES,
    "loo-open-stream": STREAM, "loo-baseline": BASELINE,
}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    where = tmp_path_factory.mktemp("qp_fisher_host")
    exe = str(where / "qp_fisher_host_check")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True,
                        cwd=str(where))
    assert cc.returncode == 0, cc.stderr
    if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        assert cc.stderr == "", cc.stderr
    return exe


def test_refusals_and_sizes_on_the_host_under_sanitizers(program, tmp_path):
    run = subprocess.run([program], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    said = dict(line.split(" : ", 1) for line in run.stdout.splitlines())
    assert said == EXPECTED


def test_the_library_uses_the_checks_and_the_sizes():
    """the entries in psoap_gp.hip go through fisher_qp_check / loo_qp_check and the runs with their quasi-periodic argument;
    fisher_run sizes the tile records by fisher_qp_sizes with the record length the host program assumes; qp_refused decides NaN"""
    csrc = os.path.join(ROOT, "psoap_amd", "csrc")
    with open(os.path.join(csrc, "psoap_gp.hip")) as fh:
        hip = fh.read()
    with open(os.path.join(csrc, "analysis_host.hpp")) as fh:
        runs = fh.read()
    with open(os.path.join(csrc, "qp_plan.hpp")) as fh:
        plan = fh.read()
    for name, check, run in (("psoap_chunk_fisher_qp", "fisher_qp_check(", "fisher_run("), ("psoap_chunk_loo_qp", "loo_qp_check(", "loo_run(")):
        entry = hip[hip.index(f'extern "C" int {name}('):]
        entry = entry[:entry.index("\n}\n")]
        assert check in entry and run in entry and "&qp)" in entry, name
    assert "fisher_qp_sizes(c, N, P, T, QpTile::DOUBLES).part" in runs
    assert "static_assert(QpTile::DOUBLES == 6 * 128 + 3 * 5" in hip
    assert runs.count("qp_refused(qp->gamma, qp->period, c, 0)") == 2
    assert "hip/" not in plan and "hip_runtime" not in plan
