"""The skyline-aware list rules (psoap_amd/csrc/dag_plan.hpp, PSOAP_SKY_SPLIT) built by a host compiler alone into
tests/host/sky_split_host_check.cpp, with AddressSanitizer and UBSan, and run as a child process: a clean run over its grid of
envelopes with the rules on and off, and every line it prints reproduced by the same call into libpsoap_gp.so."""
import os
import subprocess

import pytest

from psoap_amd import _lib
from test_plan_host import FLAGS, ROOT, _fmt_list, _ints, _list_outputs, host_compiler

SOURCE = os.path.join(ROOT, "tests", "host", "sky_split_host_check.cpp")


def envelope(P, kind):
    """sky_split_host_check.cpp's envelope()"""
    out = []
    for j in range(P):
        cap = max(j - 1, 0)
        v = (j - P // 2, j - 2, cap, j - max(P // 2, 1), 0 if j < P // 2 else P // 2 - 1)[kind]
        out.append(min(max(v, 0), cap))
    return out


def test_the_rules_run_clean_under_sanitizers_and_match_the_library(tmp_path, monkeypatch):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    exe = str(tmp_path / "sky_split_host_check")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True,
                        cwd=str(tmp_path))
    assert cc.returncode == 0, cc.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("PSOAP_")}
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path), env=env)
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    lines = run.stdout.splitlines()
    assert len(lines) >= 300 and {ln.split()[0] for ln in lines} == {"plan_sky"}
    for name in [k for k in os.environ if k.startswith("PSOAP_")]:
        monkeypatch.delenv(name)
    L = _lib.load()
    differ = 0
    for ln in lines:
        head, text = ln.split(" : ")
        p = {k: int(v) for k, v in (kv.split("=") for kv in head.split()[1:])}
        monkeypatch.setenv("PSOAP_SKY_SPLIT", str(p["split"]))
        first = _ints(envelope(p["P"], p["kind"]))
        got = _fmt_list(*_list_outputs(lambda *a: L.psoap_dag_plan_sky(p["B"], p["P"], first, p["workers"], *a)))
        assert got == text, (head, got, text)
        differ += p["split"] == 1 and text != dict(l.split(" : ") for l in lines)[head.replace("split=1", "split=0")]
    assert differ > 0, "the rules change some list of the grid"
