"""The planner and the pure-host entry points of the C ABI (psoap_amd/csrc/plan_abi.hpp, dag_plan.hpp, sky_rules.hpp) built
by a host compiler alone into tests/host/plan_host_check.cpp, with AddressSanitizer and UBSan, and run as a child process:
a clean run over its grid of cases, and every line it prints -- the counts and FNV-1a hashes of every output array --
reproduced by the same call through ctypes into libpsoap_gp.so (the hipcc build of the same headers)."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import pytest

from psoap_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "plan_host_check.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all"]
M64 = 0xFFFFFFFFFFFFFFFF


def host_compiler():
    """CXX, else the clang++ beside hipcc, else g++; None: no host compiler here"""
    if os.environ.get("CXX"):
        return shutil.which(os.environ["CXX"].split()[0])
    hipcc = shutil.which(build.hipcc())
    if hipcc:
        dirs = [os.path.dirname(os.path.realpath(hipcc))]
        try:
            out = subprocess.run([hipcc, "--version"], capture_output=True, text=True, timeout=60).stdout
            dirs += re.findall(r"InstalledDir:\s*(\S+)", out)
        except (OSError, subprocess.TimeoutExpired):
            pass
        for d in dirs:
            if os.path.exists(os.path.join(d, "clang++")):
                return os.path.join(d, "clang++")
    return shutil.which("g++")


def fnv1a(data):
    h = 0xcbf29ce484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001b3) & M64
    return "%016x" % h


class DagTask(ctypes.Structure):     # 16 bytes (dag_task.hpp)
    _fields_ = [("bytes", ctypes.c_ubyte * 16)]


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _list_outputs(call):
    """A task-list entry point called as the program calls it: once for the count, once into buffers of that size.
    call(out, max_tasks, n_tasks, n_slots, n_ctrs, queue_first) -> status"""
    n, ns, nc = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
    assert call(None, 0, ctypes.byref(n), None, None, None) == 0
    tasks = (DagTask * n.value)()
    qf = (ctypes.c_uint32 * 9)()
    assert call(tasks, n.value, ctypes.byref(n), ctypes.byref(ns), ctypes.byref(nc), qf) == 0
    return n.value, ns.value, nc.value, qf, tasks


def _fmt_list(n, ns, nc, qf, tasks):
    s = f"n_tasks={n} n_slots={ns} n_ctrs={nc}"
    if qf is not None:
        s += f" queue_first={fnv1a(qf)}"
    return s + f" tasks={fnv1a(tasks)}"


def _splitmix(s):
    s = (s + 0x9E3779B97F4A7C15) & M64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return s, z ^ (z >> 31)


def sky_inputs(c, B, N, kind, seed):
    """plan_host_check.cpp's sky_inputs, operation for operation"""
    base, s = [], seed
    for _ in range(N):
        s, u = _splitmix(s)
        unit = float(u >> 60) / 16.0 if kind == 1 else float(u >> 11) / 9007199254740992.0
        base.append(8.5 + 0.1 * unit)
    lwl, gp = [], []
    for b in range(B):
        for k in range(c):
            for i in range(N):
                x = base[i] + 2e-3 * k * float(i % 3 - 1)
                lwl.append(x + 1e-4 * b)
            gp += [1.0 + 0.25 * k, 4.0 + k + 0.5 * b]
    if kind == 2:
        nan = struct.unpack("<d", struct.pack("<Q", 0x7ff8000000000000))[0]
        lwl[N // 2] = nan
        if B > 1:
            lwl[(1 * c + (c - 1)) * N] = nan
    return (ctypes.c_double * len(lwl))(*lwl), (ctypes.c_double * len(gp))(*gp)


def library_line(L, name, p):
    """The text behind " : " of the program's line for entry point `name` with the parameters p, from the library"""
    if name == "plan":
        return _fmt_list(*_list_outputs(lambda *a: L.psoap_dag_plan(p["B"], p["P"], p["workers"], *a)))
    if name == "plan_sky":
        first = _ints([max(j - p["width"], 0) if p["width"] > 0 else 0 for j in range(p["P"])])
        return _fmt_list(*_list_outputs(lambda *a: L.psoap_dag_plan_sky(p["B"], p["P"], first, p["workers"], *a)))
    if name == "plan_multi":
        return _fmt_list(*_list_outputs(lambda *a: L.psoap_dag_plan_multi(len(p["Ps"]), _ints(p["Ps"]), p["workers"], *a)))
    if name == "plan_aug":
        return _fmt_list(*_list_outputs(
            lambda *a: L.psoap_dag_plan_aug(p["P"], p["Mt"], p["Ms"], p["workers"], p["scheme"], *a)))
    if name == "stream_plan":
        so = ctypes.c_int(-9)
        n, ns, nc, _, tasks = _list_outputs(
            lambda out, mx, n, ns, nc, qf: L.psoap_stream_plan(p["P"], p["lanes"], p["workers"], p["scheme"], out, mx, n, ns, nc,
                                                               ctypes.byref(so) if out is not None else None))
        return f"scheme_out={so.value} " + _fmt_list(n, ns, nc, None, tasks)
    if name == "pick_workers":
        w = ctypes.c_int(-9)
        assert L.psoap_dag_pick_workers(p["B"], _ints([p["P"]] * p["B"]), p["Mt"], p["compute_units"], p["max_workers"],
                                        ctypes.byref(w)) == 0
        return f"workers={w.value}"
    if name in ("sky_first", "sky_order"):
        lwl, gp = sky_inputs(p["c"], p["B"], p["N"], p["kind"], p["seed"])
        first, perm, cand = (ctypes.c_int * ((p["N"] + 127) // 128))(), (ctypes.c_int * p["N"])(), ctypes.c_int(-9)
        if name == "sky_first":
            assert L.psoap_sky_first(p["c"], p["N"], p["B"], lwl, gp, first, perm) == 0
            return f"first={fnv1a(first)} perm={fnv1a(perm)}"
        assert L.psoap_sky_order(p["c"], p["N"], p["B"], lwl, gp, first, perm, ctypes.byref(cand)) == 0
        return f"cand={cand.value} first={fnv1a(first)} perm={fnv1a(perm)}"
    raise AssertionError(f"unknown entry point in the program's output: {name}")


def library_lines(L, lines):
    """Every line of the program's output, made again through the library"""
    out = []
    for ln in lines:
        head = ln.split(" : ")[0].split()
        p = {k: ([int(x) for x in v.split(",")] if k == "Ps" else int(v)) for k, v in (kv.split("=") for kv in head[1:])}
        out.append(ln.split(" : ")[0] + " : " + library_line(L, head[0], p))
    return out


def test_planner_runs_clean_under_sanitizers_and_matches_the_library(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    exe = str(tmp_path / "plan_host_check")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True,
                        cwd=str(tmp_path))
    assert cc.returncode == 0, cc.stderr
    # (g++ reports the `#pragma clang fp contract(off)` lines of sky_rules.hpp as unknown pragmas -- -ffp-contract=off above
    # does their work for it; under clang the compile is silent)
    if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        assert cc.stderr == "", cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    lines = run.stdout.splitlines()
    names = {ln.split()[0] for ln in lines}
    assert names == {"plan", "plan_sky", "plan_multi", "plan_aug", "stream_plan", "pick_workers", "sky_first", "sky_order"}
    again = library_lines(_lib.load(), lines)
    wrong = [(a, b) for a, b in zip(lines, again) if a != b]
    assert not wrong, f"{len(wrong)} of {len(lines)} lines differ, the first: program {wrong[0][0]!r}, library {wrong[0][1]!r}"
