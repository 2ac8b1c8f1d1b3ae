"""The host twin of the row-granular clip (psoap_sky_clip16, psoap_amd/csrc/plan_abi.hpp) built by a host compiler alone
into tests/host/sky_fine_host_check.cpp, with AddressSanitizer and UBSan, and run as a child process: a clean run over its
grid of cases, and every line it prints reproduced by the same call through ctypes into libpsoap_gp.so (the hipcc build
of the same headers)."""
import ctypes
import os
import struct
import subprocess

import pytest

from psoap_amd import _lib
from test_plan_host import FLAGS, ROOT, _splitmix, fnv1a, host_compiler

SOURCE = os.path.join(ROOT, "tests", "host", "sky_fine_host_check.cpp")


def sky_inputs(c, B, N, kind, seed):
    """sky_fine_host_check.cpp's sky_inputs, operation for operation"""
    base, s, step = [], seed, 4e-6
    for i in range(N):
        s, u = _splitmix(s)
        unit = float(u >> 11) / 9007199254740992.0
        at = i // 8 * 8 if kind == 1 else i
        x = 8.5 + step * float(at)
        if kind != 1:
            x = x + 0.2 * step * unit
        base.append(x)
    lwl, gp = [], []
    for b in range(B):
        for k in range(c):
            for i in range(N):
                x = base[i] + 2e-5 * k * float(i % 3 - 1)
                lwl.append(x + 1e-6 * b)
            gp += [1.0 + 0.25 * k, 6.0 + k - 1.5 * b]
    if kind == 2:
        nan = struct.unpack("<d", struct.pack("<Q", 0x7ff8000000000000))[0]
        lwl[N // 2] = nan
        if B > 1:
            lwl[(1 * c + (c - 1)) * N] = nan
    return (ctypes.c_double * len(lwl))(*lwl), (ctypes.c_double * len(gp))(*gp)


def library_line(L, name, p):
    lwl, gp = sky_inputs(p["c"], p["B"], p["N"], p["kind"], p["seed"])
    rows = (ctypes.c_int * (p["B"] * ((p["N"] + 127) // 128)))()
    count, cand = ctypes.c_longlong(-9), ctypes.c_int(-9)
    if name == "sky_clip":
        assert L.psoap_sky_clip(p["c"], p["N"], p["B"], lwl, gp, rows, ctypes.byref(count), ctypes.byref(cand)) == 0
        return f"cand={cand.value} units={count.value} first_b={fnv1a(rows)}"
    assert name == "sky_clip16", name
    assert L.psoap_sky_clip16(p["c"], p["N"], p["B"], lwl, gp, rows, ctypes.byref(count), ctypes.byref(cand)) == 0
    return f"cand={cand.value} stages={count.value} first16_b={fnv1a(rows)}"


def test_the_twin_runs_clean_under_sanitizers_and_matches_the_library(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    exe = str(tmp_path / "sky_fine_host_check")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True,
                        cwd=str(tmp_path))
    assert cc.returncode == 0, cc.stderr
    if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        assert cc.stderr == "", cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    lines = run.stdout.splitlines()
    assert {ln.split()[0] for ln in lines} == {"sky_clip", "sky_clip16"} and len(lines) == 2 * 3 * 2 * 7 * 3
    L = _lib.load()
    wrong, units, narrowed = [], {}, 0
    for ln in lines:
        head, tail = ln.split(" : ")
        name, *kv = head.split()
        p = {k: int(v) for k, v in (x.split("=") for x in kv)}
        again = library_line(L, name, p)
        if again != tail:
            wrong.append((ln, again))
        # the two twins of one case: the stages never exceed 8 per unit
        count = int(tail.split()[1].split("=")[1])
        if name == "sky_clip":
            units[tuple(kv)] = count
        else:
            assert count <= 8 * units[tuple(kv)], ln
            narrowed += count < 8 * units[tuple(kv)]
    assert not wrong, f"{len(wrong)} of {len(lines)} lines differ, the first: program {wrong[0][0]!r}, library {wrong[0][1]!r}"
    assert narrowed > 0, "no case of the grid starts a column inside its first tile"
