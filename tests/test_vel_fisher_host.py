"""The host-only part of the epoch-velocity Fisher information (psoap_amd/csrc/vel_fisher_plan.hpp: the epoch bins of every
tile row, the tile lists, the workspace size, the refusals) built by a host compiler alone into
tests/host/vel_fisher_host_check.cpp, with AddressSanitizer and UBSan, and run as a child process: a clean run -- the program
checks its own invariants -- and the lines it prints against a plain-Python twin of the binning rule and against
psoap_vel_fisher_plan through ctypes.  Then the boundary: the entry points are declared in include/psoap_gp.h, bound in
psoap_amd._lib.SIGNATURES with the declared argument lists, exported by the built library and reachable from Python."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_plan_host import FLAGS, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "vel_fisher_host_check.cpp")
NAMES = ("psoap_chunk_fisher_vel", "psoap_chunk_fisher_vel_release", "psoap_vel_fisher_plan")
NB = 128


def _cases():
    """the epoch indices of the program's cases, by the same rules"""
    scattered, s = [], 12345
    for _ in range(400):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        scattered.append((s >> 8) % 140)
    return {"equal": (2, 6, [i // 50 for i in range(300)]),
            "unequal": (3, 8, [e for e, n in enumerate((7, 121, 1, 0, 130, 41)) for _ in range(n)]),
            "one": (1, 1, [0] * 128),
            "plus-one": (2, 2, [0] * 128 + [1]),
            "descending": (2, 5, [4 - i // 52 for i in range(260)]),
            "scattered": (3, 140, scattered)}


def _twin(c, E, ep):
    """(P, first, slot epochs, bytes): the distinct epochs of every 128-row tile row, ascending"""
    N = len(ep)
    P = (N + NB - 1) // NB
    rows = [sorted(set(ep[q * NB:(q + 1) * NB])) for q in range(P)]
    first = [0]
    for r in rows:
        first.append(first[-1] + len(r))
    S, Npad = first[-1], P * NB
    ints = Npad + (P + 1) + 2 * S + (E + 1) + 2 * P * P + P * (P + 1)
    nbytes = 8 * ((1 + 2 * c) * Npad * Npad + c * (c + 1) // 2 * S * S + (c * E) ** 2) + 4 * ints
    return P, first, [e for r in rows for e in r], nbytes


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    tmp = tmp_path_factory.mktemp("vel_fisher_host")
    exe = str(tmp / "vel_fisher_host_check")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True,
                        cwd=str(tmp))
    assert cc.returncode == 0, cc.stderr
    if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        assert cc.stderr == "", cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    return run.stdout.splitlines()


def test_plan_against_the_python_twin(lines):
    assert "limits : NB 128 VEL_MAX_EPOCHS 2048" in lines
    plans = [ln for ln in lines if ln.startswith("plan ")]
    assert len(plans) == len(_cases())
    for ln in plans:
        head, tail = ln.split(" : ")
        name = head.split()[1]
        c, E, ep = _cases()[name]
        P, first, epochs, nbytes = _twin(c, E, ep)
        assert head == f"plan {name} c={c} N={len(ep)} E={E}"
        parts = tail.split(" | ")
        assert parts[0] == f"P {P} S {first[-1]} max {max(b - a for a, b in zip(first, first[1:]))}"
        assert parts[1] == "first " + " ".join(str(v) for v in first)
        assert parts[2] == "epochs " + " ".join(str(v) for v in epochs[:24])
        assert parts[3] == f"tiles {P * P} {P * (P + 1) // 2}"
        assert parts[4] == f"bytes {nbytes}"


def test_library_twin_returns_the_same_plan(lines):
    from psoap_amd import _lib
    L = _lib.load()
    i32 = ctypes.POINTER(ctypes.c_int32)
    for name, (c, E, ep) in _cases().items():
        P, first, epochs, nbytes = _twin(c, E, ep)
        N = len(ep)
        epa = np.array(ep, dtype=np.int32)
        S, na, nu, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        slot_of, sf, se = (ctypes.c_int * N)(), (ctypes.c_int * (P + 1))(), (ctypes.c_int * len(epochs))()
        assert L.psoap_vel_fisher_plan(c, N, E, epa.ctypes.data_as(i32), ctypes.byref(S), slot_of, sf, se, len(epochs),
                                       ctypes.byref(na), ctypes.byref(nu), ctypes.byref(nb)) == 0
        assert (S.value, na.value, nu.value, nb.value) == (first[-1], P * P, P * (P + 1) // 2, nbytes)
        assert list(sf) == first and list(se) == epochs
        assert all(epochs[slot_of[i]] == ep[i] and first[i // NB] <= slot_of[i] < first[i // NB + 1] for i in range(N))
        assert L.psoap_vel_fisher_plan(c, N, E, epa.ctypes.data_as(i32), None, None, None, None, 0, None, None, None) == 0
    epa = np.zeros(10, dtype=np.int32)
    epa[4] = 2
    for c, N, E, msg in ((0, 10, 3, b"number of components"), (2, 0, 3, b"the chunk has no pixel"), (2, 10, 0, b"n_epochs must be at least 1"),
                         (2, 10, 2049, b"n_epochs must be at most 2048"), (2, 10, 2, b"epoch index out of range")):
        assert L.psoap_vel_fisher_plan(c, N, E, epa.ctypes.data_as(i32), None, None, None, None, 0, None, None, None) == 2
        err = L.psoap_last_error()
        assert err.startswith(b"psoap_vel_fisher_plan: ") and msg in err, err


def test_refusals(lines):
    got = dict(ln[len("check "):].split(" : ") for ln in lines if ln.startswith("check "))
    assert len(got) == 11
    assert {k for k, v in got.items() if v == "accepted"} == {"ok", "E-limit"}
    assert got["c0"] == got["c4"] == "number of components must be 1, 2 or 3"
    assert got["N0"] == "the chunk has no pixel"
    assert got["E0"] == got["E-neg"] == "n_epochs must be at least 1"
    assert got["E-huge"] == "n_epochs must be at most 2048"
    assert got["null"] == "bad arguments"
    assert got["index-high"] == got["index-neg"] == "epoch index out of range"


def _declaration(name):
    text = open(os.path.join(ROOT, "include", "psoap_gp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/psoap_gp.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entry_points_are_declared_bound_and_exported():
    from psoap_amd import _lib, build
    L = ctypes.CDLL(build.build())
    dp, vp, ip = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)
    as_ctype = {"psoap_chunk *": vp, "int": ctypes.c_int, "const double *": dp, "double *": dp, "int *": ip,
                "const int32_t *": ctypes.POINTER(ctypes.c_int32), "long long *": ctypes.POINTER(ctypes.c_longlong)}
    for name in NAMES:
        assert hasattr(L, name), f"{name} is not exported by libpsoap_gp.so"
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        assert [as_ctype[re.sub(r"\s*\w+$", "", a).strip()] for a in _declaration(name)] == list(argtypes), name
    assert [len(_declaration(n)) for n in NAMES] == [7, 1, 12]


def test_python_surface_exists():
    from psoap_amd import covariance, lnprob
    from psoap_amd.chunk import ChunkHandle
    assert list(inspect.signature(ChunkHandle.fisher_vel).parameters) == ["self", "lwls", "gp", "epoch_index", "n_epochs"]
    assert hasattr(ChunkHandle, "fisher_vel_release")
    assert list(inspect.signature(covariance.velocity_information).parameters) == ["lwls", "fl", "sigma", "gp", "epoch_index"]
    assert list(inspect.signature(lnprob.ChunkWorker.fisher_vel_at).parameters) == ["self", "vel", "p_gp"]
    assert list(inspect.signature(lnprob.ChunkWorker.lnlike_grad_vel).parameters) == ["self", "vel", "p_gp", "mu_GP"]
    sig = inspect.signature(lnprob.epoch_velocities)
    assert list(sig.parameters)[:4] == ["workers", "p", "max_iter", "tol"]
    assert (sig.parameters["max_iter"].default, sig.parameters["tol"].default) == (20, 1e-10)
    assert "fixed hyper-parameters" in lnprob.epoch_velocities.__doc__.lower() and hasattr(lnprob.EpochVelocities, "write_table")


def test_null_handle_is_refused_without_a_device():
    from psoap_amd import _lib
    L = _lib.load()
    assert L.psoap_chunk_fisher_vel(None, 2, None, None, 3, None, None) == 2
    assert L.psoap_last_error() == b"psoap_chunk_fisher_vel: bad arguments"
    assert L.psoap_chunk_fisher_vel_release(None) == 2
    assert L.psoap_last_error() == b"null handle"      # (as psoap_chunk_fisher_release answers)
