"""The host-only part of the mixture moments (psoap_amd/csrc/mix_plan.hpp: the padding, the upper tiles of the rank-S product,
the bytes of the buffers, the argument checks) built by a host compiler alone into tests/host/mix_host_check.cpp, with
AddressSanitizer and UBSan, and run as a child process: a clean run -- the program checks its own invariants -- and every line
it prints against the plain-Python twin of the padding rules (tests/mix_reference.py) and against psoap_mix_plan through
ctypes.  Then the boundary: the five entry points are declared in include/psoap_gp.h, bound in psoap_amd._lib.SIGNATURES with
the declared argument lists, exported by the built library and reachable from Python, and the argument checks that need no
device answer 2 with their message."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

import mix_reference as mr
from test_plan_host import FLAGS, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "mix_host_check.cpp")
NAMES = ("psoap_chunk_mix_begin", "psoap_chunk_mix_add", "psoap_chunk_mix_finish", "psoap_chunk_mix_release", "psoap_mix_plan")
NO_MIX = ("no mixture on this handle (psoap_chunk_mix_begin first; psoap_chunk_set_data, psoap_chunk_set_baseline and "
          "psoap_chunk_mix_release end one)")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    tmp = tmp_path_factory.mktemp("mix_host")
    exe = str(tmp / "mix_host_check")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True,
                        cwd=str(tmp))
    assert cc.returncode == 0, cc.stderr
    if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        assert cc.stderr == "", cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    return run.stdout.splitlines()


def _plans(lines):
    out = []
    for ln in lines:
        if ln.startswith("plan "):
            head, tail = ln.split(" : ")
            R, S, want = (int(kv.split("=")[1]) for kv in head.split()[1:])
            out.append((R, S, want, tail.split(" | ")))
    return out


def test_plan_against_the_python_twin(lines):
    assert f"limits : NB {mr.NB} KB {mr.KB} MIX_MAX_S {mr.MIX_MAX_S} MIX_MAX_R {mr.MIX_MAX_R}" in lines
    plans = _plans(lines)
    assert {(R, S) for R, S, _, _ in plans} == {(R, S) for R in (1, 127, 128, 129, 256, 3072)
                                                for S in (1, mr.KB - 1, mr.KB, mr.KB + 1, mr.MIX_MAX_S)}
    assert len(plans) == 60
    for R, S, want, parts in plans:
        Rp, Sp = mr.rpad(R), mr.spad(S)
        Rt = Rp // mr.NB
        assert parts[0] == f"Rpad {Rp} Spad {Sp} Rt {Rt}"
        tiles = mr.upper_tiles(Rt) if want else []
        if Rt <= 3:
            assert [tuple(int(v) for v in m) for m in re.findall(r"\((\d+),(\d+)\)", parts[1])] == tiles
        else:
            assert parts[1] == f"tiles {len(tiles)}"
        r2 = Rp * Rp
        assert parts[2] == f"doubles {r2 if want else Rp} {r2 if want else 0} {Sp * Rp} {Sp + 3 * Rp + 1}"
        assert parts[3] == f"bytes {mr.plan_bytes(R, S, want)}"


def test_library_twin_returns_the_same_plan(lines):
    from psoap_amd import _lib
    L = _lib.load()
    for R, S, want, parts in _plans(lines):
        Rp, Sp, nt, nbytes = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        assert L.psoap_mix_plan(R, S, want, ctypes.byref(Rp), ctypes.byref(Sp), ctypes.byref(nt), None, 0, ctypes.byref(nbytes)) == 0
        Rt = mr.rpad(R) // mr.NB
        assert (Rp.value, Sp.value, nbytes.value) == (mr.rpad(R), mr.spad(S), mr.plan_bytes(R, S, want))
        assert nt.value == (Rt * (Rt + 1) // 2 if want else 0)
        if want:
            buf = (ctypes.c_int * (2 * nt.value))()
            assert L.psoap_mix_plan(R, S, want, None, None, None, buf, nt.value, None) == 0
            assert list(zip(buf[0::2], buf[1::2])) == mr.upper_tiles(Rt)
    for R, S, want, msg in ((0, 4, 1, b"the prediction must have at least 1 row"), (mr.MIX_MAX_R + 1, 4, 1, b"at most 32768 rows"),
                            (128, 0, 1, b"S_max must be at least 1"), (128, mr.MIX_MAX_S + 1, 0, b"S_max must be at most 4096"),
                            (128, 4, 2, b"want_sigma must be 0")):
        assert L.psoap_mix_plan(R, S, want, None, None, None, None, 0, None) == 2
        err = L.psoap_last_error()
        assert err.startswith(b"psoap_mix_plan: ") and msg in err, err


def test_argument_checks(lines):
    got = dict(ln[len("check "):].split(" : ") for ln in lines if ln.startswith("check "))
    assert len(got) == 8 + 12 + 9 + 6
    accepted = {k for k, v in got.items() if v == "accepted"}
    assert accepted == {"plan ok", "plan S-limit", "begin ok", "begin ok-marg-var", "begin R-mode1", "add ok", "add ok-last",
                        "finish ok", "finish ok-var"}
    assert got["plan R0"] == "the prediction must have at least 1 row"
    assert got["plan R-huge"] == got["begin R-huge"] == "the prediction must have at most 32768 rows"
    assert got["plan S0"] == got["plan S-neg"] == got["begin S0"] == "S_max must be at least 1"
    assert got["plan S-huge"] == got["begin S-huge"] == "S_max must be at most 4096"
    assert got["plan sigma2"] == "want_sigma must be 0 (variances only) or 1 (full Sigma)"
    assert got["begin null"] == got["add null"] == got["finish null"] == "bad arguments"
    assert got["begin marg2"] == "marg must be 0 (the plain conditional) or 1 (under the marginalised continuum)"
    assert got["begin mode3"] == got["begin c4"] == got["begin M0"] == "mode must be 0, 1 or 2, c 1 .. 3 and M at least 1"
    assert got["begin mode2-c2"] == "mode 2 (predict_f) needs c == 1"
    assert got["add no-begin"] == got["finish no-begin"] == NO_MIX
    assert got["add w0"] == got["add w-neg"] == got["add w-inf"] == got["add w-nan"] == "weight must be finite and > 0"
    assert got["add full"] == "the mixture already holds S_max samples"
    assert got["finish sigma-in-var"] == "Sigma_out must be NULL in the variance-only mode (want_sigma = 0 at psoap_chunk_mix_begin)"
    assert got["finish empty"] == "no sample has been folded yet"


def _declaration(name):
    text = open(os.path.join(ROOT, "include", "psoap_gp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/psoap_gp.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_mix_entry_points_are_declared_bound_and_exported():
    from psoap_amd import _lib, build
    L = ctypes.CDLL(build.build())
    dp, vp, ip = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)
    as_ctype = {"psoap_chunk *": vp, "int": ctypes.c_int, "double": ctypes.c_double, "const double *": dp, "double *": dp,
                "int *": ip, "long long *": ctypes.POINTER(ctypes.c_longlong)}
    for name in NAMES:
        assert hasattr(L, name), f"{name} is not exported by libpsoap_gp.so"
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        assert [as_ctype[re.sub(r"\s*\w+$", "", a).strip()] for a in _declaration(name)] == list(argtypes), name
    assert [len(_declaration(n)) for n in NAMES] == [9, 5, 7, 1, 9]


def test_python_surface_exists():
    from psoap_amd import covariance, retrieve
    from psoap_amd.chunk import ChunkHandle
    assert list(inspect.signature(ChunkHandle.mix_begin).parameters) == ["self", "mode", "lwls_predict", "mu_c", "s_max", "want_sigma",
                                                                          "marg"]
    assert list(inspect.signature(ChunkHandle.mix_add).parameters) == ["self", "lwls", "gp", "weight"]
    assert hasattr(ChunkHandle, "mix_finish") and hasattr(ChunkHandle, "mix_release")
    sig = inspect.signature(covariance.predict_mixture)
    assert list(sig.parameters) == ["lwls_list", "fl", "sigma", "lwls_predict", "mus", "gps", "weights", "mode", "baseline",
                                    "want_sigma", "draws_per_sample", "seed", "nugget"]
    assert [sig.parameters[k].default for k in ("weights", "mode", "baseline", "want_sigma", "draws_per_sample", "seed", "nugget")] == \
        [None, 0, None, True, 0, None, 1e-8]
    sig = inspect.signature(retrieve.retrieve_posterior)
    assert list(sig.parameters) == ["model", "chunk", "parameters", "flatchain", "fix_params", "n_samples", "thin_seed",
                                    "n_pix_predict", "get_Sigma", "baseline", "draws_per_sample", "seed"]
    assert (sig.parameters["n_samples"].default, sig.parameters["thin_seed"].default) == (64, 0)
    assert "ONE grid" in retrieve.retrieve_posterior.__doc__


def test_null_handle_is_refused_without_a_device():
    from psoap_amd import _lib
    L = _lib.load()
    st = ctypes.c_int(0)
    assert L.psoap_chunk_mix_begin(None, 0, 0, 2, 64, None, None, 4, 1) == 2
    assert L.psoap_last_error() == b"psoap_chunk_mix_begin: bad arguments"
    assert L.psoap_chunk_mix_add(None, None, None, 1.0, ctypes.byref(st)) == 2
    assert L.psoap_last_error() == b"psoap_chunk_mix_add: bad arguments"
    assert L.psoap_chunk_mix_finish(None, None, None, None, None, None, None) == 2
    assert L.psoap_last_error() == b"psoap_chunk_mix_finish: bad arguments"
    assert L.psoap_chunk_mix_release(None) == 2
    assert L.psoap_last_error() == b"psoap_chunk_mix_release: null handle"
