"""The host-only part of the posterior draws (psoap_amd/csrc/draw_rng.hpp: the Philox4x32-10 core of the generator;
draw_plan.hpp: the layout, the block rows of the factorisation, the tiles and K-loops of the triangular product, the argument
check) built by a host compiler alone into tests/host/draw_host_check.cpp, with AddressSanitizer and UBSan, and run as a child
process: a clean run -- the program checks its own invariants -- the counter blocks bit for bit those of the plain-Python
restatement (tests/draw_reference.py) and of psoap_draw_philox through ctypes, and the plan that of a brute-force enumeration."""
import ctypes
import os
import re
import subprocess

import pytest

import draw_reference as dr
from test_plan_host import FLAGS, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "draw_host_check.cpp")
NB = 128


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    tmp = tmp_path_factory.mktemp("draw_host")
    exe = str(tmp / "draw_host_check")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True,
                        cwd=str(tmp))
    assert cc.returncode == 0, cc.stderr
    if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        assert cc.stderr == "", cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    return run.stdout.splitlines()


def _philox_lines(lines):
    out = []
    for ln in lines:
        if ln.startswith("philox "):
            head, tail = ln.split(" : ")
            p = {k: int(v) for k, v in (kv.split("=") for kv in head.split()[1:])}
            words, ints = tail.split(" | ")
            out.append((p, tuple(int(w, 16) for w in words.split()), tuple(int(v) for v in ints.split())))
    return out


def test_the_two_python_forms_agree_and_meet_the_known_answer():
    """the plain-integer form and the NumPy form of the restatement, and the published vector for a zero counter and key"""
    assert dr.philox4x32_10((0, 0, 0, 0), (0, 0)) == dr.KAT_ZERO
    for seed, d in ((0, 0), (0x123456789abcdef0, 3), (2 ** 64 - 1, 2 ** 32 - 1)):
        pairs = [0, 1, 63, 64, 131071, 2 ** 32 - 1]
        w = dr.blocks(seed, pairs, d)
        for k, p in enumerate(pairs):
            assert tuple(int(v) for v in w[:, k]) == dr.block(seed, p, d)


def test_counter_blocks_match_the_restatement_bit_for_bit(lines):
    kat = [ln for ln in lines if ln.startswith("kat : ")]
    assert len(kat) == 1 and tuple(int(w, 16) for w in kat[0].split(" : ")[1].split()) == dr.KAT_ZERO
    got = _philox_lines(lines)
    assert len(got) == 5 * 6 * 4
    assert {p["seed"] for p, _, _ in got} == {0, 1, 0x123456789abcdef0, 2 ** 64 - 1, 0x1ffffffff}
    for p, words, ints in got:
        want = dr.block(p["seed"], p["pair"], p["draw"])
        assert words == want, p
        assert ints == (dr.bits53(want[0], want[1]), dr.bits53(want[2], want[3])), p


def test_library_twin_returns_the_same_blocks(lines):
    from psoap_amd import _lib
    L = _lib.load()
    out = (ctypes.c_uint * 4)()
    for p, words, _ in _philox_lines(lines):
        assert L.psoap_draw_philox(ctypes.c_ulonglong(p["seed"]), p["pair"], p["draw"], out) == 0
        assert tuple(out) == words, p
    assert L.psoap_draw_philox(ctypes.c_ulonglong(0), 0, 0, None) == 2
    assert b"psoap_draw_philox" in L.psoap_last_error()


def test_plan_against_brute_force(lines):
    plans = [ln for ln in lines if ln.startswith("plan ")]
    assert len(plans) == 15
    seen = set()
    for ln in plans:
        head, tail = ln.split(" : ")
        R, D = (int(kv.split("=")[1]) for kv in head.split()[1:])
        seen.add((R, D))
        Rt, Dt = (R + NB - 1) // NB, (D + NB - 1) // NB
        parts = tail.split(" | ")
        assert parts[0] == f"ld {NB * (Rt + Dt)}"
        rows = [tuple(int(v) for v in m) for m in re.findall(r"\((\d+),(\d+)\)", parts[1])]
        assert rows == [((Rt - p) if p else 0, Rt - p - 1) for p in range(Rt)]
        tiles = [tuple(int(v) for v in m) for m in re.findall(r"\((\d+),(\d+),(\d+)\)", parts[2])]
        pairs = [(td, tj, k) for td, tj, kb in tiles for k in range(kb)]
        # every (tile, k-block) pair with k <= tj exactly once, none with k > tj
        assert sorted(pairs) == sorted((td, tj, k) for td in range(Dt) for tj in range(Rt) for k in range(tj + 1))
        assert len(set(pairs)) == len(pairs) and all(k <= tj for _, tj, k in pairs)
        # the long K-loops are handed out first
        assert [kb for _, _, kb in tiles] == sorted((kb for _, _, kb in tiles), reverse=True)
        assert parts[3] == f"doubles {NB * Rt * NB * (Rt + Dt)} {NB * Dt * NB * Rt}"
        upd = sum(p * (Rt - p) for p in range(1, Rt))
        assert parts[4] == f"units {upd:.1f} {Dt * Rt * (Rt + 1) / 2:.1f}"
    assert seen == {(R, D) for R in (1, 127, 128, 129, 257) for D in (1, 128, 129)}


def test_argument_check(lines):
    got = [ln[len("check "):] for ln in lines if ln.startswith("check ")]
    no_sigma = ("no predict call has formed Sigma on this handle (psoap_chunk_predict or psoap_chunk_predict_marg with "
                "Sigma_out first)")
    assert got == ["ok : accepted", "ok-zero : accepted", "no-sigma : " + no_sigma, "D0 : D must be at least 1",
                   "D-neg : D must be at least 1", "D-huge : D must be at most 1048576",
                   "nugget-neg : nugget must be finite and >= 0", "nugget-inf : nugget must be finite and >= 0",
                   "nugget-nan : nugget must be finite and >= 0"]
