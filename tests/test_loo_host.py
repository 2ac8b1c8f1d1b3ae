"""The pure-host part of leave-one-out cross-validation (psoap_amd/csrc/loo_plan.hpp: the contiguity check, the packed-block
offsets, the band tile list) built by a host compiler alone into tests/host/loo_host_check.cpp, with AddressSanitizer and
UBSan, and run as a child process: a clean run -- the program checks its own invariants -- and every line it prints
reproduced by the restatement below."""
import os
import subprocess

import pytest

from test_plan_host import FLAGS, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "loo_host_check.cpp")
NB = 128


def _pad(n):
    return (n + NB - 1) // NB * NB


def layout(epoch, N, n_epochs):
    """loo_plan.hpp restated: -> the text behind " : " of the program's line"""
    if epoch is None:
        n_epochs = _pad(N) // NB
        epoch = [i // NB for i in range(N)]
    if n_epochs < 1:
        return "refused: n_epochs must be at least 1"
    start, count = {}, {}
    for i, e in enumerate(epoch):
        if e < 0 or e >= n_epochs:
            return "refused: epoch index out of range"
        if e not in count:
            start[e], count[e] = i, 0
        elif start[e] + count[e] != i:
            return "refused: the pixels of an epoch are not contiguous"
        count[e] += 1
    order = sorted(count, key=lambda e: (_pad(count[e]), e))
    blocks, groups, off, rhs, wt = [], [], 0, 0, 0
    for k, e in enumerate(order):
        side = _pad(count[e])
        blocks.append((e, start[e], count[e], side, off, rhs, wt))
        if not groups or groups[-1][0] != side:
            groups.append([side, k, 0])
        groups[-1][2] += 1
        off, rhs, wt = off + side * side, rhs + side, wt + side // NB * NB * NB
    tiles = set()
    for e in count:
        t0, t1 = start[e] // NB, (start[e] + count[e] - 1) // NB
        tiles |= {(ti, tj) for ti in range(t0, t1 + 1) for tj in range(ti, t1 + 1)}
    fmt = lambda rows: "".join(" (" + ",".join(str(v) for v in r) + ")" for r in rows)      # noqa: E731
    return f"blocks{fmt(blocks)} | groups{fmt(groups)} | tiles{fmt(sorted(tiles))} | doubles {off} {rhs} {wt}"


def runs(*pairs):
    return [e for e, n in pairs for _ in range(n)]


EXPECTED = [
    ("a", runs((0, 25), (1, 25), (2, 25), (3, 25)), 100, 4),
    ("b", runs((0, 128)), 128, 1),
    ("c", runs((0, 128), (1, 1)), 129, 2),
    ("d", runs((0, 128), (1, 128), (2, 128)), 384, 3),
    ("e", runs((0, 1), (1, 299), (3, 130), (4, 270)), 700, 5),
    ("f", runs((2, 100), (0, 100), (1, 100)), 300, 3),
    ("null", None, 700, 6),
    ("null", None, 128, 1),
    ("ones", [129 - i for i in range(130)], 130, 130),
    ("whole", [0] * 1000, 1000, 1),
    ("split", runs((0, 10), (1, 10), (0, 1)), 21, 2),
    ("range", runs((0, 10), (2, 10)), 20, 2),
    ("negative", runs((0, 10), (-1, 1)), 11, 2),
    ("none", runs((0, 10)), 10, 0),
]


def test_case_e_by_hand():
    """the restatement itself on case e: pixel 0 | 1..299 | 300..429 | 430..699 -> sides 128, 384, 256, 384; the 299-pixel epoch
    spans tiles 0..2, the 130-pixel one tiles 2..3, the 270-pixel one tiles 3..5"""
    line = layout(EXPECTED[4][1], 700, 5)
    assert "blocks (0,0,1,128,0,0,0) (3,300,130,256,16384,128,16384) (1,1,299,384,81920,384,49152) (4,430,270,384,229376,768,98304)" in line
    assert "groups (128,0,1) (256,1,1) (384,2,2)" in line
    assert "tiles (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) (2,3) (3,3) (3,4) (3,5) (4,4) (4,5) (5,5) |" in line


def test_loo_layout_runs_clean_under_sanitizers_and_matches_the_restatement(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    exe = str(tmp_path / "loo_host_check")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True,
                        cwd=str(tmp_path))
    assert cc.returncode == 0, cc.stderr
    if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        assert cc.stderr == "", cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    lines = run.stdout.splitlines()
    assert len(lines) == len(EXPECTED)
    for ln, (name, epoch, N, ne) in zip(lines, EXPECTED):
        assert ln == f"{name} N={N} n_epochs={ne} : {layout(epoch, N, ne)}", ln      # (no index: the tile count is shown)
    refused = [ln.split(" : ")[1] for ln in lines if "refused" in ln]
    assert refused == ["refused: the pixels of an epoch are not contiguous", "refused: epoch index out of range",
                       "refused: epoch index out of range", "refused: n_epochs must be at least 1"]
