"""The pure-host part of the gradient of the continuum-marginalised likelihood (psoap_amd/csrc/marg_grad_plan.hpp: the layout
of [K | I | Ht], first rows, the launches of every block row, the group size, argument validation) built by a host compiler alone
into tests/host/marg_grad_host_check.cpp, with AddressSanitizer and UBSan, and run as a child process: a clean run -- the
program checks its own invariants -- and every line it prints reproduced by the restatement below."""
import os
import subprocess

import pytest

from test_plan_host import FLAGS, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "marg_grad_host_check.cpp")
NB = 128


def plan(rs, n_epochs, order):
    """marg_grad_plan.hpp (on marg_plan.hpp) restated: -> the text behind " : " of the program's line"""
    epoch = [e for e, n in rs for _ in range(n)]
    N = len(epoch)
    P = (N + NB - 1) // NB
    start = {}
    for i, e in enumerate(epoch):
        start.setdefault(e, i)
    q = n_epochs * (order + 1)
    Q = (q + NB - 1) // NB
    first = [P] * Q
    for e, s in start.items():
        for t in range(e * (order + 1) // NB, (e * (order + 1) + order) // NB + 1):
            first[t] = min(first[t], s // NB)
    column = sorted(range(Q), key=lambda t: (first[t], t))
    slot = [column.index(t) for t in range(Q)]
    cols = [(P + j, j) for j in range(P)] + [(2 * P + slot[t], first[t]) for t in range(Q)]
    rows = []
    for p in range(P):
        act = sum(f <= p for f in first)
        rows.append((P + 1 if p else 0, act if p else 0, P, act))
    fmt = lambda rws: "".join(" (" + ",".join(str(v) for v in r) + ")" for r in rws)      # noqa: E731
    return f"ld {NB * (2 * P + Q)} | cols{fmt(cols)} | rows{fmt(rows)}"


EXPECTED = [
    ("a", [(0, 25), (1, 25), (2, 25), (3, 25)], 4, 1),
    ("b", [(0, 64), (1, 64)], 2, 0),
    ("c", [(0, 43), (1, 43), (2, 43)], 3, 2),
    ("d", [(0, 128), (1, 128), (2, 128)], 3, 3),
    ("e", [(2, 120), (0, 100), (3, 80)], 4, 1),
    ("f", [(e, 12) for e in range(26)], 26, 4),
    ("shuffled", [(e, 100) for e in range(8, 12)] + [(e, 50) for e in range(8)], 12, 15),
    ("hollow", [(0, 200), (20, 1)], 21, 7),
]
REFUSALS = [
    "ok : accepted",
    "B0 : B must be at least 1",
    "c0 : number of components must be 1, 2 or 3",
    "c4 : number of components must be 1, 2 or 3",
    "unset : call psoap_chunk_set_baseline first",
    "stale : psoap_chunk_set_data changed the data the baseline's weights were given for (psoap_chunk_set_baseline again)",
]


def test_restatement_by_hand():
    """case f (N = 312: P = 3, Q = 2): I at tile columns 3 .. 5, H's first tile column (first row 0) at 6, its second (the
    last two columns of epoch 25, rows 300 ..: block row 2) at 7; block row 1 updates 4 + 1 tiles and solves 3 + 1, block row 2
    takes the second slot too.  "shuffled" (P = 7): columns 0 .. 127 start at block row 3 and take slot 1, tile column 15."""
    assert plan(EXPECTED[5][1], 26, 4) == ("ld 1024 | cols (3,0) (4,1) (5,2) (6,0) (7,2) | rows (0,0,3,1) (4,1,3,1) (4,2,3,2)")
    assert " (15,3) (14,0) | rows (0,0,7,1) (8,1,7,1) (8,1,7,1) (8,2,7,2)" in plan(EXPECTED[6][1], 12, 15)
    assert plan(EXPECTED[0][1], 4, 1) == "ld 384 | cols (1,0) (2,0) | rows (0,0,1,1)"


def test_the_refusals_are_those_of_the_marginal_likelihood():
    """the two messages about the baseline are the ones psoap_chunk_lnlike_marg gives"""
    src = open(os.path.join(ROOT, "psoap_amd", "csrc", "psoap_gp.hip")).read()
    assert 'FAIL("psoap_chunk_lnlike_marg: call psoap_chunk_set_baseline first")' in src
    tail = REFUSALS[5].split(" : ")[1]
    joined = src.replace('"\n             "', "")
    assert tail in joined


def test_marg_grad_plan_runs_clean_under_sanitizers_and_matches_the_restatement(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    exe = str(tmp_path / "marg_grad_host_check")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True,
                        cwd=str(tmp_path))
    assert cc.returncode == 0, cc.stderr
    if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        assert cc.stderr == "", cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    lines = run.stdout.splitlines()
    assert len(lines) == len(EXPECTED) + len(REFUSALS)
    for ln, (name, rs, ne, order) in zip(lines, EXPECTED):
        N = sum(n for _, n in rs)
        assert ln == f"{name} N={N} n_epochs={ne} order={order} : {plan(rs, ne, order)}", ln
    assert lines[len(EXPECTED):] == REFUSALS
