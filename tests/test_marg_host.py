"""The pure-host part of the continuum-marginalised likelihood (psoap_amd/csrc/marg_plan.hpp: validation, the column layout,
first non-zero rows, the order of the appended tile columns, Gram tiles, the abscissa map) built by a host compiler alone into
tests/host/marg_host_check.cpp, with AddressSanitizer and UBSan, and run as a child process: a clean run -- the program checks
its own invariants -- and every line it prints reproduced by the restatement below."""
import os
import subprocess

import pytest

from test_plan_host import FLAGS, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "marg_host_check.cpp")
NB = 128


def runs(*pairs):
    return list(pairs)


def plan(rs, n_epochs, order, sd=None):
    """marg_plan.hpp restated: -> the text behind " : " of the program's line"""
    import math
    epoch = [e for e, n in rs for _ in range(n)]
    x = [8.5 + 1e-5 * i for _, n in rs for i in range(n)]
    N = len(epoch)
    if order < 0 or order > 15:
        return "refused: order must lie in [0, 15]"
    if n_epochs < 1:
        return "refused: n_epochs must be at least 1"
    if (order + 1) * n_epochs > 1024:
        return "refused: (order + 1) n_epochs must not exceed 1024"
    sd = [1.0] * (order + 1) if sd is None else sd
    if any(not (s > 0.0) or math.isinf(s) for s in sd):
        return "refused: prior_sd must be finite and positive"
    P = (N + NB - 1) // NB
    start, count = {}, {}
    for i, e in enumerate(epoch):
        if e < 0 or e >= n_epochs:
            return "refused: epoch index out of range"
        if e not in count:
            start[e], count[e] = i, 0
        elif start[e] + count[e] != i:
            return "refused: the pixels of an epoch are not contiguous"
        count[e] += 1
    q = n_epochs * (order + 1)
    Q = (q + NB - 1) // NB
    first = [P] * Q
    eps = []
    for e in range(n_epochs):
        c0 = e * (order + 1)
        if e not in count:
            eps.append((c0, 0, 0, 0.0, 0.0))
            continue
        xs = x[start[e]:start[e] + count[e]]
        a, b = min(xs), max(xs)
        off, scl = ((-b - a) / (b - a), 2.0 / (b - a)) if b > a else (0.0, 0.0)
        eps.append((c0, start[e], count[e], off, scl))
        for t in range(c0 // NB, (c0 + order) // NB + 1):
            first[t] = min(first[t], start[e] // NB)
    column = sorted(range(Q), key=lambda t: (first[t], t))
    slot = [column.index(t) for t in range(Q)]
    active = [sum(f <= p for f in first) for p in range(P)]
    tiles = [(ti, tj, slot[ti], slot[tj], NB * max(first[ti], first[tj])) for ti in range(Q) for tj in range(ti, Q)]
    fmt = lambda rows: "".join(" (" + ",".join(str(v) for v in r) + ")" for r in rows)      # noqa: E731
    g17 = lambda v: "%.17g" % v      # noqa: E731
    return (f"q {q} Q {Q} | first{fmt(zip(first, slot))} | active{''.join(' %d' % a for a in active)} | tiles{fmt(tiles)} | "
            f"epochs{fmt((c0, s, n, g17(o), g17(k)) for c0, s, n, o, k in eps)}")


EXPECTED = [
    ("a", runs((0, 25), (1, 25), (2, 25), (3, 25)), 4, 1, None),
    ("b", runs((0, 64), (1, 64)), 2, 0, None),
    ("c", runs((0, 43), (1, 43), (2, 43)), 3, 2, None),
    ("d", runs((0, 128), (1, 128), (2, 128)), 3, 3, None),
    ("e", runs((2, 120), (0, 100), (3, 80)), 4, 1, None),
    ("f", runs(*[(e, 12) for e in range(26)]), 26, 4, None),
    ("shuffled", runs(*[(e, 100) for e in range(8, 12)], *[(e, 50) for e in range(8)]), 12, 15, None),
    ("hollow", runs((0, 200), (20, 1)), 21, 7, None),
    ("single", runs((0, 1)), 1, 0, None),
    ("order-", runs((0, 10)), 1, -1, None),
    ("order+", runs((0, 10)), 1, 16, None),
    ("wide", runs((0, 10)), 257, 3, None),
    ("sd0", runs((0, 10)), 1, 1, [1.0, 0.0]),
    ("sdnan", runs((0, 10)), 1, 1, [float("nan"), 1.0]),
    ("sdinf", runs((0, 10)), 1, 0, [float("inf")]),
    ("split", runs((0, 10), (1, 10), (0, 1)), 2, 1, None),
    ("range", runs((0, 10), (2, 10)), 2, 1, None),
    ("negative", runs((0, 10), (-1, 1)), 2, 1, None),
    ("none", runs((0, 10)), 0, 1, None),
]


def test_restatement_by_hand():
    """case e: rows 0..119 epoch 2, 120..219 epoch 0, 220..299 epoch 3 -> one tile column that starts at block row 0; case f:
    q = 130, the second tile column holds the last two columns of epoch 25 (rows 300..311: block row 2); "shuffled": columns
    0..127 (epochs 0..7) start at row 400, block row 3, columns 128..191 at row 0 -- the second tile column takes slot 0"""
    assert plan(EXPECTED[4][1], 4, 1).startswith("q 8 Q 1 | first (0,0) | active 1 1 1 | tiles (0,0,0,0,0) | epochs (0,120,100,")
    assert plan(EXPECTED[5][1], 26, 4).startswith(
        "q 130 Q 2 | first (0,0) (2,1) | active 1 1 2 | tiles (0,0,0,0,0) (0,1,0,1,256) (1,1,1,1,256) |")
    assert plan(EXPECTED[6][1], 12, 15).startswith(
        "q 192 Q 2 | first (3,1) (0,0) | active 1 1 1 2 2 2 2 | tiles (0,0,1,1,384) (0,1,1,0,384) (1,1,0,0,0) |")
    assert " | first (0,0) (1,1) | " in plan(EXPECTED[7][1], 21, 7) and "(8,0,0,0,0)" in plan(EXPECTED[7][1], 21, 7)
    assert plan(EXPECTED[8][1], 1, 0).endswith("epochs (0,0,1,0,0)")


def test_marg_plan_runs_clean_under_sanitizers_and_matches_the_restatement(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    exe = str(tmp_path / "marg_host_check")
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
    for ln, (name, rs, ne, order, sd) in zip(lines, EXPECTED):
        N = sum(n for _, n in rs)
        assert ln == f"{name} N={N} n_epochs={ne} order={order} : {plan(rs, ne, order, sd)}", ln
    refused = [ln.split(" : ")[1] for ln in lines if "refused" in ln]
    assert refused == ["refused: order must lie in [0, 15]", "refused: order must lie in [0, 15]",
                       "refused: (order + 1) n_epochs must not exceed 1024"] + 3 * ["refused: prior_sd must be finite and positive"] + \
        ["refused: the pixels of an epoch are not contiguous", "refused: epoch index out of range",
         "refused: epoch index out of range", "refused: n_epochs must be at least 1"]
