"""The pure-host part of the prediction under the marginalised continuum (psoap_amd/csrc/marg_predict_plan.hpp: the layout
of [K | Cx^T | Ht], first rows, the launches of every block row of both factorisations, the Gram and Sigma tiles, the
workspace bytes, argument validation) built by a host compiler alone into tests/host/marg_predict_host_check.cpp, with
AddressSanitizer and UBSan, and run as a child process: a clean run -- the program checks its own invariants -- and every
line it prints reproduced by the restatement below."""
import os
import subprocess

import pytest

from test_plan_host import FLAGS, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "marg_predict_host_check.cpp")
NB = 128


def plan(rs, n_epochs, order, mode, c, M):
    """marg_predict_plan.hpp (on marg_plan.hpp) restated: -> the text behind " : " of the program's line"""
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
    R = c * M if mode == 0 else M
    Rt = (R + NB - 1) // NB
    cols = [(P + j, 0) for j in range(Rt)] + [(P + Rt + slot[t], first[t]) for t in range(Q)]
    rows = []
    for p in range(P):
        n = P - p + Rt + sum(f <= p for f in first)
        rows.append((n if p else 0, n - 1))
    mrows = [((Q - p + Rt) if p else 0, Q - p - 1 + Rt) for p in range(Q)]
    gram = [(ti, tj, P + Rt + slot[ti], P + Rt + slot[tj], NB * max(first[ti], first[tj]), int(ti == tj))
            for ti in range(Q) for tj in range(ti, Q)]
    gram += [(t, Q + j, P + Rt + slot[t], P + j, NB * first[t], 0) for t in range(Q) for j in range(Rt)]
    ld, ldm = NB * (P + Rt + Q), NB * (Q + Rt)
    fmt = lambda rws: "".join(" (" + ",".join(str(v) for v in r) + ")" for r in rws)      # noqa: E731
    return (f"ld {ld} | cols{fmt(cols)} | rows{fmt(rows)} | ldm {ldm} | mrows{fmt(mrows)} | gram{fmt(gram)} | "
            f"sigma {Rt} {Rt * (Rt + 1) // 2} | bytes {8 * NB * P * ld} {8 * NB * Q * ldm} {8 * (NB * Rt) ** 2}")


RUNS = {
    "a": ([(0, 25), (1, 25), (2, 25), (3, 25)], 4, 1),
    "b": ([(0, 64), (1, 64)], 2, 0),
    "c": ([(0, 43), (1, 43), (2, 43)], 3, 2),
    "d": ([(0, 128), (1, 128), (2, 128)], 3, 3),
    "e": ([(2, 120), (0, 100), (3, 80)], 4, 1),
    "f": ([(e, 12) for e in range(26)], 26, 4),
    "shuffled": ([(e, 100) for e in range(8, 12)] + [(e, 50) for e in range(8)], 12, 15),
    "hollow": ([(0, 200), (20, 1)], 21, 7),
}
# (name, chunk, mode, c, M): the cases of tests/marg_predict_reference.py, then the two layouts of test_marg_grad_host
EXPECTED = [("a", "a", 0, 2, 50), ("a1", "a", 1, 2, 130), ("b", "b", 2, 1, 128), ("c", "c", 0, 2, 65), ("d", "d", 2, 1, 129),
            ("e", "e", 0, 3, 43), ("f", "f", 0, 2, 100), ("shuffled", "shuffled", 0, 2, 100), ("hollow", "hollow", 0, 3, 50)]
_STALE = "psoap_chunk_set_data changed the data the baseline's weights were given for (psoap_chunk_set_baseline again)"
REFUSALS = [
    "ok : accepted",
    "ok-sum : accepted",
    "ok-f : accepted",
    "mode3 : bad arguments",
    "c4 : bad arguments",
    "M0 : bad arguments",
    "f-c2 : mode 2 (predict_f) needs c == 1",
    "sum-c3 : mode 1 with three components is not provided (the transposed mean of predict_f_g_h_sum, covariance.py:294)",
    "sum-c1 : mode 1 (the sum) needs c == 2",
    "comp-c1 : mode 0 (the components) needs c == 2 or 3",
    "unset : call psoap_chunk_set_baseline first",
    "stale : " + _STALE,
]


def test_the_cases_are_those_of_the_reference():
    import marg_predict_reference as mp
    import marg_reference as mr
    for (name, chunk, mode, c, M), pc in zip(EXPECTED, mp.PCASES):
        case = mr.case_named(pc[0])
        assert (chunk, mode, M, c) == (pc[0], pc[1], pc[2], case[2])
        assert (list(case[4]), case[3], case[5]) == (RUNS[chunk][0], RUNS[chunk][1], RUNS[chunk][2])


def test_restatement_by_hand():
    """case f (N = 312: P = 3, Q = 2; R = 200: Rt = 2): Cx^T at tile columns 3 and 4, H's first tile column (first row 0) at 5,
    its second (the last two columns of epoch 25, rows 300 ..: block row 2) at 6.  Block row 0 solves 2 + 2 + 1 tiles, block
    row 1 updates 2 + 2 + 1 and solves 4, block row 2 takes the second slot too.  [M | G] has 3 + 4 tiles; the K loops of
    those in H's second tile column start at row 256."""
    text = plan(*RUNS["f"], 0, 2, 100)
    assert text.startswith("ld 896 | cols (3,0) (4,0) (5,0) (6,2) | rows (0,5) (5,4) (5,4) | ldm 512 | mrows (0,3) (3,2) | gram "
                           "(0,0,5,5,0,1) (0,1,5,6,256,0) (1,1,6,6,256,1) (0,2,5,3,0,0) (0,3,5,4,0,0) (1,2,6,3,256,0) (1,3,6,4,256,0) | "
                           "sigma 2 3 | bytes ")
    assert plan(*RUNS["a"], 0, 2, 50) == ("ld 384 | cols (1,0) (2,0) | rows (0,2) | ldm 256 | mrows (0,1) | gram (0,0,2,2,0,1) "
                                          f"(0,1,2,1,0,0) | sigma 1 1 | bytes {8 * 128 * 384} {8 * 128 * 256} {8 * 128 * 128}")
    # "shuffled" (P = 7, Rt = 2): columns 0 .. 127 of H start at block row 3 and take slot 1, tile column 10 -- block row 3
    # has one tile of K fewer than block row 2 and one slot more
    assert " (10,3) (9,0) | rows (0,9) (9,8) (8,7) (8,7) (7,6) (6,5) (5,4) | ldm" in plan(*RUNS["shuffled"], 0, 2, 100)


def test_the_refusals_are_those_of_the_marginal_likelihood():
    """the two messages about the baseline are the ones psoap_chunk_lnlike_marg gives"""
    src = open(os.path.join(ROOT, "psoap_amd", "csrc", "psoap_gp.hip")).read()
    assert 'FAIL("psoap_chunk_lnlike_marg: call psoap_chunk_set_baseline first")' in src
    assert _STALE in src.replace('"\n             "', "")


def test_marg_predict_plan_runs_clean_under_sanitizers_and_matches_the_restatement(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    exe = str(tmp_path / "marg_predict_host_check")
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
    for ln, (name, chunk, mode, c, M) in zip(lines, EXPECTED):
        rs, ne, order = RUNS[chunk]
        N = sum(n for _, n in rs)
        assert ln == f"{name} N={N} n_epochs={ne} order={order} mode={mode} c={c} M={M} : {plan(rs, ne, order, mode, c, M)}", ln
    assert lines[len(EXPECTED):] == REFUSALS
