"""The pure-host part of the predict family (psoap_amd/csrc/predict_plan.hpp: argument validation, the shape of
[B | Cx^T], the layout of the pinned staging block, the sentinel rows of the persistent launch, prior means and variances,
the flop count) built by a host compiler alone into tests/host/predict_host_check.cpp, with AddressSanitizer and UBSan, and
run as a child process: a clean run -- the program checks its own invariants and the values written out by hand in it -- and
every line it prints reproduced by the restatement below."""
import os
import subprocess

import pytest

from test_plan_host import FLAGS, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "predict_host_check.cpp")
NB = 128
MU0 = 0.25
_SUM3 = "predict_f_g_h_sum is only defined for len(lwl_predict) == len(lwl) (covariance.py:294)"


def up(n):
    return (n + NB - 1) // NB * NB


def shape(mode, c, N, M):
    """predict_plan.hpp's predict_check and predict_shape restated: -> the text behind " : " of the program's line"""
    if not (0 <= mode <= 2 and 1 <= c <= 3 and N > 0 and M > 0):
        return "psoap_predict: bad arguments"
    if mode == 2 and c != 1:
        return "psoap_predict: mode 2 (predict_f) needs c == 1"
    transposed = mode == 1 and c == 3
    if transposed and M != N:
        return _SUM3
    Npad, Rq, Rx = up(N), (c * M if mode == 0 else M), (N if transposed else 0)
    P, Rtot = Npad // NB, up(Rq) + up(Rx)
    offset = 1.0 if mode == 0 or (mode == 1 and c == 2) else MU0
    return (f"Npad {Npad} P {P} Rq {Rq} Rq_pad {up(Rq)} Rx {Rx} Rx_pad {up(Rx)} Rtot_pad {Rtot} ld {Npad + Rtot} Mt {Rtot // NB} "
            f"nslab {(Npad + 255) // 256} offset {offset:.2f} transposed {int(transposed)} dag {int(not transposed and P + Rtot // NB <= 255)}")


# (name, mode, c, N, M): the cases of the exact pin, the edge shapes of test_gpu_parity.py, the edge of the persistent launch,
# the refusals
EXPECTED = [("c", 0, 2, 129, 65), ("a-sum", 1, 2, 100, 130), ("b", 2, 1, 128, 128), ("f", 0, 2, 312, 100),
            ("transposed", 1, 3, 129, 129), ("one-point", 2, 1, 74, 1), ("one-point-joint", 0, 1, 74, 1),
            ("four-column-tiles", 0, 3, 252, 129), ("dag-255", 2, 1, 128 * 250, 128 * 5), ("dag-256", 2, 1, 128 * 250 + 1, 128 * 5),
            ("sum-of-three-M", 1, 3, 129, 100), ("mode3", 3, 1, 10, 10), ("c4", 0, 4, 10, 10), ("N0", 0, 2, 0, 10), ("M0", 0, 2, 10, 0),
            ("f-c2", 2, 2, 10, 10)]


def test_the_cases_are_those_of_the_pin():
    import marg_predict_reference as mp
    import marg_reference as mr
    have = {(mode, c, N, M) for _, mode, c, N, M in EXPECTED}
    for name, mode in (("c", 0), ("a", 1), ("b", 2), ("f", 0)):
        pc, = [p for p in mp.PCASES if p[:2] == (name, mode)]
        case = mr.case_named(name)
        assert (mode, case[2], mr.case_chunk(case).lwls.shape[1], pc[2]) in have


def test_restatement_by_hand():
    """case c (N = 129: two block rows; R = 130: two tile columns): rows of 512 doubles.  The sum of three on its own grid
    carries a second block of N columns for the transposed mean and never takes the persistent launch.  250 + 5 tile columns
    are the last the 8-bit indices of the persistent launch hold."""
    assert shape(0, 2, 129, 65) == ("Npad 256 P 2 Rq 130 Rq_pad 256 Rx 0 Rx_pad 0 Rtot_pad 256 ld 512 Mt 2 nslab 1 offset 1.00 "
                                    "transposed 0 dag 1")
    assert shape(1, 3, 129, 129) == ("Npad 256 P 2 Rq 129 Rq_pad 256 Rx 129 Rx_pad 256 Rtot_pad 512 ld 768 Mt 4 nslab 1 offset 0.25 "
                                     "transposed 1 dag 0")
    assert shape(2, 1, 74, 1).startswith("Npad 128 P 1 Rq 1 Rq_pad 128 Rx 0 Rx_pad 0 Rtot_pad 128 ld 256 Mt 1 nslab 1 offset 0.25")
    assert shape(0, 3, 252, 129).startswith("Npad 256 P 2 Rq 387 Rq_pad 512 ")
    assert shape(2, 1, 32000, 640).endswith("dag 1") and shape(2, 1, 32001, 640).endswith("dag 0")


def test_the_messages_are_the_librarys():
    """what psoap_last_error gives for a refused plain predict call comes from predict_plan.hpp alone"""
    plan = open(os.path.join(ROOT, "psoap_amd", "csrc", "predict_plan.hpp")).read()
    for msg in ("psoap_predict: bad arguments", "psoap_predict: mode 2 (predict_f) needs c == 1", _SUM3):
        assert f'"{msg}"' in plan
    for name in ("predict_host.hpp", "predict_kernels.hpp"):
        src = open(os.path.join(ROOT, "psoap_amd", "csrc", name)).read()
        assert "psoap_predict: bad arguments" not in src and _SUM3 not in src


def test_predict_plan_runs_clean_under_sanitizers_and_matches_the_restatement(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    exe = str(tmp_path / "predict_host_check")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True,
                        cwd=str(tmp_path))
    assert cc.returncode == 0, cc.stderr
    if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        assert cc.stderr == "", cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    lines = run.stdout.splitlines()
    assert len(lines) == len(EXPECTED) + 1
    for ln, (name, mode, c, N, M) in zip(lines, EXPECTED):
        assert ln == f"{name} mode={mode} c={c} N={N} M={M} : {shape(mode, c, N, M)}", ln
    assert lines[-1] == "no-arrays : psoap_predict: bad arguments"
