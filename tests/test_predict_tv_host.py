"""The pure-host part of the predict under the time-variable kernel (psoap_amd/csrc/predict_plan.hpp: predict_tv_check,
predict_tv_taus, predict_tv_flops, and the shape and staging arithmetic predict_tv_run takes from the plain call) built by a
host compiler alone into tests/host/predict_tv_host_check.cpp, with AddressSanitizer and UBSan, and run as a child process:
a clean run -- the program checks its own invariants -- and every line it prints reproduced by the restatement below."""
import os
import subprocess

import pytest

from test_plan_host import FLAGS, host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "predict_tv_host_check.cpp")
NB = 128
SUM3 = "mode 1 with three components is not provided (the transposed mean of predict_f_g_h_sum, covariance.py:294)"
NO_TIMES = "call psoap_chunk_set_times first"
STREAM = "the handle has an open stream (psoap_stream_close first)"
BASELINE = ("the handle has a baseline (psoap_chunk_set_baseline): the time-variable kernel under the marginalised continuum is not "
            "built yet")
TAU = "every tau must be a time scale: positive, +inf for a static component"
T_PRED = "t_pred must be finite"


def up(n):
    return (n + NB - 1) // NB * NB


def tiles(n):
    return (n + NB - 1) // NB


def flops(n, r, sigma, var):
    return n * n * n / 3.0 + n * n * r + (n * r * r if sigma else (2.0 * n * r if var else 0.0)) + 2.0 * n * r


def shape(mode, c, N, M):
    """predict_tv_check's mode rules and what predict_tv_run sizes and launches, restated: the text behind " : " """
    if not (0 <= mode <= 2 and 1 <= c <= 3 and M >= 1):
        return "bad arguments"
    if mode == 2 and c != 1:
        return "mode 2 (predict_f) needs c == 1"
    if mode == 1 and c == 3:
        return SUM3
    if mode == 1 and c != 2:
        return "mode 1 (the sum) needs c == 2"
    if mode == 0 and c < 2:
        return "mode 0 (the components) needs c == 2 or 3"
    Npad, Rq = up(N), (c * M if mode == 0 else M)
    P, Mt, St = Npad // NB, up(Rq) // NB, up(Rq) // NB
    blocks = c if mode == 0 else 1
    update = sum(p * (P - p + Mt) for p in range(1, P))
    strip = sum(P - p + Mt - 1 for p in range(P))
    n, r = float(Npad), float(up(Rq))
    return (f"ld {Npad + up(Rq)} Rq {Rq} Rq_pad {up(Rq)} staging {4 * up(Rq) + 4} cross {blocks}x({tiles(M)},{tiles(N)}) "
            f"prior {blocks}x({tiles(M)},{tiles(M)}) sym {P * (P + 1) // 2} update {update} strip {strip} sigma {St * (St + 1) // 2} "
            f"gemv ({(Rq + 127) // 128},{(Npad + 255) // 256}) flops {flops(n, r, True, False):.6e} {flops(n, r, False, True):.6e} "
            f"{flops(n, r, False, False):.6e}")


# (name, mode, c, N, M): the cases of tests/test_gpu_timevar_predict.py, the retrieve shape of profiles/predict_timevar.md, the
# refusals by mode
EXPECTED = [("N100-c2", 0, 2, 100, 50), ("N100-c2-sum", 1, 2, 100, 130), ("N300-c1", 2, 1, 300, 129), ("N129-c2", 0, 2, 129, 65),
            ("N300-c3", 0, 3, 300, 43), ("N300-c2", 0, 2, 300, 100), ("N520-c2", 0, 2, 520, 64), ("retrieve", 0, 3, 8192, 1024),
            ("retrieve-two-dates", 0, 3, 8192, 2048), ("one-point", 2, 1, 74, 1), ("sum-of-three", 1, 3, 129, 129), ("f-c2", 2, 2, 10, 10),
            ("sum-c1", 1, 1, 10, 10), ("components-c1", 0, 1, 10, 10), ("mode3", 3, 1, 10, 10), ("c4", 0, 4, 10, 10), ("M0", 0, 2, 10, 0)]
STATE = [("ok", "ok"), ("inf-tau", "ok"), ("no-arrays", "bad arguments"), ("no-tau", "bad arguments"), ("no-t_pred", "bad arguments"),
         ("no-times", NO_TIMES), ("open-stream", STREAM), ("baseline", BASELINE), ("tau-zero", TAU), ("tau-negative", TAU),
         ("tau-nan", TAU), ("t_pred-inf", T_PRED), ("t_pred-minus-inf", T_PRED), ("t_pred-nan", T_PRED)]


def test_the_cases_are_those_of_the_gpu_test():
    import timevar_predict_reference as tp
    have = {(mode, c, N, M) for _, mode, c, N, M in EXPECTED}
    for pc in tp.PCASES:
        mode, lwls = tp.pcase_args(pc)[:2]
        assert (mode, lwls.shape[0], lwls.shape[1], pc[2]) in have, pc


def test_restatement_by_hand():
    """N129-c2 with 65 points: two block rows, two tile columns appended -- row 0 solves 3 tiles, row 1 updates 3 and solves 2;
    one 128-tile of Sigma when R = 128 exactly"""
    assert shape(0, 2, 129, 65).startswith("ld 512 Rq 130 Rq_pad 256 staging 1028 cross 2x(1,2) prior 2x(1,1) sym 3 update 3 strip 5 "
                                           "sigma 3 gemv (2,1) ")
    assert " sigma 1 " in shape(0, 2, 520, 64) and " update 30 strip 15 " in shape(0, 2, 520, 64)
    assert shape(1, 2, 100, 130).startswith("ld 384 Rq 130 Rq_pad 256 staging 1028 cross 1x(2,1) prior 1x(2,2) sym 1 update 0 strip 2 ")


def test_the_messages_are_the_librarys():
    """what psoap_last_error gives for a refused call comes from predict_plan.hpp alone; the baseline's wording is that of
    psoap_chunk_lnlike_tv_grad"""
    plan = open(os.path.join(ROOT, "psoap_amd", "csrc", "predict_plan.hpp")).read().replace('"\n               "', "")
    for msg in (SUM3, NO_TIMES, STREAM, BASELINE, TAU, T_PRED):
        assert f'"{msg}"' in plan, msg
    hip = " ".join(open(os.path.join(ROOT, "psoap_amd", "csrc", "psoap_gp.hip")).read().replace('"\n             "', "").split())
    assert f'"psoap_chunk_lnlike_tv_grad: {BASELINE}"' in hip


def test_predict_tv_plan_runs_clean_under_sanitizers_and_matches_the_restatement(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    exe = str(tmp_path / "predict_tv_host_check")
    cc = subprocess.run([cxx, *os.environ.get("CXX", "").split()[1:], *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True,
                        cwd=str(tmp_path))
    assert cc.returncode == 0, cc.stderr
    if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        assert cc.stderr == "", cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    lines = run.stdout.splitlines()
    assert len(lines) == len(EXPECTED) + len(STATE)
    for ln, (name, mode, c, N, M) in zip(lines, EXPECTED):
        assert ln == f"{name} mode={mode} c={c} N={N} M={M} : {shape(mode, c, N, M)}", ln
    for ln, (name, why) in zip(lines[len(EXPECTED):], STATE):
        assert ln == f"{name} : {why}", ln
