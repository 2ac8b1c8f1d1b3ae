"""The device-sharing layer (psoap_amd/csrc/share.hpp: the per-device lock, the slot files, the driver's process count, the
staged-or-persistent policy) built by a host compiler alone into tests/host/share_host_check.cpp, with AddressSanitizer and
UBSan, and run as a child process once per mode: the layer reads several settings once per process, so every mode has a
process, an environment and a lock directory of its own.  The program checks what the layer does; this file checks that it
leaves clean and what the layer says on stderr.  No GPU, nothing under /sys: the bus ids are the program's, the driver's
tree is one it writes, and the count from the real one is switched off wherever share_procs would ask for it."""
import os
import subprocess

import pytest

from test_plan_host import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "share_host_check.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-pthread"]
FLAGS = COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
TSAN_FLAGS = COMMON + ["-fsanitize=thread"]

NO_DIR = "psoap: {dir} is not a directory of this user: several processes on one GPU are not serialised"
NO_LOCK = "psoap: cannot open the device lock {what}: several processes on this GPU are not serialised"
HINT = "psoap: 9 processes share this GPU: evaluations take the staged path (safe, slower)."
BEYOND = "psoap: {n} processes share this GPU and the persistent kernel was pinned there (PSOAP_SHARE_POLICY=dag or "
DETECT_ONLY = "psoap: PSOAP_SHARE_DETECT_ONLY=1: evaluations that reported a moved workgroup are handed out as they are"

# id -> (mode, what the lock directory is before the run, the mode's environment, the lines expected on stderr: each begins
# with its entry once `{dir}` is filled in, and there are no others)
RUNS = {
    "dir": ("dir", "missing", {}, []),
    "dir-symlink": ("dir-symlink", "symlink", {}, [NO_DIR, NO_LOCK.format(what="(no lock directory)")]),
    "dir-file": ("dir-file", "file", {}, [NO_DIR, NO_LOCK.format(what="(no lock directory)")]),
    "lock-symlink": ("lock-symlink", "dir", {}, [NO_LOCK.format(what="{dir}/gpu_0000_c1_00_0.lock")]),
    "lock": ("lock", "dir", {}, []),
    "timeout": ("timeout", "dir", {"PSOAP_DEVICE_LOCK_TIMEOUT_S": "0.3"}, []),
    "fork": ("fork", "dir", {"PSOAP_DEVICE_LOCK_TIMEOUT_S": "0.3"}, []),
    "slots": ("slots", "dir", {}, []),
    "slots-off": ("slots-off", "dir", {"PSOAP_DEVICE_SLOTS": "0"}, []),
    "kfd": ("kfd", "dir", {"PSOAP_KFD_COUNT": None}, []),
    "kfd-off": ("kfd-off", "dir", {"PSOAP_KFD_COUNT": "0"}, []),
    "policy": ("policy", "dir", {}, [HINT, BEYOND.format(n=16)]),
    "policy-quiet": ("policy", "dir", {"PSOAP_QUIET": "1"}, []),
    "policy-nolock": ("policy-nolock", "dir", {"PSOAP_DEVICE_LOCK": "0", "PSOAP_QUIET": "1"}, []),
    "policy-dag": ("policy-dag", "dir", {"PSOAP_SHARE_POLICY": "dag"}, [BEYOND.format(n=9)]),
    "policy-staged": ("policy-staged", "dir", {"PSOAP_SHARE_POLICY": "staged", "PSOAP_QUIET": "1"}, []),
    "knobs": ("knobs", "dir", {"PSOAP_SHARE_DETECT_ONLY": "1", "PSOAP_TEST_TAINT_EVERY": "3"}, [DETECT_ONLY]),
    "threads": ("threads", "dir", {}, []),
}


def compile_program(cxx, flags, exe, cwd):
    return subprocess.Popen([cxx, *os.environ.get("CXX", "").split()[1:], *flags, SOURCE, "-o", exe], stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True, cwd=cwd)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """(the ASan+UBSan program, the ThreadSanitizer program); both compiles run side by side and both must succeed"""
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, the clang++ beside hipcc, g++)")
    where = tmp_path_factory.mktemp("share_host")
    exe, exe_tsan = str(where / "share_host_check"), str(where / "share_host_check_tsan")
    cc, cc_tsan = compile_program(cxx, FLAGS, exe, str(where)), compile_program(cxx, TSAN_FLAGS, exe_tsan, str(where))
    err, err_tsan = cc.communicate()[1], cc_tsan.communicate()[1]
    assert cc.returncode == 0, err
    assert cc_tsan.returncode == 0, err_tsan
    if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        assert err == "" and err_tsan == "", err + err_tsan
    return exe, exe_tsan


def run_mode(exe, tmp_path, run_id):
    mode, before, extra, _ = RUNS[run_id]
    locks = tmp_path / "locks"
    if before == "dir":
        locks.mkdir(mode=0o700)
    elif before == "file":
        locks.write_text("")
    elif before == "symlink":
        (tmp_path / "real").mkdir(mode=0o700)
        locks.symlink_to(tmp_path / "real")
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    env = {k: v for k, v in os.environ.items() if not k.startswith("PSOAP_")}
    env.update(PSOAP_LOCK_DIR=str(locks), PSOAP_KFD_COUNT="0")
    for k, v in extra.items():
        if v is None:
            env.pop(k)
        else:
            env[k] = v
    return subprocess.run([exe, mode, str(scratch)], capture_output=True, text=True, timeout=60, cwd=str(tmp_path), env=env)


@pytest.mark.parametrize("run_id", list(RUNS))
def test_sharing_layer_on_the_host_under_sanitizers(programs, tmp_path, run_id):
    run = run_mode(programs[0], tmp_path, run_id)
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stdout == RUNS[run_id][0] + " ok\n"
    said, want = run.stderr.splitlines(), [w.format(dir=tmp_path / "locks") for w in RUNS[run_id][3]]
    assert len(said) == len(want) and all(s.startswith(w) for s, w in zip(said, want)), run.stderr


def test_threads_mode_under_thread_sanitizer(programs, tmp_path):
    run = run_mode(programs[1], tmp_path, "threads")
    # (the one excuse: the runtime refuses some kernels' address-space layouts and ends before main)
    if run.returncode != 0 and run.stdout == "" and "FATAL: ThreadSanitizer" in run.stderr:
        pytest.skip("ThreadSanitizer does not start here: " + run.stderr.strip()[-300:])
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stdout == "threads ok\n" and run.stderr == ""
