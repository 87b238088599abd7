"""The whole-batch NodeAffinity plan of the in-library node-sharded cycle
(csrc/ms_nam_layout.h nam_plan_whole), swept on the CPU by a stand-alone
program under ASan/UBSan (tests/cpp/test_nam_class_plan.cpp): the launch
precondition, the carve within the allocation, the per-class shard inputs
behind it, and a class-record count that no rank's row count changes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mini-kube-scheduler_amd")


def test_nam_class_plan_asan(tmp_path):
    exe = str(tmp_path / "test_nam_class_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_nam_class_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-I", os.path.join(PKG, "csrc"), src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[-1] == "0 failed", out.stdout
    assert lines[0] == "grid points checked: 392", out.stdout  # 8 row counts x 7 set counts x 7 pod counts
