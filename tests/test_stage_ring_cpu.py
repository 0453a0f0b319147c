"""csrc/stage_ring.h -- the host bookkeeping of the pinned ring behind hp_agent_train_cycle -- is plain C++: its stand-alone check
(tests/host/stage_ring_main.cpp, a program with its own main and a stub for the event calls) is built for the CPU with the address
and undefined-behaviour sanitizers and run."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_ring_rotation_growth_release_under_sanitizers(tmp_path):
    cxx = next((c for c in ("g++", "clang++", "c++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "a host C++ compiler is needed (the ROCm toolchain that builds the library brings one)"
    exe = tmp_path / "stage_ring_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "rl_arm_under_sparse_reward_amd", "csrc"),
                           os.path.join(REPO, "tests", "host", "stage_ring_main.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "stage_ring ok" in p.stdout, p.stdout + p.stderr
