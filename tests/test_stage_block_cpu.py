"""csrc/stage_block.h -- which doubles of a staged block a scatter thread of the cycle-opening launch owns, where each goes, whether
a batch fits the direct form, and the rows per LDS trip of the normalizer update -- is plain C++ without loads or stores: its
stand-alone check (tests/host/stage_block_main.cpp, a program with its own main) is built for the CPU with the address and
undefined-behaviour sanitizers and run over every shape of the multi-chunk and multi-trip GPU tests."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_block_ownership_locate_fit_and_chunk_sizes_under_sanitizers(tmp_path):
    cxx = next((c for c in ("g++", "clang++", "c++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "a host C++ compiler is needed (the ROCm toolchain that builds the library brings one)"
    exe = tmp_path / "stage_block_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "rl_arm_under_sparse_reward_amd", "csrc"),
                           os.path.join(REPO, "tests", "host", "stage_block_main.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "stage_block ok" in p.stdout, p.stdout + p.stderr
