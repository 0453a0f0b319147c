"""Compile one unit of csrc/ for the device as the Makefile compiles it and read what the code object says of its kernels.  No
GPU is needed: `hipcc -S --cuda-device-only` and the metadata at the end of the assembly, nothing else of it."""
import os
import re
import shutil
import subprocess

from conftest import REPO

CSRC = os.path.join(REPO, "rl_arm_under_sparse_reward_amd", "csrc")
FIGURES = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def kernel_metadata(tmp_path, unit, source=None):
    """The kernels of `unit` (a file of csrc/ that the Makefile lists in EXACT_SRCS and so compiles without contraction), built
    with the Makefile's own flags: kernel name -> {VGPRs, SGPRs, LDS bytes, private_segment_fixed_size, spilled VGPRs, SGPRs}
    under the names of FIGURES.  `source`: the text of a stand-in unit named `unit` (a header's kernels alone, where the unit that
    compiles them is too slow for a test), compiled with the same flags and csrc/ on the include path."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    line = lambda name: re.search(rf"^{name} :?\??= (.*)$", mk, flags=re.M).group(1)
    assert (source is not None or unit in line("EXACT_SRCS").split()) and "-ffp-contract=off" in line("EXACT")
    path = os.path.join(CSRC, unit)
    if source is not None:
        path = str(tmp_path / unit)
        with open(path, "w") as f:
            f.write(source)
    hipcc = line("HIPCC")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc is needed to build the library at all"
    flags = line("COMMON").replace("$(ARCH)", "gfx950").replace("$(INC)", f"-I{os.path.join(REPO, 'include')} -I{CSRC}").split()
    out = tmp_path / (unit + ".s")
    subprocess.check_call([hipcc, *flags, *line("EXACT").split(), "--cuda-device-only", "-S", path, "-o", str(out)])
    meta = {}
    for block in out.read_text().split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in FIGURES}
    return meta
