"""The kernels of the rollout-side forward without a device: which unit holds them and the static figures of each, from a
cross-compile with the Makefile's flags.  csrc/agent_forward.hip is host code: every kernel it launches is compiled by
csrc/agent_engines.hip -- k_policy_slab8 (slab8.h) because moved it was not the same device code, the four pack kernels
(forward_kernels.h) because the code object's layout behind them is measured (profiles/policy_call_refactor.txt, sections 1 and 4).
That unit is too slow to compile here, so the pack kernels are compiled alone, out of their header."""
import re

import pytest

from kernel_metadata import kernel_metadata

# the four pack kernels of the layer-per-launch chain, as the mangled names spell them
FORWARD = {"k_pack_inputs": r"_Z13k_pack_inputs", "k_policy_inputs": r"_Z15k_policy_inputs",
           "k_pack_scaled_actions": r"_Z21k_pack_scaled_actions", "k_unpack_actions": r"_Z16k_unpack_actions"}
ALONE = '#define FORWARD_KERNELS_HERE\n#include "forward_kernels.h"\n'


@pytest.fixture(scope="module")
def pack(tmp_path_factory):
    return kernel_metadata(tmp_path_factory.mktemp("forward_kernels"), "forward_kernels_alone.hip", source=ALONE)


def test_agent_forward_compiles_no_kernel_and_the_header_holds_exactly_the_four(tmp_path, pack):
    assert kernel_metadata(tmp_path, "agent_forward.hip") == {}
    found = {label: [n for n in pack if re.match(pattern, n)] for label, pattern in FORWARD.items()}
    assert all(len(v) == 1 for v in found.values()), (found, sorted(pack))
    assert len(pack) == 4, sorted(pack)


def test_no_pack_kernel_uses_scratch_lds_or_spills_a_vector_register(pack):
    for name, m in pack.items():
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["group_segment_fixed_size"] == 0, (name, m)
