"""The kernels of the replay buffer's two units, csrc/buffer.hip (storage) and csrc/sampler.hip (the stand-alone sampler), without a
device: which kernels the units hold and the static figures of each, from a cross-compile with the Makefile's flags."""
import re

import pytest

from kernel_metadata import kernel_metadata

# name (and template arguments, as the mangled name spells them) of the fourteen kernels, and the unit each lives in
STORAGE = {"k_pack_rows": r"_Z11k_pack_rows", "k_goal_reward": r"_Z13k_goal_reward", "k_store_scatter": r"_Z15k_store_scatter"}
SAMPLER = {"k_gather_dict": r"_Z13k_gather_dict",
           "k_gather_fused<4>": r"_Z14k_gather_fusedILi4EE", "k_gather_fused<1>": r"_Z14k_gather_fusedILi1EE"}
for _k, _n in (("k_gather_fused2", 15), ("k_gather_packed", 15)):
    for _flight in (4, 1):
        for _fast in (0, 1):
            SAMPLER[f"{_k}<{_flight},{'true' if _fast else 'false'}>"] = rf"_Z{_n}{_k}ILi{_flight}ELb{_fast}EE"


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sampler_kernels")
    return {"buffer.hip": kernel_metadata(tmp, "buffer.hip"), "sampler.hip": kernel_metadata(tmp, "sampler.hip")}


def _named(meta, table):
    found = {label: [n for n in meta if re.match(pattern, n)] for label, pattern in table.items()}
    assert all(len(v) == 1 for v in found.values()), (found, sorted(meta))
    return {label: meta[v[0]] for label, v in found.items()}


def test_the_two_units_hold_exactly_the_fourteen_kernels(units):
    storage, sampler = _named(units["buffer.hip"], STORAGE), _named(units["sampler.hip"], SAMPLER)
    assert len(storage) == 3 and len(sampler) == 11
    assert len(units["buffer.hip"]) == 3, sorted(units["buffer.hip"])
    assert len(units["sampler.hip"]) == 11, sorted(units["sampler.hip"])


def test_no_kernel_uses_scratch_or_spills_a_vector_register(units):
    for unit, meta in units.items():
        for name, m in meta.items():
            print(unit, name, m)
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (unit, name, m)


def test_the_two_transition_kernels_keep_their_registers(units):
    """The plan-reading instantiations of k_gather_fused2 and k_gather_packed spill no SGPR to lanes, and every instantiation the
    launch rule can pick below the fast draw's deep form stays at or under 128 VGPRs: four waves per SIMD for the <4, false> forms
    that carry the large batches, and the <1, *> forms of a batch of 256 far below it."""
    sampler = _named(units["sampler.hip"], SAMPLER)
    for k in ("k_gather_fused2", "k_gather_packed"):
        for flight in (4, 1):
            m = sampler[f"{k}<{flight},false>"]
            assert m["sgpr_spill_count"] == 0, (k, flight, m)
        assert sampler[f"{k}<4,false>"]["vgpr_count"] <= 128, (k, sampler[f"{k}<4,false>"])
        for fast in ("false", "true"):
            assert sampler[f"{k}<1,{fast}>"]["vgpr_count"] <= 128, (k, fast, sampler[f"{k}<1,{fast}>"])
