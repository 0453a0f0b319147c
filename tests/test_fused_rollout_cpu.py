"""Whole episodes in one launch, without a device: the decision between the fused and the per-step wave
(device_env.fused_rollout_reason), the native point mass as a plain environment on the CPU, its descriptor, the ABI table, and the
fused kernel's device assembly (no scratch, LDS within a CU's)."""
import os
import re

import numpy as np
import torch

from conftest import REPO, bits
from kernel_metadata import kernel_metadata
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.device_env import NativePointMassVecEnv, PointMassVecEnv, fused_rollout_reason


def test_the_decision_names_each_fallback_and_nothing_else():
    for explore, streams in ((True, True), (False, True), (False, False)):
        assert fused_rollout_reason(True, True, explore, streams) is None, (explore, streams)
    assert "single shared stream" in fused_rollout_reason(True, True, True, False)
    for explore, streams in ((True, True), (True, False), (False, True), (False, False)):
        assert "not native" in fused_rollout_reason(False, True, explore, streams)
        assert "not slab-shaped" in fused_rollout_reason(True, False, explore, streams)
    assert fused_rollout_reason(getattr(PointMassVecEnv(2, device="cpu"), "is_native_device_env", False), True, False, True)


def test_the_native_point_mass_is_its_parent_on_the_cpu():
    a, b = PointMassVecEnv(5, seed=3, device="cpu", max_timesteps=20), NativePointMassVecEnv(5, seed=3, device="cpu", max_timesteps=20)
    assert b.is_device_vec_env and b.is_native_device_env and not getattr(a, "is_native_device_env", False)
    assert b.env_params == a.env_params
    for k in (5, 3):                                         # a full and a partial wave
        oa, ob = a.reset(k if k < 5 else None), b.reset(k if k < 5 else None)
        rs = np.random.RandomState(k)
        for _ in range(20):
            for key in oa:
                assert np.array_equal(bits(oa[key].numpy()), bits(ob[key].numpy())), key
            act = torch.from_numpy(rs.uniform(-0.7, 0.7, (k, 4)).astype(np.float32))
            (oa, ra, _, ia), (ob, rb, _, ib) = a.step(act), b.step(act)
            assert torch.equal(ra, rb) and torch.equal(ia["is_success"], ib["is_success"])
        assert np.array_equal(bits(a.pos.numpy()), bits(b.pos.numpy())) and np.array_equal(bits(a.vel.numpy()), bits(b.vel.numpy()))


def test_native_desc_has_the_documented_fields():
    env = NativePointMassVecEnv(4, seed=1, device="cpu", step_scale=0.07, distance_threshold=0.03)
    env.reset(3)
    d = env.native_desc()
    assert sorted(d) == ["kind", "params", "state"] and d["kind"] == _lib.ENV_POINT_MASS == 1
    assert d["params"] == [0.07, 0.03]
    assert len(d["state"]) == 3 and d["state"][0] is env.pos and d["state"][1] is env.vel and d["state"][2] is env.goal
    for t in d["state"]:
        assert t.dtype == torch.float64 and tuple(t.shape) == (3, 3) and t.is_contiguous()
    desc = _lib.EnvDesc(kind=d["kind"])
    assert len(desc.params) == 8 and len(desc.state_dev) == 4 and desc.reserved == 0


def test_abi_table_and_header_carry_the_entry_point():
    assert "hp_rollout_episodes" in _lib.PROTOTYPES and "hp_rollout_episodes" not in _lib.DEBUG_SYMBOLS
    header = open(os.path.join(REPO, "include", "rlarm_hip.h")).read()
    assert re.search(r"#define\s+HP_ABI_VERSION\s+4\b", header)
    assert re.search(r"enum\s*\{\s*HP_ENV_POINT_MASS\s*=\s*1\s*\}", header) and "hp_env_desc;" in header


def test_the_fused_kernel_uses_no_scratch(tmp_path):
    """The device assembly of csrc/env_point_mass.hip (the unit that instantiates the point mass's kernels), compiled as the Makefile
    compiles it: k_rollout_episodes has
    private_segment_fixed_size 0 and no spilled vector register, and its LDS fits the 160 KiB of a CU."""
    meta = kernel_metadata(tmp_path, "env_point_mass.hip")
    fused = [k for k in meta if "k_rollout_episodes" in k]
    assert len(fused) == 1 and "PointMassEnvDev" in fused[0], sorted(meta)
    m = meta[fused[0]]
    print("k_rollout_episodes:", m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    assert m["group_segment_fixed_size"] <= 160 * 1024, m
