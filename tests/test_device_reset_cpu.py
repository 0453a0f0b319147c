"""Reset on the device and all waves in one launch, without a device: the ABI table and the header, the device assembly of the
kernel that runs the wave loop (no scratch, no spilled vector register, LDS within a CU's), how a training state carries the
environments' reset streams (train_state on hand-built arrays and manifests), and the Python switches."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, bits
from cpu_common import stream_arrays, synthetic_state
from kernel_metadata import kernel_metadata
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd import train_state as ts
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.device_env import NativePointMassVecEnv, PointMassVecEnv

NEW = ("hp_env_reset", "hp_rollout_waves")


def test_abi_table_and_header_carry_the_entry_points():
    header = open(os.path.join(REPO, "include", "rlarm_hip.h")).read()
    for name in NEW:
        assert name in _lib.PROTOTYPES and name not in _lib.DEBUG_SYMBOLS, name
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
    assert re.search(r"#define\s+HP_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    # hp_rollout_episodes' arguments with the reset streams behind the exploration streams, n_envs behind the descriptor and the
    # launch count at the end
    old, new = _lib.PROTOTYPES["hp_rollout_episodes"][1], _lib.PROTOTYPES["hp_rollout_waves"][1]
    assert new[:5] == old[:5] and new[6] is old[5] and new[8:14] == old[6:] and len(new) == len(old) + 3
    cap = int(re.search(r"#define\s+HP_ROLLOUT_MAX_LAUNCH_TIMESTEPS\s+(\d+)", header).group(1))
    assert cap == _lib.ROLLOUT_MAX_LAUNCH_TIMESTEPS and cap * 31e-6 < 0.5          # the slowest measured timestep: 31 us
    # the layout of hp_env_desc is the one the ABI version names
    desc = _lib.EnvDesc(kind=1)
    assert len(desc.params) == 8 and len(desc.state_dev) == 4 and desc.reserved == 0
    assert Args().device_reset is False


def test_the_wave_loop_kernel_uses_no_scratch(tmp_path):
    """The device assembly of csrc/env_point_mass.hip (the unit that instantiates the point mass's kernels), compiled as the Makefile
    compiles it: the kernel that runs the wave loop is the one instantiation of k_rollout_episodes, with private_segment_fixed_size
    0, no spilled vector register and LDS within the 160 KiB of a CU; the stand-alone reset kernel has no scratch either."""
    csrc = os.path.join(REPO, "rl_arm_under_sparse_reward_amd", "csrc")
    meta = kernel_metadata(tmp_path, "env_point_mass.hip")
    fused = [k for k in meta if "k_rollout_episodes" in k]
    assert len(fused) == 1 and "PointMassEnvDev" in fused[0], sorted(meta)
    # the wave loop lives in that kernel: the host entry of hp_rollout_waves (rollout.hip) launches it and no other, through the
    # one launch of the kind's table row (env_kind_entry, rollout_episodes.h)
    src = open(os.path.join(csrc, "rollout.hip")).read()
    units = src + open(os.path.join(csrc, "rollout_episodes.h")).read() + open(os.path.join(csrc, "env_point_mass.hip")).read()
    assert len(re.findall(r"hipLaunchKernelGGL\(k_rollout_episodes<", units)) == 1 and "A.waves" in src
    assert "kind->launch_episodes" in src
    m = meta[fused[0]]
    print("k_rollout_episodes:", m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    assert m["group_segment_fixed_size"] <= 160 * 1024, m
    reset = [k for k in meta if "k_env_reset" in k]
    assert len(reset) == 1 and meta[reset[0]]["private_segment_fixed_size"] == 0 and meta[reset[0]]["vgpr_spill_count"] == 0, meta


# ---------------------------------------------------------------------------------------------------------- training state
def state_with_reset_streams(n=3, explore=False):
    arrays, manifest = synthetic_state()
    extra, manifest["reset_streams"] = ts.stream_record(*stream_arrays(n), family="reset")
    arrays.update(extra)
    if explore:
        extra, manifest["explore_streams"] = ts.stream_record(*stream_arrays(n, pending=(0, 2)))
        arrays.update(extra)
    return arrays, manifest


@pytest.mark.parametrize("explore", [False, True])
def test_a_state_with_reset_streams_round_trips_and_verifies(tmp_path, explore):
    arrays, manifest = state_with_reset_streams(3, explore)
    assert ts.RESET_STREAM_ARRAYS == ("reset_stream_keys", "reset_stream_pos", "reset_stream_has_gauss", "reset_stream_gauss")
    assert manifest["reset_streams"]["n"] == 3 and sorted(manifest["reset_streams"]["arrays"]) == sorted(ts.RESET_STREAM_ARRAYS)
    assert arrays["reset_stream_has_gauss"].tolist() == [0, 1, 0] and arrays["reset_stream_gauss"][1] != 0.0
    path = ts.write_state(tmp_path / "s.npz", arrays, manifest)
    back, m = ts.read_state(path)
    assert m == manifest
    for name, a in zip(ts.RESET_STREAM_ARRAYS, stream_arrays(3)):
        assert back[name].dtype == np.dtype(ts.stream_shapes(3, "reset")[name][0]) and np.array_equal(back[name], a), name
    assert ts.verify(path)["reset_streams"]["n"] == 3
    assert ("explore_streams" in ts.verify(path)) == explore
    assert ts.main(["verify", path]) == 0


@pytest.mark.parametrize("name", ts.RESET_STREAM_ARRAYS)
def test_verify_names_a_missing_or_damaged_reset_stream_array(tmp_path, name):
    arrays, manifest = state_with_reset_streams(4, explore=True)
    gone = {k: v for k, v in arrays.items() if k != name}
    with pytest.raises(ts.StateError, match=f"array '{name}' is missing"):
        ts.verify(ts.write_state(tmp_path / "gone.npz", gone, manifest))
    bad = dict(arrays)
    bad[name] = arrays[name].copy()
    flat = bad[name].reshape(-1).view(np.uint8)
    flat[flat.size // 2] ^= 0x04
    with pytest.raises(ts.StateError, match=f"array '{name}' sums to"):
        ts.verify(ts.write_state(tmp_path / "bad.npz", bad, manifest))
    short = dict(arrays)
    short[name] = arrays[name][:3]
    with pytest.raises(ts.StateError, match=f"array '{name}' is .* 4 streams imply"):
        ts.verify(ts.write_state(tmp_path / "short.npz", short, manifest))


def test_verify_refuses_a_wrong_sum_in_the_manifest(tmp_path):
    arrays, manifest = state_with_reset_streams(2)
    manifest["reset_streams"]["arrays"]["reset_stream_pos"]["sum"][0] ^= 1
    with pytest.raises(ts.StateError, match="array 'reset_stream_pos' sums to .* the manifest says"):
        ts.verify(ts.write_state(tmp_path / "s.npz", arrays, manifest))


def test_verify_refuses_reset_stream_arrays_the_manifest_does_not_list(tmp_path):
    arrays, manifest = state_with_reset_streams(2, explore=True)
    del manifest["reset_streams"]
    with pytest.raises(ts.StateError, match="array 'reset_stream_keys' is present but the manifest has no 'reset_streams'"):
        ts.verify(ts.write_state(tmp_path / "s.npz", arrays, manifest))


@pytest.mark.parametrize("pos", [-1, 625])
def test_verify_refuses_a_reset_position_outside_the_key(tmp_path, pos):
    keys, p, has, val = stream_arrays(2)
    p[1] = pos
    arrays, manifest = synthetic_state()
    extra, manifest["reset_streams"] = ts.stream_record(keys, p, has, val, family="reset")
    arrays.update(extra)
    with pytest.raises(ts.StateError, match="'reset_stream_pos' holds a position outside"):
        ts.verify(ts.write_state(tmp_path / "s.npz", arrays, manifest))
    p[1] = 624                                            # numpy's lazy form: a fresh block is due
    extra, manifest["reset_streams"] = ts.stream_record(keys, p, has, val, family="reset")
    arrays.update(extra)
    ts.verify(ts.write_state(tmp_path / "ok.npz", arrays, manifest))


def test_a_state_without_reset_streams_is_written_as_before(tmp_path):
    arrays, manifest = synthetic_state()
    back, m = ts.read_state(ts.write_state(tmp_path / "s.npz", arrays, manifest))
    assert "reset_streams" not in m and not [k for k in back if k.startswith("reset_stream")]
    assert ts.STREAM_ARRAYS == tuple(ts.stream_shapes(0)) and all(n.startswith("explore_stream_") for n in ts.STREAM_ARRAYS)


# ------------------------------------------------------------------------------------------------------------- environment
def test_enable_device_reset_needs_a_gpu_environment():
    env = NativePointMassVecEnv(3, seed=2, device="cpu")
    with pytest.raises(ValueError, match="enable_device_reset: the environment lives on device 'cpu'"):
        env.enable_device_reset()
    assert env.reset_streams is None


def test_native_desc_without_device_reset_is_unchanged():
    """Same keys, the environment's own tensors, shaped for the rows stepped now; and the environment still is its parent."""
    env, twin = NativePointMassVecEnv(4, seed=1, device="cpu", step_scale=0.07, distance_threshold=0.03), PointMassVecEnv(4, seed=1, device="cpu")
    assert env.reset_streams is None
    oa, ob = env.reset(3), twin.reset(3)
    for key in oa:
        assert np.array_equal(bits(oa[key].numpy()), bits(ob[key].numpy())), key
    d = env.native_desc()
    assert sorted(d) == ["kind", "params", "state"] and d["kind"] == _lib.ENV_POINT_MASS == 1 and d["params"] == [0.07, 0.03]
    assert len(d["state"]) == 3 and d["state"][0] is env.pos and d["state"][1] is env.vel and d["state"][2] is env.goal
    for t in d["state"]:
        assert t.dtype == torch.float64 and tuple(t.shape) == (3, 3) and t.is_contiguous()
    desc = env.env_desc()
    assert desc.kind == 1 and list(desc.params)[:2] == [0.07, 0.03] and [desc.state_dev[i] for i in range(3)] == [t.data_ptr() for t in d["state"]]
    assert desc.state_dev[3] is None
