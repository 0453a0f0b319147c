"""The push-block environment without a device: the host environment (synthetic.PushBlockGoalEnv) against its tensor twin
(device_env.PushBlockVecEnv on the CPU) bit for bit over a scripted sequence that takes every branch of `step`, the rejection loop
of `reset` counted through the stream position, the pinned constants of header and ABI table, and the device assembly of the
translation unit that instantiates the kernels for the kind (csrc/env_push_block.hip)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, bits
from kernel_metadata import kernel_metadata
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.device_env import NativePushBlockVecEnv, PushBlockVecEnv, fused_rollout_reason
from rl_arm_under_sparse_reward_amd.synthetic import (PUSH_RESET_BOUNDS, PUSH_START_Z, PUSH_X_HI, PUSH_X_LO, PUSH_Y_HI, PUSH_Y_LO,
                                                      PUSH_Z_HI, PushBlockGoalEnv)

# attempts of eight consecutive resets from RandomState(seed), measured with the host rule: first-try and multi-try resets
RESET_ATTEMPTS = {21: [2, 1, 1, 1, 2, 2, 1, 4], 22: [3, 1, 1, 1, 3, 3, 4, 1], 23: [1, 1, 1, 1, 1, 1, 1, 2],
                  24: [2, 2, 4, 3, 2, 1, 1, 1], 25: [1, 3, 2, 1, 1, 1, 3, 4]}
# parameters with exact binary fractions, so that the tie and dx == 0 are exact: a = +-0.25 moves the gripper by 1/32
EXACT = dict(step_scale=0.125, half_width=0.0625, z_touch=0.25, table_z=0.2)
HOST_STATE = ("grip", "blk", "goal", "gvel", "bvel")


def position_after(words):
    """numpy's `pos` after `words` 32-bit words out of a fresh RandomState (pos = 624: a twist is due before the first word)"""
    return 624 if words == 0 else (words - 1) % 624 + 1


def assert_twins_equal(hosts, vec, where):
    k = vec.active
    assert k == len(hosts)
    host = {name: np.stack([getattr(h, name) for h in hosts]) for name in HOST_STATE}
    got = {"grip": vec.grip[:k], "blk": vec.blk[:k], "goal": vec.goal[:k], "gvel": vec.vel[:k, 0:3], "bvel": vec.vel[:k, 3:6]}
    for name in HOST_STATE:
        assert np.array_equal(bits(host[name]), bits(got[name].numpy())), (where, name)
    for i, h in enumerate(hosts):
        a, b = h.rs.get_state(), vec.rs[i].get_state()
        assert np.array_equal(a[1], b[1]) and a[2:] == b[2:], (where, "stream", i)


def assert_outputs_equal(host_out, vec_out, where):
    """step's 4-tuples of the host environments against the twin's"""
    ov, rv, dv, iv = vec_out
    for i, (oh, rh, dh, ih) in enumerate(host_out):
        for key in oh:
            assert np.array_equal(bits(np.asarray(oh[key])), bits(ov[key][i].numpy())), (where, i, key)
        assert np.float32(rh) == rv[i].item() and dh is dv is False and np.float32(ih["is_success"]) == iv["is_success"][i].item(), (where, i)


def branches_of(env, action):
    """The branches of `step` the host environment `env` is about to take with `action`, recomputed from its state"""
    r, taken = env.half_width, set()
    a = np.clip(np.asarray(action, dtype=np.float64), -0.5, 0.5)
    free = env.grip + env.step_scale * a[:3]
    new = np.clip(free, [PUSH_X_LO, PUSH_Y_LO, env.table_z], [PUSH_X_HI, PUSH_Y_HI, PUSH_Z_HI])
    if np.any(new != free):
        taken.add("gripper clamped")
    dx, dy = env.blk[0] - new[0], env.blk[1] - new[1]
    if not new[2] < env.z_touch:
        return taken | {"too high"}
    if not (abs(dx) < r and abs(dy) < r):
        return taken | {"too far"}
    px, py = r - abs(dx), r - abs(dy)
    if px == py:
        taken.add("tie")
    if px <= py:
        taken.add("+x" if dx >= 0 else "-x")
        if dx == 0:
            taken.add("dx == 0")
        moved = new[0] + (r if dx >= 0 else -r)
        if not PUSH_X_LO <= moved <= PUSH_X_HI:
            taken.add("block clamped")
    else:
        taken.add("+y" if dy >= 0 else "-y")
        moved = new[1] + (r if dy >= 0 else -r)
        if not PUSH_Y_LO <= moved <= PUSH_Y_HI:
            taken.add("block clamped")
    return taken


# (gripper, block x y, actions): the block and the gripper are placed, then the actions run.  The fourth component is ignored and
# 0.7 is clamped to 0.5 before it is scaled.
SCRIPT = [
    ("too high", (0.25, 0.25, 0.3), (0.25, 0.25), [(0, 0, 0, 0.3)]),
    ("too far", (0.1, 0.1, 0.2), (0.4, 0.4), [(0.25, 0, 0, 0)]),
    ("+x", (0.15, 0.3, 0.2), (0.22, 0.3), [(0.25, 0, 0, 0), (0.25, 0, 0, -0.4), (0.1, 0.05, 0, 0)]),
    ("-x", (0.29, 0.3, 0.2), (0.22, 0.3), [(-0.25, 0, 0, 0), (-0.25, 0.02, 0, 0)]),
    ("+y", (0.3, 0.25, 0.2), (0.3, 0.32), [(0, 0.25, 0, 0), (0.01, 0.25, 0, 0)]),
    ("-y", (0.3, 0.39, 0.2), (0.3, 0.32), [(0, -0.25, 0, 0), (0, -0.25, 0.7, 0)]),
    ("tie", (0.25, 0.25, 0.2), (0.28125, 0.28125), [(0, 0, 0, 0)]),
    ("dx == 0", (0.25, 0.25, 0.2), (0.25, 0.25), [(0, 0, 0, 0)]),
    ("block clamped", (0.42, 0.3, 0.2), (0.49, 0.3), [(0.25, 0, 0, 0), (0.25, 0, 0, 0)]),
    ("block clamped", (0.3, 0.62, 0.2), (0.3, 0.69), [(0, 0.25, 0, 0), (0, 0.7, 0, 0)]),
    ("gripper clamped", (0.49, 0.3, 0.21), (0.2, 0.3), [(0.7, 0, -0.5, 0), (0, -0.7, 0.5, 0)]),
]


def test_twins_agree_on_a_script_that_takes_every_branch():
    n = 2
    hosts = [PushBlockGoalEnv(seed=5 + i, max_timesteps=10, **EXACT) for i in range(n)]
    vec = PushBlockVecEnv(n, seed=5, device="cpu", max_timesteps=10, **EXACT)
    first, ov = [h.reset() for h in hosts], vec.reset()
    for i, oh in enumerate(first):
        for key in oh:
            assert np.array_equal(bits(oh[key]), bits(ov[key][i].numpy())), key
    assert_twins_equal(hosts, vec, "reset")
    taken, moved = set(), set()
    for name, grip, blk, actions in SCRIPT:
        for i, h in enumerate(hosts):                      # environment 1: the same scene and actions, its block a millimetre off
            shift = 0.0 if i == 0 else 0.001
            h.grip = np.array(grip)
            h.blk = np.array([blk[0] + shift, blk[1], h.table_z])
            vec.grip[i] = torch.from_numpy(h.grip)
            vec.blk[i] = torch.from_numpy(h.blk)
        for step, action in enumerate(actions):
            act = np.array([action, action], dtype=np.float32)
            now = branches_of(hosts[0], act[0])
            taken |= now
            assert name in now or step > 0, (name, now)
            out = [h.step(act[i]) for i, h in enumerate(hosts)]
            assert_outputs_equal(out, vec.step(torch.from_numpy(act)), (name, step))
            assert_twins_equal(hosts, vec, (name, step))
            bvel = hosts[0].bvel
            moved |= {axis for axis, v in zip("xy", bvel[:2]) if v != 0} | ({"still"} if not bvel.any() else set())
            assert bvel[2] == 0 and hosts[0].blk[2] == hosts[0].table_z
            if not now & {"+x", "-x", "+y", "-y"}:
                assert not bvel.any(), (name, step)
    assert taken == {"too high", "too far", "+x", "-x", "+y", "-y", "tie", "dx == 0", "block clamped", "gripper clamped"}, taken
    assert moved == {"x", "y", "still"}
    # the observation's layout (bmirobot_env_push_F.py:208-222) on the last state
    o, h = hosts[0]._observation(), hosts[0]
    want = np.zeros(27)
    want[0:3], want[6:9], want[12:15], want[18:21], want[21:24] = h.grip, h.gvel, h.blk, h.blk - h.grip, h.bvel
    assert np.array_equal(bits(o["observation"]), bits(want))
    assert np.array_equal(o["achieved_goal"], h.blk) and np.array_equal(o["desired_goal"], h.goal)


@pytest.mark.parametrize("k", [3, 2])
def test_twins_agree_under_random_actions_with_frequent_contact(k):
    """Three environments, full and partial waves, parameters under which random actions touch the block every few steps"""
    kw = dict(half_width=0.15, z_touch=0.6, step_scale=0.3, max_timesteps=20)
    hosts = [PushBlockGoalEnv(seed=40 + i, **kw) for i in range(3)][:k]
    vec = PushBlockVecEnv(3, seed=40, device="cpu", **kw)
    assert vec.env_params == hosts[0].env_params == {'obs': 27, 'goal': 3, 'action': 4, 'action_max': 0.5, 'max_timesteps': 20}
    rs = np.random.RandomState(k)
    contact = 0
    for episode in range(3):
        for h in hosts:
            h.reset()
        vec.reset(k if k < 3 else None)
        assert_twins_equal(hosts, vec, ("reset", episode))
        assert vec.reset_attempts[:k] == [h.reset_attempts for h in hosts]
        for t in range(20):
            act = rs.uniform(-0.7, 0.7, (k, 4)).astype(np.float32)
            out = [h.step(act[i]) for i, h in enumerate(hosts)]
            assert_outputs_equal(out, vec.step(torch.from_numpy(act)), (episode, t))
            assert_twins_equal(hosts, vec, (episode, t))
            contact += sum(bool(h.bvel.any()) for h in hosts)
    assert contact >= 5, contact
    # her_sampler probes the reward function with numpy arrays
    ag, g = np.stack([h.blk for h in hosts]), np.stack([h.goal for h in hosts])
    assert np.array_equal(vec.compute_reward(ag, g, None), hosts[0].compute_reward(ag, g, None))


@pytest.mark.parametrize("seed", sorted(RESET_ATTEMPTS))
def test_reset_attempts_follow_the_stream(seed):
    """Eight words an attempt: the stream position after every reset says how many attempts it took, on both twins"""
    host, vec = PushBlockGoalEnv(seed=seed), PushBlockVecEnv(1, seed=seed, device="cpu")
    attempts = 0
    for i, want in enumerate(RESET_ATTEMPTS[seed]):
        host.reset(); vec.reset()
        attempts += want
        assert host.reset_attempts == vec.reset_attempts[0] == want, (i, host.reset_attempts)
        assert host.rs.get_state()[2] == vec.rs[0].get_state()[2] == position_after(8 * attempts), i
        d = host.blk[:2] - host.goal[:2]
        assert np.sqrt(d[0] * d[0] + d[1] * d[1]) >= host.min_separation
        assert np.array_equal(bits(host.blk), bits(vec.blk[0].numpy())) and np.array_equal(bits(host.goal), bits(vec.goal[0].numpy()))
        assert host.grip.tolist() == [0.25, 0.1, PUSH_START_Z] and host.blk[2] == host.goal[2] == 0.2 and not host.gvel.any()
    assert {1} < set(RESET_ATTEMPTS[seed])                      # first-try and multi-try resets


def test_an_exhausted_reset_keeps_the_last_attempt():
    """min_separation = 10 accepts nothing: 100 attempts, 800 words, from RandomState(21) across a block regeneration to 176"""
    host, vec = PushBlockGoalEnv(seed=21, min_separation=10.0), PushBlockVecEnv(1, seed=21, device="cpu", min_separation=10.0)
    host.reset(); vec.reset()
    assert host.reset_attempts == vec.reset_attempts[0] == 100
    assert host.rs.get_state()[2] == vec.rs[0].get_state()[2] == position_after(800) == 176
    rs = np.random.RandomState(21)
    for _ in range(100):
        last = [rs.uniform(low, high) for low, high in PUSH_RESET_BOUNDS]
    assert np.array_equal(rs.get_state()[1], host.rs.get_state()[1])
    assert host.blk.tolist() == vec.blk[0].tolist() == [last[0], last[1], 0.2]
    assert host.goal.tolist() == vec.goal[0].tolist() == [last[2], last[3], 0.2]


def test_reset_ranges_are_float64_differences():
    """numpy computes low + (high - low) * next_double: 0.35 - 0.15 is not the literal 0.2, and the draw shows it"""
    assert 0.35 - 0.15 != 0.2
    rs, raw = np.random.RandomState(3), np.random.RandomState(3)
    for low, high in PUSH_RESET_BOUNDS * 50:
        assert rs.uniform(low, high) == low + (high - low) * raw.random_sample()
    header = open(os.path.join(REPO, "rl_arm_under_sparse_reward_amd", "csrc", "env_device.h")).read()
    assert "range = hi[k] - lo[k];" in header
    assert re.search(r"lo\[4\] = \{0\.15, 0\.2, 0\.0, 0\.2\}, hi\[4\] = \{0\.35, 0\.5, 0\.35, 0\.5\}", header)


def test_header_and_abi_table_carry_the_kind():
    header = open(os.path.join(REPO, "include", "rlarm_hip.h")).read()
    assert re.search(r"enum\s*\{\s*HP_ENV_PUSH_BLOCK\s*=\s*2\s*\}", header) and _lib.ENV_PUSH_BLOCK == 2
    assert re.search(r"enum\s*\{\s*HP_ENV_POINT_MASS\s*=\s*1\s*\}", header) and _lib.ENV_POINT_MASS == 1
    assert re.search(r"#define\s+HP_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    env = NativePushBlockVecEnv(4, seed=1, device="cpu", step_scale=0.07, distance_threshold=0.03, grip_start=(0.2, 0.15))
    assert env.is_device_vec_env and env.is_native_device_env and env.reset_streams is None
    assert fused_rollout_reason(env.is_native_device_env, True, True, True) is None
    env.reset(3)
    d = env.native_desc()
    assert sorted(d) == ["kind", "params", "state"] and d["kind"] == 2
    assert d["params"] == [0.07, 0.03, 0.04, 0.25, 0.15, 0.2, 0.2, 0.15] and len(d["params"]) == len(_lib.EnvDesc().params) == 8
    assert env.state_names == ("grip", "blk", "goal", "vel") and len(d["state"]) == len(_lib.EnvDesc().state_dev) == 4
    for t, name, width in zip(d["state"], env.state_names, (3, 3, 3, 6)):
        assert t is getattr(env, name) and t.dtype == torch.float64 and tuple(t.shape) == (3, width) and t.is_contiguous()
    assert env.pos.device == env.grip.device
    desc = env.env_desc()
    assert desc.kind == 2 and desc.reserved == 0 and list(desc.params) == d["params"]
    assert [desc.state_dev[i] for i in range(4)] == [t.data_ptr() for t in d["state"]]
    with pytest.raises(ValueError, match="enable_device_reset: the environment lives on device 'cpu'"):
        env.enable_device_reset()
    # the struct's workspace is the host's
    struct = open(os.path.join(REPO, "rl_arm_under_sparse_reward_amd", "csrc", "env_device.h")).read()
    assert f"X_LO = {PUSH_X_LO}, X_HI = {PUSH_X_HI}, Y_LO = {PUSH_Y_LO}, Y_HI = {PUSH_Y_HI}, Z_HI = {PUSH_Z_HI}, START_Z = {PUSH_START_Z}" in struct


def test_the_native_push_block_is_its_parent_on_the_cpu():
    a, b = PushBlockVecEnv(3, seed=3, device="cpu"), NativePushBlockVecEnv(3, seed=3, device="cpu")
    rs = np.random.RandomState(0)
    for k in (None, 2):
        oa, ob = a.reset(k), b.reset(k)
        for _ in range(5):
            for key in oa:
                assert np.array_equal(bits(oa[key].numpy()), bits(ob[key].numpy())), key
            act = torch.from_numpy(rs.uniform(-0.7, 0.7, (a.active, 4)).astype(np.float32))
            (oa, ra, _, ia), (ob, rb, _, ib) = a.step(act), b.step(act)
            assert torch.equal(ra, rb) and torch.equal(ia["is_success"], ib["is_success"])


def test_the_push_block_kernels_use_no_scratch(tmp_path):
    """The device assembly of csrc/env_push_block.hip, compiled as the Makefile compiles it: the one push-block instantiation of
    each kernel, private_segment_fixed_size 0, no spilled vector register, LDS within the 160 KiB of a CU."""
    csrc = os.path.join(REPO, "rl_arm_under_sparse_reward_amd", "csrc")
    meta = kernel_metadata(tmp_path, "env_push_block.hip")
    fused, reset = [k for k in meta if "k_rollout_episodes" in k], [k for k in meta if "k_env_reset" in k]
    assert len(meta) == 2 and len(fused) == 1 and len(reset) == 1 and all("PushBlockEnvDev" in k for k in meta), sorted(meta)
    for name in (fused[0], reset[0]):
        m = meta[name]
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 160 * 1024, (name, m)
    # the split by the launch cap stays in one place: this unit launches what it is told to, through the one launch of its table
    # row (env_kind_entry, rollout_episodes.h)
    src = open(os.path.join(csrc, "env_push_block.hip")).read() + open(os.path.join(csrc, "rollout_episodes.h")).read()
    assert "launch_cap" not in src and len(re.findall(r"hipLaunchKernelGGL\(k_rollout_episodes<", src)) == 1
