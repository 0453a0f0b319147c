"""Scripted demonstrations without a device: the host controller and generator (synthetic.scripted_action / scripted_demos)
against a file the reference's own generator wrote on the push-block stand-in
(tests/golden/ref_written_2_push_block_demo.npz, tools/gen_golden.py refpushdemo), every phase and the stop rule on both host
kinds against the schedule restated here, the round rule against a hand-rolled loop, the writer through both loaders, the ABI's
new entries, and the static figures of the two new kernels from a cross-compile."""
import ast
import ctypes as C
import json
import math
import os
import re
import types

import numpy as np
import pytest

from conftest import GOLDEN, REPO, bits
from kernel_metadata import kernel_metadata
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.synthetic import (DemoScript, PointMassGoalEnv, PushBlockGoalEnv, scripted_action,
                                                      scripted_demos, scripted_episode, write_demo_npz_from)

SHORT = dict(phase_end=(2, 4, 8, 10, 12))    # six phases inside T = 20
REFERENCE = "/root/reference"


def test_host_generator_reproduces_the_reference_written_file():
    """One PushBlockGoalEnv(seed=0), n_demos = 2, one episode per round: the reference's loop.  The fixture is what
    get_push_demo itself wrote on that environment, and the count beside it the episodes it attempted."""
    ref = np.load(os.path.join(GOLDEN, "ref_written_2_push_block_demo.npz"), allow_pickle=True)
    attempted_ref = json.load(open(os.path.join(GOLDEN, "ref_written_2_push_block_demo.json")))["attempted"]
    obs, ag, g, actions, info, attempted = scripted_demos([PushBlockGoalEnv(seed=0)], 2, 1)
    for name, ours in (("obs", obs), ("ag", ag), ("g", g), ("acs", actions)):
        assert ours.dtype == ref[name].dtype and ours.shape == ref[name].shape, name
        assert np.array_equal(bits(ours), bits(ref[name])), name
    ref_info = np.array([[np.float32(d["is_success"]) for d in row] for row in ref["info"]], dtype=np.float32)
    assert info.dtype == np.float32 and np.array_equal(info, ref_info) and np.all(info[:, -1] == 1.0)
    assert attempted == attempted_ref == 38


def restated_action(t, obs, g, s):
    """The schedule of get_demo_data_push.py:39-61 written out once more, phase by phase; returns (action, phase, stopped)"""
    grip, b = obs[0:3], obs[12:15]
    ends = s.phase_end
    phase = next((k for k, e in enumerate(ends) if t <= e), 5)
    if phase == 0:
        a = list(s.lift)
    elif phase in (1, 4):
        a = [(g[c] - b[c]) * s.behind + b[c] - grip[c] for c in range(3)] + [0.0]
    elif phase == 3:
        a = [s.waypoint[c] - grip[c] for c in range(3)] + [0.0]
    else:
        a = [g[c] - b[c] for c in range(3)] + [0.0]
    stopped = math.sqrt((b[0] - g[0]) * (b[0] - g[0]) + (b[1] - g[1]) * (b[1] - g[1]) + (b[2] - g[2]) * (b[2] - g[2])) < s.stop_radius
    if stopped:
        a = [0.0] * 4
    return np.array(a, dtype=np.float64), phase, stopped


@pytest.mark.parametrize("make", [lambda: PointMassGoalEnv(seed=3, max_timesteps=20), lambda: PushBlockGoalEnv(seed=3, max_timesteps=20)],
                         ids=["point_mass", "push_block"])
def test_a_short_script_visits_every_phase_and_the_stop_rule(make):
    seen, stops, largest = set(), 0, 0.0
    for radius in (0.05, 0.3):        # the wide radius stops the push block's controller too
        s = DemoScript(stop_radius=radius, lift=(0.0, -0.7, 0.7, 0.0), **SHORT)     # 0.7: stored as it is, applied as 0.5
        env, twin = make(), make()
        for _ in range(4):
            obs, ag, g, actions, ok = scripted_episode(env, s)
            o = twin.reset()
            for t in range(1, 21):
                want, phase, stopped = restated_action(t, o['observation'], o['desired_goal'], s)
                seen.add(phase)
                stops += stopped
                got = scripted_action(t, o['observation'], o['desired_goal'], s)
                assert got.dtype == np.float64 and np.array_equal(bits(got), bits(want)), (t, phase, stopped)
                assert np.array_equal(bits(actions[t - 1]), bits(want)) and np.array_equal(bits(obs[t - 1]), bits(o['observation']))
                o, _, _, info = twin.step(want)
                assert ok[t - 1] == info['is_success']
            largest = max(largest, np.abs(actions).max())
            assert np.array_equal(bits(obs[20]), bits(o['observation'])) and np.array_equal(bits(ag[20]), bits(o['achieved_goal']))
    assert seen == {0, 1, 2, 3, 4, 5} and stops > 0 and largest == 0.7
    with pytest.raises(ValueError, match="must be increasing"):
        DemoScript(phase_end=(2, 4, 4, 10, 12))


def hand_rolled(envs, n_demos, round_waves, max_episodes, script):
    """scripted_demos' rounds written as the nested loops of the definition"""
    kept, attempted, n_envs = [], 0, len(envs)
    while len(kept) < n_demos and attempted < max_episodes:
        left = min(n_envs * round_waves, max_episodes - attempted)
        for w in range(round_waves):
            for i in range(n_envs):
                if w * n_envs + i < left:
                    ep = scripted_episode(envs[i], script)
                    attempted += 1
                    if ep[4][-1] == 1.0:
                        kept.append(ep)
    return kept[:n_demos], attempted


def test_the_round_rule_is_deterministic_and_whole():
    s = DemoScript(**SHORT)
    make = lambda: [PointMassGoalEnv(seed=10 + i, max_timesteps=20) for i in range(3)]
    a, b = make(), make()
    *arrays, attempted = scripted_demos(a, 4, 2, script=s)
    kept, attempted_b = hand_rolled(b, 4, 2, 10000, s)
    assert attempted == attempted_b and attempted % 6 == 0 and len(kept) == 4
    for j, arr in enumerate(arrays):
        assert np.array_equal(bits(arr), bits(np.array([ep[j] for ep in kept]))), j
    for x, y in zip(a, b):           # the surplus of the last round is dropped, its resets are consumed
        sx, sy = x.rs.get_state(), y.rs.get_state()
        assert np.array_equal(sx[1], sy[1]) and sx[2:] == sy[2:]
    # the same call again on fresh twins: the same bits
    *again, attempted_c = scripted_demos(make(), 4, 2, script=s)
    assert attempted_c == attempted and all(np.array_equal(bits(p), bits(q)) for p, q in zip(arrays, again))


def test_max_episodes_reached_returns_fewer_and_says_how_many_ran():
    envs = [PushBlockGoalEnv(seed=0)]
    obs, ag, g, actions, info, attempted = scripted_demos(envs, 2, 8, max_episodes=30)      # attempts 5 and 38 succeed
    assert attempted == 30 and obs.shape[0] == info.shape[0] == 1
    assert obs.shape[1:] == (101, 27) and ag.shape[1:] == (101, 3) and g.shape[1:] == (100, 3) and actions.shape[1:] == (100, 4)
    obs, *_, attempted = scripted_demos([PushBlockGoalEnv(seed=0)], 2, 8, max_episodes=4)
    assert attempted == 4 and obs.shape == (0, 101, 27)


class _Recorder:
    def store_episode(self, batch):
        self.batch = batch


def test_a_written_file_loads_through_the_package_loader(tmp_path):
    from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
    obs, ag, g, actions, info, _ = scripted_demos([PushBlockGoalEnv(seed=0)], 2, 1)
    path = str(tmp_path / "bmirobot_2_push_demo.npz")
    write_demo_npz_from(path, obs, ag, g, actions, info)
    ref = np.load(os.path.join(GOLDEN, "ref_written_2_push_block_demo.npz"), allow_pickle=True)
    ours = np.load(path, allow_pickle=True)
    assert sorted(ours.files) == sorted(ref.files) == ["acs", "ag", "g", "info", "obs"]
    for k in ref.files:
        assert ours[k].dtype == ref[k].dtype and ours[k].shape == ref[k].shape, k
    assert ours["info"][1, 99] == ref["info"][1, 99] and type(ours["info"][0, 0]["is_success"]) is type(ref["info"][0, 0]["is_success"])
    me = types.SimpleNamespace(args=types.SimpleNamespace(demo_name=path, demo_source="file"), buffer=_Recorder())
    ddpg_agent._init_demo_buffer(me)
    for got, want in zip(me.buffer.batch, (obs, ag, g, actions)):
        assert np.array_equal(bits(got), bits(want))
    with pytest.raises(ValueError, match="demo_source must be"):
        ddpg_agent._init_demo_buffer(types.SimpleNamespace(args=types.SimpleNamespace(demo_name=path, demo_source="disk")))
    with pytest.raises(ValueError, match="needs a native vectorised device environment"):
        ddpg_agent._init_demo_buffer(types.SimpleNamespace(args=types.SimpleNamespace(demo_source="device"), vec_env=None))


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference's loader is read from its sources")
def test_a_written_file_loads_through_the_reference_loader(tmp_path):
    obs, ag, g, actions, info, _ = scripted_demos([PushBlockGoalEnv(seed=0)], 2, 1)
    path = str(tmp_path / "bmirobot_2_push_demo.npz")
    write_demo_npz_from(path, obs, ag, g, actions, info)
    tree = ast.parse(open(os.path.join(REFERENCE, "ddpg_agent.py")).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ddpg_agent")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_init_demo_buffer")
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "ddpg_agent.py:82-90", "exec"), ns)
    me = types.SimpleNamespace(args=types.SimpleNamespace(demo_name=path), buffer=_Recorder())
    ns["_init_demo_buffer"](me)
    for got, want in zip(me.buffer.batch, (obs, ag, g, actions)):
        assert np.array_equal(bits(got), bits(want))


def test_header_ctypes_table_and_exports_carry_the_new_entries():
    header = open(os.path.join(REPO, "include", "rlarm_hip.h")).read()
    for name in ("hp_demo_episodes", "hp_demo_compact"):
        assert name in _lib.PROTOTYPES and name not in _lib.DEBUG_SYMBOLS, name
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
    assert re.search(r"#define\s+HP_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    so = os.path.join(REPO, "rl_arm_under_sparse_reward_amd", "librlarm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as entry
        entry.build()
    lib = C.CDLL(so)
    assert hasattr(lib, "hp_demo_episodes") and hasattr(lib, "hp_demo_compact")
    # hp_demo_script, field for field: five phase ends + padding, four + three + one + one doubles
    body = re.search(r"typedef struct \{([^}]*)\}\s*hp_demo_script;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)(?:\[(\d+)\])?\s*[;,]", body)
    assert [(n, int(k or 1)) for n, k in fields] == [("phase_end", 5), ("reserved", 1), ("lift", 4), ("waypoint", 3), ("behind", 1),
                                                     ("stop_radius", 1)]
    assert [f[0] for f in _lib.DemoScriptDesc._fields_] == [n for n, _ in fields] and C.sizeof(_lib.DemoScriptDesc) == 24 + 9 * 8
    from rl_arm_under_sparse_reward_amd.device_env import default_round_waves, script_desc
    d, s = script_desc(), DemoScript()
    assert list(d.phase_end) == [10, 20, 40, 60, 80] and list(d.lift) == [0.0, -0.1, 0.1, 0.0] and d.reserved == 0
    assert list(d.waypoint) == [0.241, 0.3265, 0.294] and d.behind == -0.5 and d.stop_radius == 0.05 == s.stop_radius
    assert default_round_waves(1000, 64) == 32 and default_round_waves(1000, 1024) == 2 and default_round_waves(1, 4096) == 1
    from rl_arm_under_sparse_reward_amd.arguments import Args
    assert Args().demo_source == "file" and Args().demo_episodes == 1000 and Args().demo_max_episodes == 10000


def test_generate_demos_refuses_an_environment_it_cannot_run():
    from rl_arm_under_sparse_reward_amd.device_env import NativePushBlockVecEnv, PushBlockVecEnv, generate_demos
    with pytest.raises(ValueError, match="generate_demos: the environment is not native"):
        generate_demos(PushBlockVecEnv(2, device="cpu"), 1)
    with pytest.raises(ValueError, match="generate_demos: the environment is not reset on the device"):
        generate_demos(NativePushBlockVecEnv(2, device="cpu"), 1)


@pytest.mark.parametrize("unit, kernel, kind", [("demo_push_block.hip", "k_demo_episodes", "PushBlockEnvDev"),
                                                ("demo_point_mass.hip", "k_demo_episodes", "PointMassEnvDev"),
                                                ("demo_compact.hip", "k_demo_compact", "")])
def test_the_new_kernels_use_no_scratch(tmp_path, unit, kernel, kind):
    """private_segment_fixed_size 0 and no spilled vector register for both new kernels; k_demo_episodes keeps about the reset
    kernel's LDS (the ring) plus one row, so a CU's workgroups are bounded by its wave slots."""
    meta = kernel_metadata(tmp_path, unit)
    assert len(meta) == 1, sorted(meta)
    (name, m), = meta.items()
    print(name, m)
    assert kernel in name and kind in name
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    if kernel == "k_demo_episodes":
        ring, row = 4 * 624 * 4, (27 + 3 + 3 + 4) * 8
        assert ring + row <= m["group_segment_fixed_size"] <= ring + row + 128, m
    else:
        assert m["group_segment_fixed_size"] <= 64, m
