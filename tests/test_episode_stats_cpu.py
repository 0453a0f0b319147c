"""Episode metrics without a device: the host twin (synthetic.episode_stats / episode_stats_summary) on a case written out by
hand, its step flags and rewards against the reference's own outputs on goal pairs within a few ulp of the threshold
(tests/golden/reward_adversarial.npz, reward_dense_success.npz) and against the `info` of scripted demonstrations, the summary
loop against plain Python accumulation, the ABI's new entries, and the static figures of the two kernels from a cross-compile."""
import ctypes as C
import os
import re

import numpy as np

from conftest import GOLDEN, REPO, bits, load_golden
from cpu_common import pairs_as_episodes
from kernel_metadata import kernel_metadata
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.synthetic import (EPISODE_STATS, EPISODE_SUMMARY, DemoScript, PointMassGoalEnv, episode_stats,
                                                      episode_stats_summary, scripted_demos)


def test_every_column_of_a_hand_written_case():
    """T = 5, three goal components, threshold 0.05, the goal at a fixed point and the achieved goal at a known distance from
    it along one axis (sqrt(fl(x x)) = |x| in float64): one episode that succeeds at t = 2 alone, one that never does, one that
    succeeds at every step."""
    dist = np.array([[0.3, 0.2, 0.03, 0.2, 0.4],
                     [0.3, 0.25, 0.2, 0.15, 0.1],
                     [0.04, 0.03, 0.02, 0.01, 0.0]])
    g = np.zeros((3, 5, 3))
    ag = np.zeros((3, 6, 3))
    ag[:, 0, :] = 9.0                        # the reset's achieved goal: no step reads it
    for axis, e in enumerate(range(3)):
        ag[e, 1:, axis] = dist[e]
    stats, flags = episode_stats(ag, g, 0.05)
    assert stats.dtype == np.float64 and stats.shape == (3, 6) and flags.dtype == np.float32 and flags.shape == (3, 5)
    assert EPISODE_STATS == ("ret", "final_distance", "min_distance", "first_success_step", "success_steps", "final_success")
    want = np.array([[-4.0, 0.4, 0.03, 2.0, 1.0, 0.0],
                     [-5.0, 0.1, 0.1, 5.0, 0.0, 0.0],
                     [0.0, 0.0, 0.0, 0.0, 5.0, 1.0]])
    assert np.array_equal(bits(stats), bits(want)), stats          # +0.0 return where every step succeeds: numpy's own sum
    assert np.array_equal(flags, np.array([[0, 0, 1, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], dtype=np.float32))
    # the distance is numpy's norm for fewer than 8 components
    rs = np.random.RandomState(0)
    for gd in (1, 2, 3, 7):
        a, b = rs.uniform(0, 0.5, (4, 9, gd)), rs.uniform(0, 0.5, (4, 8, gd))
        d = np.linalg.norm(a[:, 1:] - b, axis=-1)
        s, f = episode_stats(a, b, 0.2)
        assert np.array_equal(bits(s[:, 1]), bits(d[:, -1])) and np.array_equal(bits(s[:, 2]), bits(d.min(axis=1)))
        assert np.array_equal(f, (d < 0.2).astype(np.float32))


def test_step_flags_and_rewards_are_the_references_on_pairs_next_to_the_threshold():
    dense = load_golden("reward_dense_success.npz")
    for thr in (0.05, 0.1):
        for T in (1, 64):
            ag, g = pairs_as_episodes(dense["ag"], dense["g"], T)
            stats, flags = episode_stats(ag, g, thr)
            want = dense[f"thr{thr}_success"]
            assert np.array_equal(flags.reshape(-1), want) and 0 < want.sum() < want.size
            reward = (dense[f"thr{thr}_sparse_bits"] == 0xBF800000).reshape(-1, T)      # -1.0f; the other value is -0.0f
            assert np.array_equal(stats[:, 0], -reward.sum(axis=1).astype(np.float64))
            assert np.array_equal(stats[:, 4], want.reshape(-1, T).sum(axis=1)) and np.array_equal(stats[:, 5], want.reshape(-1, T)[:, -1])
    adv = load_golden("reward_adversarial.npz")          # rewards at 0.05 on squared distances within 8 ulp of the boundary
    missed = adv["r_bits"] == 0xBF800000
    assert set(np.unique(adv["r_bits"])) == {0x80000000, 0xBF800000}
    for T in (1, 64):
        ag, g = pairs_as_episodes(adv["ag"], adv["g"], T)
        stats, _ = episode_stats(ag, g, 0.05)
        assert np.array_equal(stats[:, 0], -missed.reshape(-1, T).sum(axis=1).astype(np.float64))


def test_step_flags_are_the_info_of_scripted_demonstrations():
    """Two definitions of the step flag -- the environment's `is_success` while it steps, and the twin's on the recorded goals --
    on a generated run and on the file the reference's own generator wrote."""
    s = DemoScript(phase_end=(2, 4, 8, 10, 12))
    envs = [PointMassGoalEnv(seed=10 + i, max_timesteps=20) for i in range(3)]
    _, ag, g, _, info, _ = scripted_demos(envs, 4, 2, script=s)
    stats, flags = episode_stats(ag, g, envs[0].distance_threshold)
    assert info.shape == (4, 20) and np.array_equal(flags, info) and np.all(stats[:, 5] == 1.0) and 0 < info.sum() < info.size
    assert np.array_equal(stats[:, 3], info.argmax(axis=1))
    ref = np.load(os.path.join(GOLDEN, "ref_written_2_push_block_demo.npz"), allow_pickle=True)
    ref_info = np.array([[np.float32(d["is_success"]) for d in row] for row in ref["info"]], dtype=np.float32)
    stats, flags = episode_stats(ref["ag"], ref["g"], 0.05)
    assert np.array_equal(flags, ref_info) and np.array_equal(stats[:, 4], ref_info.sum(axis=1))


def test_the_summary_is_a_left_to_right_loop():
    rs = np.random.RandomState(3)
    stats = rs.uniform(-100, 100, (37, 6))
    stats[:, 4] = rs.randint(0, 3, 37)
    stats[:, 5] = rs.randint(0, 2, 37)
    total = [0.0] * 6
    for row in stats.tolist():
        for k, v in enumerate((row[0], row[1], row[2], row[3], row[5], 1.0 if row[4] > 0 else 0.0)):
            total[k] = total[k] + v
    want = np.array([t / 37.0 for t in total])
    got = episode_stats_summary(stats)
    assert got.dtype == np.float64 and np.array_equal(bits(got), bits(want))
    assert EPISODE_SUMMARY == ("ret", "final_distance", "min_distance", "first_success_step", "success_rate", "any_success_rate")
    one = episode_stats_summary(stats[:1])
    assert np.array_equal(one, [stats[0, 0], stats[0, 1], stats[0, 2], stats[0, 3], stats[0, 5], float(stats[0, 4] > 0)])


def test_header_ctypes_table_and_exports_carry_the_new_entries():
    header = open(os.path.join(REPO, "include", "rlarm_hip.h")).read()
    names = ("hp_episode_stats", "hp_episode_stats_block", "hp_episode_stats_summary")
    for name in names:
        assert name in _lib.PROTOTYPES and name not in _lib.DEBUG_SYMBOLS, name
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
    assert re.search(r"#define\s+HP_EPISODE_STATS\s+6\b", header) and _lib.EPISODE_STATS == 6 == len(EPISODE_STATS)
    assert re.search(r"#define\s+HP_EPISODE_SUMMARY\s+6\b", header) and _lib.EPISODE_SUMMARY == 6 == len(EPISODE_SUMMARY)
    assert re.search(r"#define\s+HP_EPISODE_MAX_GOAL_DIM\s+256\b", header) and _lib.EPISODE_MAX_GOAL_DIM == 256
    assert re.search(r"#define\s+HP_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4       # additions only
    assert "ddpg_agent.py:280-304" in header
    so = os.path.join(REPO, "rl_arm_under_sparse_reward_amd", "librlarm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as entry
        entry.build()
    lib = C.CDLL(so)
    assert all(hasattr(lib, name) for name in names)
    from rl_arm_under_sparse_reward_amd.arguments import Args
    assert Args().eval_metrics is False


def test_the_two_kernels_use_no_scratch_and_no_lds(tmp_path):
    """Exactly two kernels in the unit; private_segment_fixed_size 0, no spilled register, LDS under 1 KB (none at all: the
    reductions cross the wave through ds_swizzle and readlane).  The figures are DESIGN 3.7's."""
    meta = kernel_metadata(tmp_path, "episode_stats.hip")
    print(meta)
    assert len(meta) == 2, sorted(meta)
    assert all("k_episode_stats" in n for n in meta) and sum("k_episode_stats_summary" in n for n in meta) == 1, sorted(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] < 1024, (name, m)
        assert m["vgpr_count"] <= 64, (name, m)        # a one-wave workgroup far below any occupancy limit
