"""The Bellman audit without a device: the host twins (synthetic.episode_bellman_targets / episode_bellman_stats /
episode_bellman_summary) on arrays written out by hand, the ABI's four new entries, and the static figures of the new unit's
kernels from a cross-compile."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO, bits
from kernel_metadata import kernel_metadata
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.synthetic import (BELLMAN_STATS, bellman_constants, episode_bellman_stats, episode_bellman_summary,
                                                      episode_bellman_targets)

f32 = lambda *v: np.array([v], dtype=np.float32)


def test_targets_hit_the_clamp_on_both_sides_and_lie_inside_it():
    """gamma 0.5: clip 2, every value dyadic, so what is expected is exact.  Steps: inside the clamp (-1 + .5 * -1 = -1.5), on the
    floor from below (-1 + .5 * -3 = -2.5 -> -2), on the ceiling from above (-0 + .5 * 1 = .5 -> 0), exactly the floor and exactly
    the ceiling (unchanged: not clipped), and a dense reward inside it."""
    assert BELLMAN_STATS == ("td_mean", "td_abs", "td_sq", "target_mean", "clipped_share", "reward_mean")
    gamma32, clip32 = bellman_constants(0.5)
    assert gamma32.dtype == clip32.dtype == np.float32 and gamma32 == 0.5 and clip32 == 2.0
    assert bellman_constants(0.98) == (np.float32(0.98), np.float32(1.0 / (1.0 - 0.98)))
    r = f32(-1.0, -1.0, -0.0, -1.0, -0.0, -0.25)
    q_next = f32(-1.0, -3.0, 1.0, -2.0, 0.0, -0.5)
    y = episode_bellman_targets(q_next, r, gamma32, clip32)
    assert y.dtype == np.float32 and np.array_equal(y, f32(-1.5, -2.0, 0.0, -2.0, 0.0, -0.5))
    q = f32(-1.0, -1.0, -0.5, -2.0, 0.25, -0.5)
    got = episode_bellman_stats(q, q_next, r, y, gamma32)
    d = [-0.5, -1.0, 0.5, 0.0, -0.25, 0.0]
    want = np.array([[sum(d) / 6.0, sum(abs(v) for v in d) / 6.0, sum(v * v for v in d) / 6.0, -6.0 / 6.0, 2.0 / 6.0, -3.25 / 6.0]])
    assert got.dtype == np.float64 and got.shape == (1, 6) and np.array_equal(bits(got), bits(want)), (got, want)
    # a y that is not the update's: every step whose raw value differs counts, whatever the side
    assert episode_bellman_stats(q, q_next, r, y - np.float32(0.25), gamma32)[0, 4] == 1.0
    two = np.concatenate([got, got * 3.0])
    assert np.array_equal(bits(episode_bellman_summary(two)), bits((got[0] + got[0] * 3.0) / 2.0))
    assert np.array_equal(episode_bellman_summary(got), got[0])


@pytest.mark.parametrize("T", [1, 64, 65, 70])
def test_the_columns_are_left_to_right_sums_in_ascending_t(T):
    """Every column is the plain ascending loop over t (a large first term makes the float64 sums depend on the order), not
    numpy's pairwise sum.  T = 1, 64, 65, 70: the device's chunk loop ends, fills and wraps there."""
    rs = np.random.RandomState(T)
    n = 3
    q_next = rs.normal(-3, 2, (n, T)).astype(np.float32)
    r = -(rs.uniform(size=(n, T)) < 0.7).astype(np.float32)
    q = rs.normal(-3, 2, (n, T)).astype(np.float32)
    q[:, 0] = np.float32(-2.0 ** 30)
    gamma32, clip32 = bellman_constants(0.98)
    y = episode_bellman_targets(q_next, r, gamma32, clip32)
    assert ((y > -clip32) & (y < 0)).any() and (y <= 0).all() and (y >= -clip32).all()
    got = episode_bellman_stats(q, q_next, r, y, gamma32)
    d = y.astype(np.float64) - q.astype(np.float64)
    for e in range(n):
        cols = [d[e], np.abs(d[e]), d[e] * d[e], y[e].astype(np.float64), None, r[e].astype(np.float64)]
        for k, terms in enumerate(cols):
            if terms is None:
                clipped = int(((r[e] + gamma32 * q_next[e]) != y[e]).sum())
                assert got[e, k] == clipped / T
                assert clipped == int(((r[e] + gamma32 * q_next[e] > 0) | (r[e] + gamma32 * q_next[e] < -clip32)).sum())
                continue
            acc = 0.0
            for v in terms.tolist():
                acc = acc + v
            assert got[e, k] == acc / T, (e, k)


def test_a_sparse_reward_of_negative_zero_and_the_sign_of_reward_mean():
    """Every sum starts at +0.0, as in the other audits' columns, and +0.0 + -0.0 is +0.0 in round-to-nearest: no order of an
    episode's steps lets the sign of a -0.0 reward reach reward_mean, so the mean of rewards that are all -0.0 has the bits of
    +0.0 (the device's loop is the same and is compared bit for bit in test_gpu_episode_bellman.py).  The sign does reach y: with
    q_next = -0.0 the target -0.0 + gamma * -0.0 is -0.0, and it counts as unclipped."""
    gamma32, clip32 = bellman_constants(0.98)
    r = np.full((1, 5), -0.0, dtype=np.float32)
    assert np.signbit(r).all()
    q_next = np.full((1, 5), -1.0, dtype=np.float32)
    y = episode_bellman_targets(q_next, r, gamma32, clip32)
    assert np.array_equal(bits(y), bits(np.full((1, 5), -gamma32, dtype=np.float32)))        # -0.0 + x is x
    got = episode_bellman_stats(y, q_next, r, y, gamma32)
    assert got[0, 5] == 0.0 and not np.signbit(got[0, 5]) and got[0, 4] == 0.0 and not got[0, :3].any()
    mixed = r.copy()
    mixed[0, 2] = -1.0
    assert episode_bellman_stats(y, q_next, mixed, y, gamma32)[0, 5] == -1.0 / 5.0
    raw = r + gamma32 * np.full((1, 5), -0.0, dtype=np.float32)
    assert np.signbit(raw).all() and episode_bellman_stats(raw, raw, r, raw, gamma32)[0, 4] == 0.0


def test_what_is_refused_on_the_host():
    a = np.zeros((1, 3), np.float32)
    with pytest.raises(ValueError, match="q_next \\[n, T\\] float32"):
        episode_bellman_targets(a.astype(np.float64), a, 0.98, 50.0)
    with pytest.raises(ValueError, match="q_next \\[n, T\\] float32"):
        episode_bellman_targets(a, a[:, :2], 0.98, 50.0)
    with pytest.raises(ValueError, match="q, q_next, r and y"):
        episode_bellman_stats(a, a, a.astype(np.float64), a, 0.98)
    with pytest.raises(ValueError, match="q, q_next, r and y"):
        episode_bellman_stats(a, a, a, a[:, :2], 0.98)
    with pytest.raises(ValueError, match="gamma"):
        episode_bellman_stats(a, a, a, a, 1.5)
    with pytest.raises(ValueError, match="gamma"):
        bellman_constants(1.0)
    with pytest.raises(ValueError, match="stats \\[n >= 1, 6\\]"):
        episode_bellman_summary(np.zeros((0, 6)))


def test_header_ctypes_table_and_exports_carry_the_new_entries():
    header = open(os.path.join(REPO, "include", "rlarm_hip.h")).read()
    names = ("hp_episode_bellman", "hp_episode_bellman_block", "hp_episode_bellman_stats", "hp_episode_bellman_summary")
    for name in names:
        assert name in _lib.PROTOTYPES and name not in _lib.DEBUG_SYMBOLS, name
        decl = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.PROTOTYPES[name][1]), name       # one ctypes argument per parameter
    assert re.search(r"#define\s+HP_BELLMAN_STATS\s+6\b", header) and _lib.BELLMAN_STATS == 6 == len(BELLMAN_STATS)
    assert re.search(r"#define\s+HP_GOAL_DESIRED\s+0\b", header) and _lib.GOAL_DESIRED == 0
    assert re.search(r"#define\s+HP_GOAL_FINAL\s+1\b", header) and _lib.GOAL_FINAL == 1
    assert re.search(r"#define\s+HP_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4       # additions only
    so = os.path.join(REPO, "rl_arm_under_sparse_reward_amd", "librlarm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as entry
        entry.build()
    lib = C.CDLL(so)
    assert all(hasattr(lib, name) for name in names)
    from rl_arm_under_sparse_reward_amd.arguments import Args
    from rl_arm_under_sparse_reward_amd.episode_audit import EpisodeAudit
    assert Args().audit_bellman is False
    assert all(hasattr(EpisodeAudit, m) for m in ("episode_bellman", "episode_bellman_stats", "episode_bellman_stats_host"))


def test_the_new_units_kernels_use_no_scratch(tmp_path):
    """episode_bellman.hip holds exactly two kernels.  Neither uses scratch or spills a register; k_episode_bellman has the policy
    slab's LDS and nothing more, below the 160 KiB of a CU, at 512 threads and two waves per SIMD; the one-wave kernel has no
    LDS."""
    meta = kernel_metadata(tmp_path, "episode_bellman.hip")
    print(meta)
    assert len(meta) == 2, sorted(meta)
    named = {want: [n for n in meta if re.search(rf"{want}(?![a-z_])", n)] for want in ("k_episode_bellman", "k_episode_bellman_stats")}
    assert all(len(v) == 1 for v in named.values()), (named, sorted(meta))
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    slab, stats = meta[named["k_episode_bellman"][0]], meta[named["k_episode_bellman_stats"][0]]
    assert 0 < slab["group_segment_fixed_size"] <= 160 * 1024, slab
    policy = [m for n, m in kernel_metadata(tmp_path, "episode_policy.hip").items() if re.search(r"k_episode_policy(?![a-z_])", n)]
    assert len(policy) == 1 and slab["group_segment_fixed_size"] == policy[0]["group_segment_fixed_size"]
    assert slab["vgpr_count"] <= 128, slab                                             # 512 threads at two waves per SIMD
    assert stats["group_segment_fixed_size"] == 0 and stats["vgpr_count"] <= 64, stats
