"""The policy audit without a device: the host twins (synthetic.episode_policy_stats / episode_policy_summary) on arrays written
out by hand and against independently written loops; the ABI's five new entries; and the static figures of the new unit's kernels
from a cross-compile."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO, bits
from kernel_metadata import kernel_metadata
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.synthetic import POLICY_STATS, episode_policy_stats, episode_policy_summary

NAN = np.uint64(0x7FF8000000000000)       # the quiet NaN the device writes and float("nan") is


def test_columns_of_hand_written_episodes():
    """T = 2, two action components, max_action 0.5; every value is dyadic, so what is expected is exact.
    Episode 0: pi = a everywhere and Q(s, a) = Q(s, pi): no gap, no advantage, nothing filtered, nothing saturated (|pi| = 0.25).
    Episode 1: pi = +-0.5 (every component saturated), the recorded actions 0.3, 0.4 away in step 0 (distance 0.5) and equal in
    step 1, and the critic prefers the recorded action at every step."""
    assert POLICY_STATS == ("q_pi_mean", "advantage_mean", "q_filter_share", "action_gap_mean", "saturated_share", "action_l2_mean")
    pi = np.array([[[0.25, -0.25], [0.25, 0.25]], [[0.5, -0.5], [-0.5, 0.5]]], dtype=np.float32)
    actions = pi.astype(np.float64)
    actions[1, 0] = [0.5 - 0.1875, -0.5 + 0.25]          # d = (-0.1875, 0.25): 0.03515625 + 0.0625 = 0.09765625 = 0.3125^2
    q_pi = np.array([[-1.0, -3.0], [-4.0, -8.0]], dtype=np.float32)
    q = np.array([[-1.0, -3.0], [-3.5, -7.0]], dtype=np.float32)
    got = episode_policy_stats(pi, q_pi, actions, 0.5, q=q)
    want = np.array([[-2.0, 0.0, 0.0, 0.0, 0.0, 0.25],           # l2: ((.5^2 + .5^2) / 2) twice / 2
                     [-6.0, -0.75, 1.0, 0.3125, 1.0, 1.0]])      # gap: (0.3125 + 0) / 0.5 / 2
    assert got.dtype == np.float64 and got.shape == (2, 6) and np.array_equal(bits(got), bits(want)), got
    summary = episode_policy_summary(got)
    assert np.array_equal(bits(summary), bits(np.array([-4.0, -0.375, 0.5, 0.15625, 0.5, 0.625])))
    assert np.array_equal(episode_policy_summary(got[1:]), got[1])


def test_sat_exactly_on_a_component_counts():
    """|pi| >= sat * max_action: a component exactly on the bound is saturated, the float32 below it is not.  max_action is the
    networks' float32, so the bound is formed from float32(0.7) widened, not from the double 0.7."""
    ma = float(np.float32(0.7))
    on = np.float32(0.5 * ma)                # 0.5 * float32 is exact in float32 and in float64
    assert float(on) == 0.5 * ma
    below = np.nextafter(on, np.float32(0))
    pi = np.array([[[on, below, -on]]], dtype=np.float32)
    got = episode_policy_stats(pi, np.zeros((1, 1), np.float32), pi.astype(np.float64), 0.7, sat=0.5)
    assert got[0, 4] == 2.0 / 3.0
    assert episode_policy_stats(pi, np.zeros((1, 1), np.float32), pi.astype(np.float64), 0.7, sat=1.0)[0, 4] == 0.0
    assert episode_policy_stats(pi, np.zeros((1, 1), np.float32), pi.astype(np.float64), 0.7, sat=0.0)[0, 4] == 1.0
    # the default: 0.99
    pi = np.array([[[0.5, 0.49, -0.4949, -0.496]]], dtype=np.float32)
    assert episode_policy_stats(pi, np.zeros((1, 1), np.float32), pi.astype(np.float64), 0.5)[0, 4] == 0.5


def test_without_q_two_columns_are_nan_and_the_rest_unchanged():
    rs = np.random.RandomState(3)
    pi = rs.uniform(-0.5, 0.5, (3, 7, 4)).astype(np.float32)
    actions = rs.uniform(-0.5, 0.5, (3, 7, 4))
    q_pi, q = rs.normal(-5, 2, (3, 7)).astype(np.float32), rs.normal(-5, 2, (3, 7)).astype(np.float32)
    both, alone = episode_policy_stats(pi, q_pi, actions, 0.5, q=q), episode_policy_stats(pi, q_pi, actions, 0.5)
    assert np.isfinite(both).all()
    assert (np.ascontiguousarray(alone[:, 1:3]).view(np.uint64) == NAN).all()
    keep = [0, 3, 4, 5]
    assert np.array_equal(bits(alone[:, keep]), bits(both[:, keep]))
    summary = episode_policy_summary(alone)
    assert np.isnan(summary[1:3]).all() and np.array_equal(bits(summary[keep]), bits(episode_policy_summary(both)[keep]))


def loops(pi, q_pi, actions, max_action, q, sat):
    """The columns as nested loops written here, on numpy float64 scalars"""
    ma = np.float64(np.float32(max_action))
    out = []
    for e in range(pi.shape[0]):
        T, ad = pi.shape[1:]
        s_q = s_a = s_g = s_l = np.float64(0)
        filt = satd = 0
        for t in range(T):
            s_q = s_q + np.float64(q_pi[e, t])
            s_a = s_a + (np.float64(q_pi[e, t]) - np.float64(q[e, t]))
            filt += int(q[e, t] > q_pi[e, t])
            dd = vv = np.float64(0)
            for j in range(ad):
                p = np.float64(pi[e, t, j])
                dd = dd + (actions[e, t, j] - p) * (actions[e, t, j] - p)
                vv = vv + (p / ma) * (p / ma)
                satd += int(np.abs(p) >= np.float64(sat) * ma)
            s_g = s_g + np.sqrt(dd)
            s_l = s_l + vv / np.float64(ad)
        out.append([s_q / T, s_a / T, np.float64(filt) / T, s_g / ma / T, np.float64(satd) / np.float64(T * ad), s_l / T])
    return np.array(out, dtype=np.float64)


def test_columns_and_their_summary_against_nested_loops():
    rs = np.random.RandomState(9)
    for T, n, ad, ma in ((1, 1, 1, 2.0), (1, 3, 4, 0.5), (3, 4, 3, 0.7), (65, 5, 4, 0.5), (130, 2, 1, 1.0)):
        pi = (ma * np.tanh(rs.normal(0, 2.0, (n, T, ad)))).astype(np.float32)
        actions = np.clip(pi.astype(np.float64) + rs.normal(0, 0.1, pi.shape), -ma, ma)
        q_pi = rs.uniform(-50, 0, (n, T)).astype(np.float32)
        q = q_pi.copy()
        move = rs.rand(n, T) < 0.6
        q[move] += rs.normal(0, 1, move.sum()).astype(np.float32)
        for sat in (0.99, 0.5):
            got = episode_policy_stats(pi, q_pi, actions, ma, q=q, sat=sat)
            assert np.array_equal(bits(got), bits(loops(pi, q_pi, actions, ma, q, sat))), (T, n, ad, ma, sat)
            assert ((0 <= got[:, [2, 4]]) & (got[:, [2, 4]] <= 1)).all() and (got[:, 3] >= 0).all() and (got[:, 5] <= 1).all()
            total = [0.0] * 6
            for row in got.tolist():
                for k in range(6):
                    total[k] = total[k] + row[k]
            assert np.array_equal(bits(episode_policy_summary(got)), bits(np.array([v / n for v in total])))
        if T == 1:                           # a single step: its own terms, nothing summed
            assert np.array_equal(got[:, 0], q_pi[:, 0].astype(np.float64))
            d = actions[:, 0] - pi[:, 0].astype(np.float64)
            gap = np.array([math.sqrt(sum(float(x) * float(x) for x in row)) for row in d]) / float(np.float32(ma))
            assert np.array_equal(bits(got[:, 3]), bits(gap))


def test_what_is_refused_on_the_host():
    pi, q = np.zeros((1, 3, 2), np.float32), np.zeros((1, 3), np.float32)
    with pytest.raises(ValueError, match="pi \\[n, T, act\\] float32"):
        episode_policy_stats(pi.astype(np.float64), q, pi, 0.5)
    with pytest.raises(ValueError, match="pi \\[n, T, act\\] float32"):
        episode_policy_stats(pi, q[:, :2], pi, 0.5)
    with pytest.raises(ValueError, match="q \\[n, T\\] float32"):
        episode_policy_stats(pi, q, pi, 0.5, q=q.astype(np.float64))
    with pytest.raises(ValueError, match="sat"):
        episode_policy_stats(pi, q, pi, 0.5, sat=1.5)
    with pytest.raises(ValueError, match="max_action"):
        episode_policy_stats(pi, q, pi, 0.0)
    with pytest.raises(ValueError, match="stats \\[n >= 1, 6\\]"):
        episode_policy_summary(np.zeros((0, 6)))


def test_header_ctypes_table_and_exports_carry_the_new_entries():
    header = open(os.path.join(REPO, "include", "rlarm_hip.h")).read()
    names = ("hp_episode_policy", "hp_episode_policy_block", "hp_episode_policy_stats", "hp_episode_policy_stats_block",
             "hp_episode_policy_summary")
    for name in names:
        assert name in _lib.PROTOTYPES and name not in _lib.DEBUG_SYMBOLS, name
        decl = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.PROTOTYPES[name][1]), name       # one ctypes argument per parameter
    assert re.search(r"#define\s+HP_POLICY_STATS\s+6\b", header) and _lib.POLICY_STATS == 6 == len(POLICY_STATS)
    assert re.search(r"#define\s+HP_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4       # additions only
    so = os.path.join(REPO, "rl_arm_under_sparse_reward_amd", "librlarm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as entry
        entry.build()
    lib = C.CDLL(so)
    assert all(hasattr(lib, name) for name in names)
    from rl_arm_under_sparse_reward_amd.arguments import Args
    assert Args().audit_policy is False


def test_the_new_units_kernels_use_no_scratch(tmp_path):
    """episode_policy.hip holds exactly two kernels, and its summary is episode_returns.hip's column means.  None uses scratch or
    spills a register; k_episode_policy has the policy slab's LDS (one workgroup per CU, below the 160 KiB of a CU) at 512 threads
    and two waves per SIMD; the two one-wave kernels have no LDS to speak of.  The figures read here are DESIGN 3.7's."""
    meta = kernel_metadata(tmp_path, "episode_policy.hip")
    assert len(meta) == 2, sorted(meta)
    meta.update({n: m for n, m in kernel_metadata(tmp_path, "episode_returns.hip").items() if "k_episode_column_means" in n})
    print(meta)
    assert len(meta) == 3, sorted(meta)
    named = {want: [n for n in meta if re.search(rf"{want}(?![a-z_])", n)] for want in
             ("k_episode_policy", "k_episode_policy_stats", "k_episode_column_means")}
    assert all(len(v) == 1 for v in named.values()), (named, sorted(meta))
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 163840, (name, m)
    slab = meta[named["k_episode_policy"][0]]
    q_only = next(iter(kernel_metadata(tmp_path, "episode_q.hip").values()))
    assert slab["group_segment_fixed_size"] == q_only["group_segment_fixed_size"]       # one PolicyLds and nothing else
    assert slab["vgpr_count"] <= 128, slab                                             # 512 threads at two waves per SIMD
    for want in ("k_episode_policy_stats", "k_episode_column_means"):
        m = meta[named[want][0]]
        assert m["group_segment_fixed_size"] < 1024 and m["vgpr_count"] <= 64, (want, m)
