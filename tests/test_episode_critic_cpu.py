"""The critic audit without a device: the host twins (synthetic.episode_returns / episode_critic_stats / episode_critic_summary)
on episodes written out by hand, against the sparse return of episode_stats, against the reference's own rewards on goal pairs
within a few ulp of the threshold (tests/golden/reward_adversarial.npz) and against independently written loops; the order of the
critic columns' sums shown to matter; the ABI's five new entries; and the static figures of the new kernels from a cross-compile."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO, bits, load_golden
from cpu_common import pairs_as_episodes
from kernel_metadata import kernel_metadata
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.synthetic import (CRITIC_STATS, episode_critic_stats, episode_critic_summary, episode_returns,
                                                      episode_stats)


def along_one_axis(dist, gd=3):
    """Episodes whose step t has the achieved goal at distance dist[e][t] from the goal along one axis (sqrt(fl(x x)) = |x|)"""
    dist = np.asarray(dist, dtype=np.float64)
    n, T = dist.shape
    g, ag = np.zeros((n, T, gd)), np.zeros((n, T + 1, gd))
    ag[:, 0, :] = 9.0                        # the reset's achieved goal: no step reads it
    ag[:, 1:, 0] = dist
    return ag, g


def test_returns_of_hand_written_episodes():
    """T = 3, gamma = 0.5, threshold 0.05.  Episode 0 misses, misses, succeeds; episode 1 succeeds, misses, misses.  Every G_t
    below is written out by hand; all of them are dyadic, so the expected values are exact."""
    ag, g = along_one_axis([[0.25, 0.125, 0.03125], [0.03125, 0.125, 0.25]])
    # sparse rewards: e0 = (-1, -1, -0), e1 = (-0, -1, -1)
    zero = episode_returns(ag, g, 0.05, 0.5, "sparse", "zero")
    #   e0: G2 = -0 + .5 * 0 = 0;      G1 = -1 + 0 = -1;         G0 = -1 - .5 = -1.5
    #   e1: G2 = -1;                   G1 = -1 - .5 = -1.5;      G0 = -0 - .75 = -.75
    assert zero.dtype == np.float64 and zero.shape == (2, 3)
    assert np.array_equal(bits(zero), bits(np.array([[-1.5, -1.0, 0.0], [-0.75, -1.5, -1.0]])))
    persist = episode_returns(ag, g, 0.05, 0.5, "sparse", "persist")
    #   e0: G3 = -0 / .5 = -0;  G2 = -0 + .5 * -0 = -0;  G1 = -1 + -0 = -1;   G0 = -1.5
    #   e1: G3 = -1 / .5 = -2;  G2 = -1 - 1 = -2;        G1 = -1 - 1 = -2;    G0 = -0 - 1 = -1
    assert np.array_equal(bits(persist), bits(np.array([[-1.5, -1.0, -0.0], [-1.0, -2.0, -2.0]])))
    # dense rewards: minus the distances
    dzero = episode_returns(ag, g, 0.05, 0.5, "dense", "zero")
    #   e0: G2 = -.03125;  G1 = -.125 - .015625 = -.140625;  G0 = -.25 - .0703125 = -.3203125
    #   e1: G2 = -.25;     G1 = -.125 - .125 = -.25;         G0 = -.03125 - .125 = -.15625
    assert np.array_equal(bits(dzero), bits(np.array([[-0.3203125, -0.140625, -0.03125], [-0.15625, -0.25, -0.25]])))
    dpersist = episode_returns(ag, g, 0.05, 0.5, "dense", "persist")
    #   e0: G3 = -.0625;  G2 = -.03125 - .03125 = -.0625;  G1 = -.125 - .03125 = -.15625;  G0 = -.25 - .078125 = -.328125
    #   e1: G3 = -.5;     G2 = -.25 - .25 = -.5;           G1 = -.125 - .25 = -.375;       G0 = -.03125 - .1875 = -.21875
    assert np.array_equal(bits(dpersist), bits(np.array([[-0.328125, -0.15625, -0.0625], [-0.21875, -0.375, -0.5]])))
    # the names and the numbers of the ABI select the same thing
    assert np.array_equal(bits(episode_returns(ag, g, 0.05, 0.5, 1, 1)), bits(dpersist))
    assert np.array_equal(bits(episode_returns(ag, g, 0.05, 0.5, 0, 0)), bits(zero))


def test_undiscounted_returns_are_the_ret_column_and_gamma_zero_gives_the_rewards():
    rs = np.random.RandomState(5)
    for T, gd in ((1, 1), (7, 3), (64, 2), (100, 3)):
        ag, g = rs.uniform(0, 0.5, (6, T + 1, gd)), rs.uniform(0, 0.5, (6, T, gd))
        thr = float(np.median(np.linalg.norm(ag[:, 1:] - g, axis=-1)))
        stats, flags = episode_stats(ag, g, thr)
        G = episode_returns(ag, g, thr, 1.0, "sparse", "zero")
        assert np.array_equal(bits(G[:, 0]), bits(stats[:, 0])) and (T == 1 or 0 < flags.sum() < flags.size)
        # gamma = 0: G_t = r_t.  (By value: with the zero tail a successful step's -0.0 meets +0.0 and comes out +0.0.)
        d = np.linalg.norm(ag[:, 1:] - g, axis=-1)
        for tail in ("zero", "persist"):
            assert np.array_equal(episode_returns(ag, g, thr, 0.0, "sparse", tail), -(d > thr).astype(np.float64))
            assert np.array_equal(episode_returns(ag, g, thr, 0.0, "dense", tail), -d)
        assert np.array_equal(bits(episode_returns(ag, g, thr, 0.0, "dense", "persist")), bits(-d))
    every = episode_returns(ag, g, 10.0, 1.0, "sparse", "zero")         # an episode that succeeds throughout: +0.0, numpy's own sum
    assert np.array_equal(bits(every[:, 0]), bits(np.zeros(6))) and np.array_equal(bits(every[:, 0]), bits(episode_stats(ag, g, 10.0)[0][:, 0]))


def test_rewards_next_to_the_threshold_are_the_references():
    """gamma = 0 with the persisting tail hands the rewards out bit for bit: the reference's float32 on squared distances within
    8 ulp of the boundary, laid out as episodes."""
    adv = load_golden("reward_adversarial.npz")
    want = adv["r_bits"].view(np.float32).astype(np.float64)
    assert set(np.unique(adv["r_bits"])) == {0x80000000, 0xBF800000}
    for T in (1, 64):
        ag, g = pairs_as_episodes(adv["ag"], adv["g"], T)
        r = episode_returns(ag, g, 0.05, 0.0, "sparse", "persist")
        assert np.array_equal(bits(r), bits(want[:r.size].reshape(-1, T)))
        ret = episode_returns(ag, g, 0.05, 1.0, "sparse", "zero")[:, 0]
        assert np.array_equal(ret, want[:r.size].reshape(-1, T).sum(axis=1))


def test_what_is_refused_on_the_host():
    ag, g = along_one_axis([[0.25, 0.125, 0.03125]])
    with pytest.raises(ValueError, match="gamma 1 with tail 'persist'"):
        episode_returns(ag, g, 0.05, 1.0, "sparse", "persist")
    for gamma in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
            episode_returns(ag, g, 0.05, gamma)
    with pytest.raises(ValueError, match="reward_type"):
        episode_returns(ag, g, 0.05, 0.5, "shaped")
    with pytest.raises(ValueError, match="tail"):
        episode_returns(ag, g, 0.05, 0.5, "sparse", "bootstrap")
    with pytest.raises(ValueError, match=r"ag \[n, T\+1, goal\]"):
        episode_returns(ag[:, :-1], g, 0.05, 0.5)
    with pytest.raises(ValueError, match="float32"):
        episode_critic_stats(np.zeros((1, 3)), np.zeros((1, 3)), 0.5)


def loops(q, G, gamma, descending=True):
    """The critic columns as nested loops written here, on numpy float64 scalars, in either order of t"""
    out = []
    for qe, Ge in zip(q, G):
        T = len(qe)
        order = range(T - 1, -1, -1) if descending else range(T)
        sq = sg = sb = sa = np.float64(0)
        mx, steps = np.float64(0), 0
        for t in order:
            qd = np.float64(qe[t])
            sq, sg, sb, sa = sq + qd, sg + Ge[t], sb + (qd - Ge[t]), sa + np.abs(qd - Ge[t])
            mx = max(mx, np.abs(qd - Ge[t]))
            steps += int(gamma < 1 and qd <= -(np.float64(1) / (np.float64(1) - np.float64(gamma))))
        out.append([sq / T, sg / T, sb / T, sa / T, mx, steps])
    return np.array(out, dtype=np.float64)


def test_critic_columns_and_their_summary_against_nested_loops():
    rs = np.random.RandomState(9)
    assert CRITIC_STATS == ("q_mean", "return_mean", "bias", "abs_error", "max_abs_error", "floor_steps")
    for gamma in (0.98, 0.5, 0.0, 1.0):
        for T, n in ((1, 1), (3, 4), (65, 5), (100, 7)):
            ag, g = rs.uniform(0, 0.5, (n, T + 1, 3)), rs.uniform(0, 0.5, (n, T, 3))
            G = episode_returns(ag, g, 0.3, gamma, "dense", "zero")
            q = rs.uniform(-60, 5, (n, T)).astype(np.float32)
            if gamma < 1:
                q[rs.rand(n, T) < 0.2] = np.float32(-1 / (1 - gamma))         # values at the target clip
            got = episode_critic_stats(q, G, gamma)
            assert got.dtype == np.float64 and np.array_equal(bits(got), bits(loops(q, G, gamma))), (gamma, T, n)
            if gamma == 1.0:
                assert not got[:, 5].any()
            elif gamma in (0.5, 0.0) and n * T > 10:
                # -2 and -1 are float32 values: Q exactly at the clip counts; -1 / (1 - 0.98) rounds below the float64 bound and counts too
                assert (got[:, 5].sum() >= (q == np.float32(-1 / (1 - gamma))).sum() > 0)
            total = [0.0] * 6
            for row in got.tolist():
                for k in range(6):
                    total[k] = total[k] + row[k]
            summary = episode_critic_summary(got)
            assert summary.dtype == np.float64 and np.array_equal(bits(summary), bits(np.array([t / n for t in total])))
    assert np.array_equal(episode_critic_summary(got[:1]), got[0])


def test_the_descending_order_of_the_sums_matters():
    """Q = (1, 2^-53, 2^-53), G = 0: descending, the two small terms meet first and their sum 2^-52 survives next to 1;
    ascending, each is rounded away on its own."""
    q = np.array([[1.0, 2.0**-53, 2.0**-53]], dtype=np.float32)
    G = np.zeros((1, 3))
    got = episode_critic_stats(q, G, 0.5)
    assert got[0, 0] == (1.0 + 2.0**-52) / 3.0 and got[0, 2] == got[0, 0] and got[0, 3] == got[0, 0]
    assert np.array_equal(bits(got), bits(loops(q, G, 0.5, descending=True)))
    ascending = loops(q, G, 0.5, descending=False)
    assert ascending[0, 0] == 1.0 / 3.0 and not np.array_equal(bits(got), bits(ascending))


def test_header_ctypes_table_and_exports_carry_the_new_entries():
    header = open(os.path.join(REPO, "include", "rlarm_hip.h")).read()
    names = ("hp_episode_q", "hp_episode_q_block", "hp_episode_returns", "hp_episode_returns_block", "hp_episode_critic_summary")
    for name in names:
        assert name in _lib.PROTOTYPES and name not in _lib.DEBUG_SYMBOLS, name
        decl = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.PROTOTYPES[name][1]), name       # one ctypes argument per parameter
    assert re.search(r"#define\s+HP_CRITIC_STATS\s+6\b", header) and _lib.CRITIC_STATS == 6 == len(CRITIC_STATS)
    assert re.search(r"#define\s+HP_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4       # additions only
    assert "ddpg_agent.py:259-260" in header
    so = os.path.join(REPO, "rl_arm_under_sparse_reward_amd", "librlarm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as entry
        entry.build()
    lib = C.CDLL(so)
    assert all(hasattr(lib, name) for name in names)
    from rl_arm_under_sparse_reward_amd.arguments import Args
    assert Args().eval_critic is False


def test_the_q_kernel_is_one_kernel_without_scratch(tmp_path):
    """episode_q.hip holds exactly one kernel: no scratch, no spilled register, the policy slab's LDS (one workgroup per CU).
    The figures are DESIGN 3.7's."""
    meta = kernel_metadata(tmp_path, "episode_q.hip")
    print(meta)
    assert len(meta) == 1 and "k_episode_q" in next(iter(meta)), sorted(meta)
    m = next(iter(meta.values()))
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["group_segment_fixed_size"] == 111552 <= 163840, m         # PolicyLds and nothing else
    assert m["vgpr_count"] <= 128, m                                    # 512 threads at two waves per SIMD


def test_the_returns_kernels_use_no_scratch_and_no_lds(tmp_path):
    """Exactly two kernels in episode_returns.hip; no scratch, no spill, no LDS at all (the recursion takes its operands out of
    the lanes with v_readlane): a one-wave workgroup far below any occupancy limit."""
    meta = kernel_metadata(tmp_path, "episode_returns.hip")
    print(meta)
    assert len(meta) == 2, sorted(meta)
    assert sum("k_episode_returns" in n for n in meta) == 1 and sum("k_episode_column_means" in n for n in meta) == 1, sorted(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] < 1024, (name, m)
        assert m["vgpr_count"] <= 64, (name, m)
