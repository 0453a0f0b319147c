"""The actor-signal audit without a device: the host twins (synthetic.episode_signal_stats / episode_signal_summary) on a block
written out by hand and on a linear critic; the oracle's own count of ReLU ties on every case test_gpu_episode_action_grad.py
runs with freshly initialised networks (the cap that test relies on); the ABI's five new entries; and the static figures of the
new unit's kernels from a cross-compile."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import action_grad_cases as cases
from conftest import REPO, bits
from kernel_metadata import kernel_metadata
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.synthetic import SIGNAL_STATS, episode_signal_stats, episode_signal_summary


def test_columns_of_a_hand_written_block():
    """One episode, T = 3, two action components, max_action 0.5, action_l2 1, flat 0.5; every value is dyadic or a 3-4-5
    triangle, so what is expected is exact.
    step 0: pi = (0.25, -0.25), a = (0.5, -0.25), g = (3, 4): v = (.5, -.5), d = (.5, 0), |g| = 5, |v| = sqrt(.5), |d| = .5,
            g.d = 1.5, cos = 1.5 / 2.5 = 0.6; s = ((3 - .5) * .75, (4 + .5) * .75) = (1.875, 3.375)
    step 1: pi = (0.25, 0), a = (0, 0.5), g = (0, 0): the critic is flat; v = (.5, 0), d = (-.5, 1); |g| = 0 < flat, the
            regulariser outweighs it (1 * 1 * .5 > 0), the cosine counts 0 (zero-norm rule), g.d = 0; s = (-.5 * .75, 0)
    step 2: pi = a = (0, 0.25), g = (0, -0.25): v = (0, .5), d = 0: |g| = .25 < flat, reg: .5 > .25, the cosine counts 0
            (|d| = 0), g.d = 0; s = (0, (-.25 - .5) * .75) = (0, -.5625)"""
    assert SIGNAL_STATS == ("grad_norm", "flat_share", "reg_share", "toward_recorded", "linear_adv", "trunk_signal")
    pi = np.array([[[0.25, -0.25], [0.25, 0.0], [0.0, 0.25]]], dtype=np.float32)
    actions = np.array([[[0.5, -0.25], [0.0, 0.5], [0.0, 0.25]]], dtype=np.float64)
    g = np.array([[[3.0, 4.0], [0.0, 0.0], [0.0, -0.25]]], dtype=np.float32)
    got = episode_signal_stats(pi, g, actions, 0.5, action_l2=1.0, flat=0.5)
    s0 = math.sqrt(1.875 * 1.875 + 3.375 * 3.375)
    want = np.array([[(5.0 + 0.0 + 0.25) / 3.0, 2.0 / 3.0, 2.0 / 3.0, (0.6 + 0.0 + 0.0) / 3.0, (1.5 + 0.0 + 0.0) / 3.0,
                      ((s0 + 0.375) + 0.5625) / 3.0]])
    assert got.dtype == np.float64 and got.shape == (1, 6) and np.array_equal(bits(got), bits(want)), (got, want)
    # the zero-norm rule alone: a flat critic everywhere, and recorded actions equal to the policy's everywhere
    flat_critic = episode_signal_stats(pi, np.zeros_like(g), actions, 0.5)
    assert flat_critic[0, 0] == 0.0 and flat_critic[0, 1] == 1.0 and flat_critic[0, 3] == 0.0 and flat_critic[0, 4] == 0.0
    on_policy = episode_signal_stats(pi, g, pi.astype(np.float64), 0.5)
    assert on_policy[0, 3] == 0.0 and on_policy[0, 4] == 0.0 and np.isfinite(on_policy).all()
    # no regulariser: nothing outweighs a critic that is not flat, and what reaches the trunk is g * tanh'
    free = episode_signal_stats(pi, g, actions, 0.5, action_l2=0.0, flat=0.0)
    assert free[0, 1] == 0.0 and free[0, 2] == 0.0
    assert free[0, 5] == ((math.sqrt(2.25 * 2.25 + 3.0 * 3.0) + 0.0) + 0.1875) / 3.0
    two = np.concatenate([got, free])
    assert np.array_equal(bits(episode_signal_summary(two)), bits((got[0] + free[0]) / 2.0))
    assert np.array_equal(episode_signal_summary(got), got[0])


def test_linear_adv_of_a_linear_critic_is_the_exact_advantage():
    """Q(s, u) = w . u + b: dQ/du = w at every u, so sum_j g_j d_j with d = (a - pi) / M is Q(s, a) - Q(s, pi(s)).  Dyadic
    values: exact in float64."""
    rs = np.random.RandomState(2)
    n, T, ad, M = 3, 5, 4, 0.5
    w = (rs.randint(-8, 9, ad) / 4.0).astype(np.float32)
    pi = (rs.randint(-16, 17, (n, T, ad)) / 32.0).astype(np.float32)
    actions = rs.randint(-16, 17, (n, T, ad)) / 32.0
    g = np.broadcast_to(w, pi.shape).astype(np.float32)
    q = lambda a: (np.asarray(a, dtype=np.float64) / M) @ w.astype(np.float64) + 0.75     # noqa: E731
    got = episode_signal_stats(pi, g, actions, M)
    adv = (q(actions) - q(pi)).mean(axis=1)
    assert np.allclose(got[:, 4], adv, rtol=0, atol=1e-15) and np.abs(adv).max() > 0.1
    assert np.allclose(got[:, 0], math.sqrt(float((w.astype(np.float64) ** 2).sum())), rtol=1e-15, atol=0)


def test_what_is_refused_on_the_host():
    pi = np.zeros((1, 3, 2), np.float32)
    with pytest.raises(ValueError, match="pi \\[n, T, act\\] float32"):
        episode_signal_stats(pi.astype(np.float64), pi, pi, 0.5)
    with pytest.raises(ValueError, match="pi \\[n, T, act\\] float32"):
        episode_signal_stats(pi, pi[:, :2], pi, 0.5)
    with pytest.raises(ValueError, match="max_action"):
        episode_signal_stats(pi, pi, pi, 0.0)
    with pytest.raises(ValueError, match="action_l2"):
        episode_signal_stats(pi, pi, pi, 0.5, action_l2=-1.0)
    with pytest.raises(ValueError, match="flat"):
        episode_signal_stats(pi, pi, pi, 0.5, flat=float("nan"))
    with pytest.raises(ValueError, match="stats \\[n >= 1, 6\\]"):
        episode_signal_summary(np.zeros((0, 6)))


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_relu_ties_of_the_gpu_tests_cases_counted_by_the_oracle_alone(shape):
    """For every case test_gpu_episode_action_grad.py runs on freshly initialised networks (action_grad_cases.fresh_parameters:
    the parameters, statistics and inputs are made without a device and loaded into the agent there), the number of rows with a
    critic pre-activation below RELU_NOISE in float64: at most 1 per case, which is what that test's cap on excused rows relies
    on.  The float32 oracle is also held to the float64 one here, so that the GPU test's bar is known to be one the reference's
    own arithmetic meets."""
    params = cases.fresh_parameters(shape)
    seen = 0
    for block in cases.BLOCKS:
        for clip_obs in cases.CLIPS:
            for at in cases.ATS:
                o, x, _ = cases.fresh_case_oracle(shape, block, clip_obs, at, params)
                ties = int(o["tie"].sum())
                seen += ties
                assert ties <= 1, (shape, block, clip_obs, at, ties, o["min_preact"].min())
                keep = ~o["tie"]
                gmax = float(np.abs(o["g64"]).max())
                assert gmax > 0 and np.isfinite(o["g32"]).all()
                if keep.any():
                    assert np.abs(o["g32"][keep] - o["g64"][keep]).max() <= 1e-4 * gmax, (shape, block, clip_obs, at)
                if clip_obs < 1.0 and block[0] * block[1] > 4:
                    assert np.mean(np.abs(x) < cases.CLIP_RANGE) > 0.5 and len(np.unique(x)) < x.size       # the clip bites: repeated values
    print(f"{shape}: {seen} tie-flagged rows in {len(cases.BLOCKS) * len(cases.CLIPS) * len(cases.ATS)} cases")


def test_header_ctypes_table_and_exports_carry_the_new_entries():
    header = open(os.path.join(REPO, "include", "rlarm_hip.h")).read()
    names = ("hp_episode_action_grad", "hp_episode_action_grad_block", "hp_episode_signal_stats", "hp_episode_signal_stats_block",
             "hp_episode_signal_summary")
    for name in names:
        assert name in _lib.PROTOTYPES and name not in _lib.DEBUG_SYMBOLS, name
        decl = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.PROTOTYPES[name][1]), name       # one ctypes argument per parameter
    assert re.search(r"#define\s+HP_SIGNAL_STATS\s+6\b", header) and _lib.SIGNAL_STATS == 6 == len(SIGNAL_STATS)
    assert re.search(r"#define\s+HP_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4       # additions only
    so = os.path.join(REPO, "rl_arm_under_sparse_reward_amd", "librlarm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as entry
        entry.build()
    lib = C.CDLL(so)
    assert all(hasattr(lib, name) for name in names)
    from rl_arm_under_sparse_reward_amd.arguments import Args
    assert Args().audit_actor_signal is False


def test_the_new_units_kernels_use_no_scratch(tmp_path):
    """episode_action_grad.hip holds exactly two kernels.  Neither uses scratch or spills a register; k_episode_action_grad has
    the policy slab's LDS plus two mask planes (2 x 256 x 2 B) and the four action columns (4 x 256 x 4 B), below the 160 KiB of
    a CU, at 512 threads and two waves per SIMD; the one-wave kernel has no LDS."""
    meta = kernel_metadata(tmp_path, "episode_action_grad.hip")
    print(meta)
    assert len(meta) == 2, sorted(meta)
    named = {want: [n for n in meta if re.search(rf"{want}(?![a-z_])", n)] for want in ("k_episode_action_grad", "k_episode_signal_stats")}
    assert all(len(v) == 1 for v in named.values()), (named, sorted(meta))
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 160 * 1024, (name, m)
    slab = meta[named["k_episode_action_grad"][0]]
    policy = [m for n, m in kernel_metadata(tmp_path, "episode_policy.hip").items() if re.search(r"k_episode_policy(?![a-z_])", n)]
    assert len(policy) == 1 and slab["group_segment_fixed_size"] == policy[0]["group_segment_fixed_size"] + 2 * 256 * 2 + 4 * 256 * 4
    assert slab["vgpr_count"] <= 128, slab                                             # 512 threads at two waves per SIMD
    stats = meta[named["k_episode_signal_stats"][0]]
    assert stats["group_segment_fixed_size"] < 1024 and stats["vgpr_count"] <= 64, stats
