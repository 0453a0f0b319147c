"""Episode metrics on the device (csrc/episode_stats.hip: hp_episode_stats, hp_episode_stats_block, hp_episode_stats_summary;
DeviceEpisodes.stats, DeviceDemos.stats, collect_episodes_device(stats_out=), ddpg_agent.episode_stats_host, args.eval_metrics)
against the host twin synthetic.episode_stats / episode_stats_summary.  Every comparison is bit for bit: the kernel's reductions
are order independent and the summary's order is fixed."""
import shutil

import numpy as np
import pytest
import torch

from conftest import bits, load_golden
from cpu_common import pairs_as_episodes
from gpu_common import ctx, make_shape_episodes
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd import train_state as ts
from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_CRITIC
from rl_arm_under_sparse_reward_amd.device_env import (NativePickPlaceVecEnv, NativePointMassVecEnv, NativePushBlockVecEnv, PointMassVecEnv,
                                                       generate_demos)
from rl_arm_under_sparse_reward_amd.synthetic import EPISODE_SUMMARY, episode_stats, episode_stats_summary
from episode_common import learner
from rollout_common import CONTACT, DEV, agent_on, agent_pair, dev_ptr as p, make

pytestmark = pytest.mark.gpu


def device_stats(ag, g, thr, steps=True):
    """hp_episode_stats on uploaded arrays, in torch's stream order: (stats, step flags or None) as numpy"""
    c = ctx()
    a, b = torch.from_numpy(np.ascontiguousarray(ag)).to(DEV), torch.from_numpy(np.ascontiguousarray(g)).to(DEV)
    n, T, gd = g.shape
    stats = torch.full((n, 6), float("nan"), dtype=torch.float64, device=DEV)
    flags = torch.full((n, T), float("nan"), dtype=torch.float32, device=DEV) if steps else None
    with c.torch_bridge():
        _lib.check(c.lib.hp_episode_stats(c.h, p(a), p(b), n, T, gd, float(thr), p(stats), p(flags) if steps else None))
    return stats.cpu().numpy(), flags.cpu().numpy() if steps else None


def assert_equals_twin(ag, g, thr, steps=True):
    want, want_flags = episode_stats(ag, g, thr)
    got, got_flags = device_stats(ag, g, thr, steps)
    assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(bits(got), bits(want)), (got, want)
    if steps:
        assert got_flags.dtype == np.float32 and np.array_equal(bits(got_flags), bits(want_flags))
    return want, want_flags


# ------------------------------------------------------------------------------------------ 1. the raw-pointer entry
@pytest.mark.parametrize("T", [1, 63, 64, 65, 100])
def test_raw_entry_equals_the_twin_on_random_episodes(T):
    """Less than a wave of steps, exactly one, one more, and a second round of the lanes; one, two and three goal components;
    one episode, a few, and more workgroups than a wave has lanes.  The threshold is the median distance of the case, so about
    half of the steps succeed -- asserted wherever the case has enough steps for a share to mean something."""
    rs = np.random.RandomState(100 + T)
    for gd in (1, 2, 3):
        for n in (1, 5, 70):
            ag, g = rs.uniform(0, 0.5, (n, T + 1, gd)), rs.uniform(0, 0.5, (n, T, gd))
            thr = float(np.median(np.linalg.norm(ag[:, 1:] - g, axis=-1))) * (1 + 1e-9)
            want, flags = assert_equals_twin(ag, g, thr, steps=(n != 5))            # n = 5: without the step flags
            share = flags.mean()
            print(f"T {T} goal_dim {gd} n {n}: {share:.3f} of the steps succeed, first_success_step up to {want[:, 3].max():.0f}")
            if n * T >= 60:
                assert 0.4 <= share <= 0.6, share
                assert 0 < want[:, 4].sum() < n * T and want[:, 0].min() < 0
    ag, g = rs.uniform(0, 0.5, (5, T + 1, 3)), rs.uniform(0, 0.5, (5, T, 3))
    none, flags = assert_equals_twin(ag, g, 0.0)                     # nothing is closer than 0
    assert flags.sum() == 0 and (none[:, 0] == -T).all() and (none[:, 3] == T).all() and not none[:, 4:].any()
    every, flags = assert_equals_twin(ag, g, 10.0)
    assert flags.mean() == 1 and np.array_equal(bits(every[:, 0]), bits(np.zeros(5))) and not every[:, 3].any()
    assert (every[:, 4] == T).all() and (every[:, 5] == 1).all()


def test_the_summary_equals_the_twins_loop():
    rs = np.random.RandomState(8)
    for n in (1, 5, 70, 1000):
        ag, g = rs.uniform(0, 0.5, (n, 31, 3)), rs.uniform(0, 0.5, (n, 30, 3))
        stats = episode_stats(ag, g, 0.12)[0]
        dev, out = torch.from_numpy(stats).to(DEV), torch.full((6,), float("nan"), dtype=torch.float64, device=DEV)
        with ctx().torch_bridge():
            _lib.check(ctx().lib.hp_episode_stats_summary(ctx().h, p(dev), n, p(out)))
        want = episode_stats_summary(stats)
        assert np.array_equal(bits(out.cpu().numpy()), bits(want)), (n, out, want)
        if n == 1000:
            assert 0 < want[4] < want[5] < 1, want


# ------------------------------------------------------------------------------------------ 2. pairs next to the threshold
def test_pairs_within_a_few_ulp_of_the_threshold():
    """The reference's own outputs on goal pairs whose squared distance lies within a few ulp of the boundary, laid out as
    episodes: the step flags are the fixture's is_success, `ret` the sum of its rewards.  (reward_adversarial.npz records the
    rewards only.)"""
    dense = load_golden("reward_dense_success.npz")
    for thr in (0.05, 0.1):
        for T in (1, 64, 100):
            ag, g = pairs_as_episodes(dense["ag"], dense["g"], T)
            stats, flags = assert_equals_twin(ag, g, thr)
            n = ag.shape[0]
            assert np.array_equal(flags.reshape(-1), dense[f"thr{thr}_success"][:n * T])
            missed = (dense[f"thr{thr}_sparse_bits"][:n * T] == 0xBF800000).reshape(n, T)
            assert np.array_equal(stats[:, 0], -missed.sum(axis=1).astype(np.float64))
    adv = load_golden("reward_adversarial.npz")
    for T in (1, 64):
        ag, g = pairs_as_episodes(adv["ag"], adv["g"], T)
        stats, _ = assert_equals_twin(ag, g, 0.05)
        missed = (adv["r_bits"] == 0xBF800000).reshape(-1, T)
        assert np.array_equal(stats[:, 0], -missed.sum(axis=1).astype(np.float64)) and 0 < missed.sum() < missed.size


# ------------------------------------------------------------------------------------------ 3. a sub-range of a block
def test_a_sub_range_of_a_push_block_collection():
    """Nine episodes on eight environments (two waves) with contact-frequent parameters; episodes [3, 7) into rows [3, 7) of a
    poisoned tensor."""
    a = agent_on(NativePushBlockVecEnv, 8, 20, env_seed=21, env_kw=CONTACT, random_eps=0.3)
    eps = a.collect_episodes_device(n_rollouts=9)
    thr = a.vec_env.distance_threshold
    out = torch.full((9, 6), float("nan"), dtype=torch.float64, device=DEV)
    steps = torch.full((9, eps.T), float("nan"), dtype=torch.float32, device=DEV)
    with a.ctx.torch_bridge():
        _lib.check(a.lib.hp_episode_stats_block(eps.h, 3, 4, thr, p(out[3:]), p(steps[3:])))
    _, ag, g, _ = eps.numpy()
    assert (ag[:, 1:] != ag[:, :-1]).any()                       # the block moved: contact happened
    want, want_steps = episode_stats(ag, g, thr)
    got, got_steps = out.cpu().numpy(), steps.cpu().numpy()
    assert np.array_equal(bits(got[3:7]), bits(want[3:7])) and np.array_equal(bits(got_steps[3:7]), bits(want_steps[3:7]))
    assert np.isnan(got[:3]).all() and np.isnan(got[7:]).all() and np.isnan(got_steps[:3]).all() and np.isnan(got_steps[7:]).all()
    sub, sub_steps = eps.stats(thr, first=3, n=4, step_success=True)
    assert tuple(sub.shape) == (4, 6) and np.array_equal(bits(sub.cpu().numpy()), bits(want[3:7]))
    assert np.array_equal(bits(sub_steps.cpu().numpy()), bits(want_steps[3:7]))
    assert np.array_equal(bits(eps.stats(thr, first=7).cpu().numpy()), bits(want[7:]))
    assert np.array_equal(bits(eps.stats(thr).cpu().numpy()), bits(want))
    half = float(np.median(np.linalg.norm(ag[:, 1:] - g, axis=-1)))     # a threshold at which half of these steps succeed
    wide = episode_stats(ag, g, half)[0]
    assert 0 < wide[:, 4].sum() < 9 * eps.T and np.array_equal(bits(eps.stats(half).cpu().numpy()), bits(wide))


# ------------------------------------------------------------------------------------------ 4. the three rollout forms
@pytest.mark.parametrize("explore", [True, False])
def test_all_three_rollout_forms_hand_out_the_same_stats(explore):
    """Stepped on the tensor twin, fused per wave on the native environment, all waves in one launch with the reset on the
    device: seven episodes on four environments, identically built agents."""
    T = 20
    plain, native = agent_pair((PointMassVecEnv, NativePointMassVecEnv), 4, T, env_seed=10)
    waves = agent_on(NativePointMassVecEnv, 4, T, env_seed=10, reset=True)
    got = []
    for a, form in ((plain, "stepped"), (native, "fused"), (waves, "fused")):
        flags, stats = [], []
        eps = a.collect_episodes_device(n_rollouts=7, explore=explore, success_out=flags, stats_out=stats)
        assert a.rollout_form == form and len(stats) == 1 and tuple(stats[0].shape) == (7, 6) and stats[0].dtype == torch.float64
        s = stats[0].cpu().numpy()
        _, ag, g, _ = eps.numpy()
        assert np.array_equal(bits(s), bits(episode_stats(ag, g, a.vec_env.distance_threshold)[0])), form
        won = torch.cat([f.reshape(-1) for f in flags]).cpu().numpy()
        assert np.array_equal(s[:, 5], won.astype(np.float64)), form
        got.append(s)
    assert waves.rollout_launches == 1 and native.rollout_launches == 2
    assert np.array_equal(bits(got[0]), bits(got[1])) and np.array_equal(bits(got[1]), bits(got[2]))
    assert (got[0][:, 2] <= got[0][:, 1]).all() and (got[0][:, 1] > 0).all()
    # without stats_out nothing is handed out and the episodes are the same
    again = agent_on(NativePointMassVecEnv, 4, T, env_seed=10)
    same = again.collect_episodes_device(n_rollouts=7, explore=explore).numpy()
    for x, y in zip(same, native._rollouts[7].numpy()):
        assert np.array_equal(bits(x), bits(y))


# ------------------------------------------------------------------------------------------ 5. demonstrations
def test_the_stats_of_pick_and_place_demonstrations():
    env = NativePickPlaceVecEnv(4, seed=0, device=DEV, max_timesteps=100, step_scale=0.2)
    env.enable_device_reset(ctx())
    demos = generate_demos(env, 4)
    assert demos.kept == 4
    stats, steps = demos.stats(env.distance_threshold, step_success=True)
    info = demos.info.cpu().numpy()
    assert np.array_equal(bits(steps.cpu().numpy()), bits(info)) and 0 < info.sum() < info.size
    s = stats.cpu().numpy()
    assert np.array_equal(s[:, 3], info.argmax(axis=1).astype(np.float64)) and (s[:, 3] > 0).all() and (s[:, 5] == 1).all()
    _, ag, g, _, _ = demos.numpy()
    assert np.array_equal(bits(s), bits(episode_stats(ag, g, env.distance_threshold)[0]))
    assert np.array_equal(bits(demos.stats(env.distance_threshold).cpu().numpy()), bits(s))


# ------------------------------------------------------------------------------------------ 6. host episodes
def test_host_episodes_through_the_same_kernel():
    torch.manual_seed(0)
    a = make(None)
    for T, gd, n in ((50, 3, 6), (7, 2, 1)):
        batch = make_shape_episodes(n, 12, gd, 4, T)
        thr = float(np.median(np.linalg.norm(batch[1][:, 1:] - batch[2], axis=-1)))
        stats, steps = a.episode_stats_host(batch, thr)
        want, want_steps = episode_stats(batch[1], batch[2], thr)
        assert isinstance(stats, np.ndarray) and np.array_equal(bits(stats), bits(want)) and np.array_equal(bits(steps), bits(want_steps))
        assert 0 < want_steps.sum() < want_steps.size
    with pytest.raises(ValueError, match="episode_stats_host: ag"):
        a.episode_stats_host([batch[0], batch[1][:, :-1], batch[2], batch[3]], 0.05)


# ------------------------------------------------------------------------------------------ 7. evaluation metrics in learn()
def evaluation_episodes(a):
    """The calls of _eval_agent_device made by hand: (ag, g) of the evaluation episodes, in order"""
    ags, gs, remaining = [], [], int(a.args.n_test_rollouts)
    while remaining > 0:
        k = remaining if a.vec_env.reset_streams is not None else min(a.vec_env.n_envs, remaining)
        _, ag, g, _ = a.collect_episodes_device(n_rollouts=k, explore=False).numpy()
        ags.append(ag); gs.append(g)
        remaining -= k
    return np.concatenate(ags), np.concatenate(gs)


def epoch_by_hand(a, epoch):
    """One epoch of _learn_device and the collections of its evaluation"""
    for _ in range(a.args.n_cycles):
        a.train_cycle(a.collect_episodes_device(n_rollouts=a.args.num_rollouts_per_mpi, epoch=epoch))
    a.ctx.synchronize()
    return evaluation_episodes(a)


@pytest.mark.parametrize("reset", [False, True], ids=["wave_calls", "one_launch"])
def test_eval_metrics_are_the_twins_and_change_nothing_else(tmp_path, reset, capsys):
    """Two epochs of learn() with the option on and off: the same rates, parameters and training state to the byte, an empty
    list with it off; with it on, success_rate is the rate and every other field the twin's on the evaluation episodes --
    collected again by a twin agent for epoch 0, and for epoch 1 by an agent restored from the state the run saved after epoch 0."""
    on = learner(tmp_path, "on", reset, eval_metrics=True, state_path=str(tmp_path / "on.npz"))
    save, host_resets = on._save_epoch_state, {}

    def save_and_keep(path, epoch):          # the state after every epoch, and the simulator's own host generators beside it
        out = save(path, epoch)
        shutil.copy(ts.rank_path(path, 0), tmp_path / f"after{epoch}.npz")
        host_resets[epoch] = [r.get_state() for r in on.vec_env.rs]
        return out

    on._save_epoch_state = save_and_keep
    off = learner(tmp_path, "off", reset, state_path=str(tmp_path / "off.npz"))
    printed = []
    for a in (on, off):
        np.random.seed(11)
        a.learn()
        printed.append([line for line in capsys.readouterr().out.splitlines() if "eval success rate" in line])
    assert off.eval_metrics == [] and len(on.eval_metrics) == 2 and len(on.success_rates) == 2
    assert on.success_rates == off.success_rates
    assert [line.split("] ", 1)[1] for line in printed[0]] == [line.split("] ", 1)[1] for line in printed[1]] and len(printed[0]) == 2
    for slot in (NET_ACTOR, NET_CRITIC):
        assert np.array_equal(bits(on._get_flat(slot)), bits(off._get_flat(slot))), slot
    sa, sb = ts.read_state(ts.rank_path(str(tmp_path / "on.npz"), 0)), ts.read_state(ts.rank_path(str(tmp_path / "off.npz"), 0))
    assert sorted(sa[0]) == sorted(sb[0])
    for name in sa[0]:
        assert np.array_equal(bits(sa[0][name]), bits(sb[0][name])), name
    # the evaluation episodes again
    twin, restored = learner(tmp_path, "twin", reset), learner(tmp_path, "restored", reset)
    for a in (twin, restored):               # what learn() does before its first epoch
        a.enable_explore_streams()
        if reset:
            a.vec_env.enable_device_reset(a.ctx)
    np.random.seed(11)
    twin.rng.set_state(np.random.get_state())
    restored.load_training_state(str(tmp_path / "after1.npz"))
    assert restored.resumed_at[0] == 1
    for r, state in zip(restored.vec_env.rs, host_resets[1]):
        r.set_state(state)
    for i, a in enumerate((twin, restored)):
        ag, g = epoch_by_hand(a, i)
        want = episode_stats_summary(episode_stats(ag, g, 0.15)[0])
        m = on.eval_metrics[i]
        assert tuple(m) == EPISODE_SUMMARY and m["success_rate"] == on.success_rates[i]
        assert np.array_equal(bits(np.array([m[k] for k in EPISODE_SUMMARY])), bits(want)), (i, m, want)
        assert m["min_distance"] <= m["final_distance"] and m["any_success_rate"] >= m["success_rate"]


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_carry_the_librarys_message():
    c = ctx()
    lib = c.lib
    ag, g = torch.zeros((2, 4, 3), dtype=torch.float64, device=DEV), torch.zeros((2, 3, 3), dtype=torch.float64, device=DEV)
    out, steps = torch.zeros((2, 6), dtype=torch.float64, device=DEV), torch.zeros((2, 3), dtype=torch.float32, device=DEV)
    summary = torch.zeros(6, dtype=torch.float64, device=DEV)

    def refused(status, text):
        assert status == -1                                     # HP_ERR_INVALID
        with pytest.raises(ValueError, match=text):
            _lib.check(status)

    for args in ((None, p(ag), p(g), 2, 3, 3, 0.05, p(out), p(steps)), (c.h, None, p(g), 2, 3, 3, 0.05, p(out), p(steps)),
                 (c.h, p(ag), None, 2, 3, 3, 0.05, p(out), p(steps)), (c.h, p(ag), p(g), 2, 3, 3, 0.05, None, p(steps))):
        refused(lib.hp_episode_stats(*args), "hp_episode_stats: null argument")
    refused(lib.hp_episode_stats(c.h, p(ag), p(g), 0, 3, 3, 0.05, p(out), None), r"hp_episode_stats: n_episodes 0 outside \[1, ")
    refused(lib.hp_episode_stats(c.h, p(ag), p(g), 2, 0, 3, 0.05, p(out), None), r"hp_episode_stats: T 0 outside \[1, ")
    refused(lib.hp_episode_stats(c.h, p(ag), p(g), 2, 3, 257, 0.05, p(out), None), r"hp_episode_stats: goal_dim 257 outside \[1, 256\]")
    refused(lib.hp_episode_stats(c.h, p(ag), p(g), 2, 3, 0, 0.05, p(out), None), r"hp_episode_stats: goal_dim 0 outside \[1, 256\]")
    refused(lib.hp_episode_stats_summary(c.h, None, 2, p(summary)), "hp_episode_stats_summary: null argument")
    refused(lib.hp_episode_stats_summary(c.h, p(out), 2, None), "hp_episode_stats_summary: null argument")
    refused(lib.hp_episode_stats_summary(c.h, p(out), 0, p(summary)), "hp_episode_stats_summary: n_episodes 0 is not positive")
    torch.manual_seed(0)
    a = make(NativePointMassVecEnv(2, seed=1, device=DEV, max_timesteps=10), T=10)
    eps = a.collect_episodes_device(n_rollouts=3, explore=False)
    big = torch.zeros((4, 6), dtype=torch.float64, device=DEV)
    refused(lib.hp_episode_stats_block(None, 0, 3, 0.05, p(big), None), "hp_episode_stats_block: null argument")
    refused(lib.hp_episode_stats_block(eps.h, 0, 3, 0.05, None, None), "hp_episode_stats_block: null argument")
    refused(lib.hp_episode_stats_block(eps.h, 0, 4, 0.05, p(big), None), r"hp_episode_stats_block: episodes \[0, 4\) outside the block of 3")
    refused(lib.hp_episode_stats_block(eps.h, 2, 2, 0.05, p(big), None), r"hp_episode_stats_block: episodes \[2, 4\) outside the block of 3")
    refused(lib.hp_episode_stats_block(eps.h, -1, 2, 0.05, p(big), None), r"hp_episode_stats_block: episodes \[-1, 1\) outside the block of 3")
    refused(lib.hp_episode_stats_block(eps.h, 0, 0, 0.05, p(big), None), r"hp_episode_stats_block: episodes \[0, 0\) outside the block of 3")
    with pytest.raises(ValueError, match="outside the block of 3"):
        eps.stats(0.05, first=1, n=3)
    a.ctx.synchronize()
    assert not out.any() and not big.any() and not summary.any()         # a refused call launches nothing
