"""Scripted demonstrations generated on the device (device_env.generate_demos: k_demo_episodes of csrc/demo_episodes.h through
hp_demo_episodes, k_demo_compact through hp_demo_compact) against synthetic.scripted_demos on host twins seeded alike.  Every
comparison is bit for bit: kept episodes, per-step flags, counts, the environments' final state and the reset streams."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import bits
from gpu_common import ctx, fresh_rng
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_CRITIC, ddpg_agent
from rl_arm_under_sparse_reward_amd.device_env import (DeviceEpisodes, NativePushBlockVecEnv, PushBlockVecEnv, default_round_waves,
                                                       generate_demos, script_desc)
from rl_arm_under_sparse_reward_amd.random import DeviceRandomState
from rl_arm_under_sparse_reward_amd.replay_buffer import DeviceEpisodeBuffer
from rl_arm_under_sparse_reward_amd.synthetic import DemoScript, PushBlockGoalEnv, make_episodes, scripted_demos
from rollout_common import DEV, assert_same_as_host, assert_states_bit_equal, dev_ptr as p, make, primed, twins

pytestmark = pytest.mark.gpu
# a schedule that visits all six phases inside T = 20 and then pushes; with step_scale 0.5 the point mass halves its distance
# to the goal in every push step, so every episode succeeds (checked on the host: 20 of 20 for 1, 3 and 5 environments)
SHORT = DemoScript(phase_end=(1, 2, 3, 4, 5))


# ------------------------------------------------------------------------------------------------ 1. point mass, every episode kept
@pytest.mark.parametrize("n_envs", [1, 3, 5])
def test_point_mass_demos_equal_the_host_generator(n_envs):
    hosts, env = twins("point", n_envs, 7, 20, step_scale=0.5)
    want = scripted_demos(hosts, 7, 2, script=SHORT)
    demos = generate_demos(env, 7, round_waves=2, script=SHORT)
    assert_same_as_host(hosts, env, demos, want)
    rounds = -(-7 // (2 * n_envs))
    assert demos.kept == 7 and demos.attempted == rounds * 2 * n_envs and demos.launches == rounds
    assert env.active == n_envs
    # the stop rule and every phase were taken on the way: zero actions at the end, the constant lift at the start
    actions = demos.numpy()[3]
    assert not actions[:, -1].any() and np.array_equal(actions[:, 0], np.tile(SHORT.lift, (7, 1)))


# ----------------------------------------------------------------------------------- 2. push block, the reference's schedule, T = 100
# (n_envs, n_demos, round_waves, environment seed, max_episodes): on the host the successes are attempts
#   (1, 2, 8) seed 0: 5, 38       -> five rounds of 8, the last cut to 6 by max_episodes = 38, rounds two to four without a success
#   (3, 4, 4) seed 40: 19, 28, 41, 44 -> four rounds of 12, the last cut to 8 by max_episodes = 44, round one without a success
#   (5, 3, 1) seed 0: 13, 21, 37  -> eight rounds of 5, the last cut to 2 (environments 2 .. 4 sit it out), five without a success
PUSH_CASES = [(1, 2, 8, 0, 38), (3, 4, 4, 40, 44), (5, 3, 1, 0, 37)]


@pytest.mark.parametrize("n_envs,n_demos,round_waves,seed,max_episodes", PUSH_CASES)
def test_push_block_demos_equal_the_host_generator(n_envs, n_demos, round_waves, seed, max_episodes):
    hosts, env = twins("push", n_envs, seed, 100)
    want = scripted_demos(hosts, n_demos, round_waves, max_episodes=max_episodes)
    assert want[0].shape[0] == n_demos and want[5] == max_episodes          # reached, in a last round that max_episodes cut
    demos = generate_demos(env, n_demos, round_waves=round_waves, max_episodes=max_episodes)
    assert_same_as_host(hosts, env, demos, want)
    per = n_envs * round_waves
    assert demos.kept == n_demos and demos.launches == -(-max_episodes // per) and max_episodes % per != 0
    assert env.active == (max_episodes % per - 1) % n_envs + 1


# ---------------------------------------------------------------------------------------------- 3. max_episodes runs out
def test_max_episodes_exhausted_is_reported_and_the_agent_path_raises():
    hosts, env = twins("push", 3, 40, 100)
    want = scripted_demos(hosts, 4, 4, max_episodes=30)                     # successes at 19 and 28 only
    demos = generate_demos(env, 4, round_waves=4, max_episodes=30)
    assert demos.kept == 2 < 4 and demos.attempted == 30 and demos.launches == 3
    assert_same_as_host(hosts, env, demos, want)
    hosts, env = twins("push", 3, 40, 100)
    none = generate_demos(env, 4, round_waves=4, max_episodes=12)           # no success in the first round
    assert_same_as_host(hosts, env, none, scripted_demos(hosts, 4, 4, max_episodes=12))
    assert none.kept == 0 and none.numpy()[0].shape == (0, 101, 27)
    torch.manual_seed(0)
    _, env = twins("push", 3, 40, 100)
    with pytest.raises(RuntimeError, match=r"demo_source='device': only 2 of 4 scripted episodes succeeded in 30 attempts"):
        make(env, T=100, add_demo=True, demo_source="device", demo_episodes=4, demo_max_episodes=30)


# ------------------------------------------------------------------ 4. a reset stream leaves its 624-word block inside a launch
def test_a_reset_stream_crosses_its_block_inside_a_rejection_loop():
    """One environment, 40 waves of T = 20 in one launch.  The stream is advanced by 418 words first: the reset of wave 14 then
    starts at position 602 and takes four attempts of eight words, so the block ends inside its third attempt."""
    hosts, env = twins("push", 1, 21, 20)
    start = DeviceRandomState(21, ctx=ctx())
    start.advance(418)
    state = start.get_state()
    hosts[0].rs.bytes(4 * 418)
    assert_states_bit_equal(hosts[0].rs.get_state(), state, "advance")
    env.reset_streams.set_states([state])
    probe, crossed = PushBlockGoalEnv(seed=21, max_timesteps=20), []
    probe.rs.set_state(state)
    for k in range(40):
        before = probe.rs.get_state()[2]
        probe.reset()
        if probe.rs.get_state()[2] < before:
            crossed.append((k, before, probe.rs.get_state()[2], probe.reset_attempts))
    assert crossed == [(14, 602, 10, 4)]
    want = scripted_demos(hosts, 40, 40, max_episodes=40, script=SHORT)
    demos = generate_demos(env, 40, round_waves=40, max_episodes=40, script=SHORT)
    assert demos.launches == 1 and demos.attempted == 40
    assert_same_as_host(hosts, env, demos, want)
    assert not np.array_equal(env.reset_streams.get_state(0)[1], state[1])          # the key was rewritten


# ---------------------------------------------------------------------------------------------------------- 5. the launch cap
@pytest.mark.parametrize("cap,launches", [(40, 2), (1, 3), (0, 1)])
def test_a_round_split_by_the_launch_cap_gives_the_same_bits(cap, launches):
    """T = 20, a round of three waves on three environments, the last wave partial (max_episodes = 8): a cap of 40 timesteps
    holds two waves, a cap below T one, and 0 is the default cap."""
    hosts, env = twins("push", 3, 21, 20, half_width=0.15, z_touch=0.6, step_scale=0.3)
    want = scripted_demos(hosts, 8, 3, max_episodes=8, script=SHORT)
    demos = generate_demos(env, 8, round_waves=3, max_episodes=8, script=SHORT, launch_cap=cap)
    assert demos.launches == launches and demos.attempted == 8
    assert_same_as_host(hosts, env, demos, want)
    assert env.active == 2


# ------------------------------------------------------------------------------------------------------ 6. the agent's preload
def test_the_agent_preloads_generated_demos_like_host_arrays():
    n_envs, n_demos, T = 5, 3, 100
    agents = []
    for source in ("device", "host"):
        torch.manual_seed(0)
        hosts, env = twins("push", n_envs, 0, T)
        if source == "device":
            a = make(env, T=T, buffer_episodes=20, n_batches=2, add_demo=True, demo_source="device", demo_episodes=n_demos)
            assert a.demo_stats["kept"] == n_demos
        else:
            a = make(env, T=T, buffer_episodes=20, n_batches=2)
            *arrays, attempted = scripted_demos(hosts, n_demos, default_round_waves(n_demos, n_envs))
            a.buffer.store_episode(arrays[:4])
            assert arrays[0].shape[0] == n_demos and attempted == agents[0].demo_stats["attempted"]
        primed(a)
        agents.append(a)
    A, B = agents
    assert A.buffer.current_size == B.buffer.current_size == n_demos
    assert A.buffer.n_transitions_stored == B.buffer.n_transitions_stored == n_demos * T
    for key in ("obs", "ag", "g", "actions"):
        assert np.array_equal(bits(A.buffer._dev.read(key, 0, n_demos)), bits(B.buffer._dev.read(key, 0, n_demos))), key
    assert_states_bit_equal(A.rng.get_state(), B.rng.get_state(), "sampler stream")
    eps = make_episodes(2, seed=5, T=T, mode="walk")
    for a in agents:
        a.train_cycle(eps)
    for slot in (NET_ACTOR, NET_CRITIC):
        assert np.array_equal(bits(A._get_flat(slot)), bits(B._get_flat(slot))), slot


def test_learn_enables_the_device_reset_before_the_preload():
    """args.device_reset with an environment that is not reset on the device yet: the preload waits for learn()"""
    torch.manual_seed(0)
    env = NativePushBlockVecEnv(5, seed=0, device=DEV, max_timesteps=100)
    a = make(env, T=100, buffer_episodes=20, add_demo=True, demo_source="device", demo_episodes=3, device_reset=True, n_epochs=0)
    assert a.buffer.current_size == 0 and a._demo_preload_pending and env.reset_streams is None
    a.learn()
    assert a.buffer.current_size == 3 and env.reset_streams is not None and not a._demo_preload_pending


# ---------------------------------------------------------------------------------------------------------- 7. what stays put
def test_generation_leaves_the_other_streams_alone():
    torch.manual_seed(0)
    _, env = twins("point", 3, 7, 20, step_scale=0.5)
    a = make(env, T=20)
    a.enable_explore_streams(base_seed=900)
    learner, explore = a.rng.get_state(), a.explore_streams.get_states()
    demos = generate_demos(env, 7, round_waves=2, script=SHORT, ctx=a.ctx)
    assert demos.kept == 7
    assert_states_bit_equal(a.rng.get_state(), learner, "agent.rng")
    for i, (x, y) in enumerate(zip(explore, a.explore_streams.get_states())):
        assert_states_bit_equal(x, y, ("exploration stream", i))
    # a demo file out of the block preloads through the file path
    a.buffer.store_episode(demos.episodes)
    assert a.buffer.current_size == 7


# -------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_carry_the_librarys_message(tmp_path):
    c, n, T = ctx(), 4, 20
    lib = c.lib
    _, env = twins("push", n, 21, T)
    shape = DeviceEpisodeBuffer(1, T, 27, 3, 4, ctx=c)
    block, dst = DeviceEpisodes(c, shape, 8), DeviceEpisodes(c, shape, 3)
    success = torch.zeros(8, dtype=torch.float32, device=DEV)
    steps = torch.zeros((8, T), dtype=torch.float32, device=DEV)
    info = torch.zeros((3, T), dtype=torch.float32, device=DEV)
    kept = torch.zeros(1, dtype=torch.int32, device=DEV)
    state = [getattr(env, name).clone() for name in env.state_names]
    streams = env.reset_streams.get_states()

    def desc(kind=None, null=None):
        d = env.env_desc()
        if kind is not None:
            d.kind = kind
        if null is not None:
            d.state_dev[null] = None
        return d

    def episodes(d=None, script=None, n_envs=n, first=0, count=8, steps_T=T, blk=None):
        d = d or desc()
        with c.torch_bridge():
            _lib.check(lib.hp_demo_episodes(c.h, C.byref(d), env.reset_streams.h, C.byref(script_desc(script)), n_envs, first, count,
                                            steps_T, (blk or block).h, p(success), p(steps), None))

    def compact(src=None, count=8, to=None, n_demos=3, before=0):
        with c.torch_bridge():
            _lib.check(lib.hp_demo_compact(c.h, (src or block).h, p(success), p(steps), count, (to or dst).h, p(info), n_demos, before,
                                           p(kept)))

    with pytest.raises(ValueError, match=r"hp_demo_episodes: env->kind 7 is not an environment kind"):
        episodes(desc(kind=7))
    with pytest.raises(ValueError, match=r"hp_demo_episodes: env->state_dev\[3\] is null"):
        episodes(desc(null=3))
    with pytest.raises(ValueError, match=r"hp_demo_episodes: 5 environments, but the array holds 4 reset streams"):
        episodes(n_envs=5)
    with pytest.raises(ValueError, match=r"hp_demo_episodes: episodes \[4, 12\) outside the block of 8"):
        episodes(first=4)
    with pytest.raises(ValueError, match=r"hp_demo_episodes: T = 19, the block has T = 20"):
        episodes(steps_T=19)
    other = DeviceEpisodes(c, DeviceEpisodeBuffer(1, T, 10, 2, 3, ctx=c), 8)
    with pytest.raises(ValueError, match=r"hp_demo_episodes: env->kind 2 has dimensions 27 / 3 / 4, the block has 10 / 2 / 3"):
        episodes(blk=other)
    bad = script_desc()
    bad.phase_end[2] = bad.phase_end[1]
    with pytest.raises(ValueError, match=r"hp_demo_episodes: script->phase_end\[2\] = 20: the phase ends must be increasing"):
        with c.torch_bridge():
            _lib.check(lib.hp_demo_episodes(c.h, C.byref(desc()), env.reset_streams.h, C.byref(bad), n, 0, 8, T, block.h, p(success),
                                            p(steps), None))
    with pytest.raises(ValueError, match=r"hp_demo_episodes: null argument"):
        with c.torch_bridge():
            _lib.check(lib.hp_demo_episodes(c.h, C.byref(desc()), None, C.byref(bad), n, 0, 8, T, block.h, p(success), p(steps), None))
    with pytest.raises(ValueError, match=r"hp_demo_compact: the source block has T 20 and dimensions 10 / 2 / 3, the destination 20 and 27 / 3 / 4"):
        compact(src=other)
    with pytest.raises(ValueError, match=r"hp_demo_compact: episodes \[0, 9\) outside the source block of 8"):
        compact(count=9)
    with pytest.raises(ValueError, match=r"hp_demo_compact: episodes \[0, 4\) outside the destination block of 3"):
        compact(n_demos=4)
    with pytest.raises(ValueError, match=r"hp_demo_compact: kept = 4 outside \[0, 3\]"):
        compact(before=4)
    with pytest.raises(ValueError, match=r"hp_demo_compact: source and destination are the same block"):
        compact(to=block)
    # the Python call's own
    with pytest.raises(ValueError, match="generate_demos: the environment is not native"):
        generate_demos(PushBlockVecEnv(2, device=DEV), 1)
    with pytest.raises(ValueError, match="generate_demos: the environment is not reset on the device"):
        generate_demos(NativePushBlockVecEnv(2, device=DEV), 1)
    with pytest.raises(ValueError, match="must be increasing"):
        generate_demos(env, 1, script=DemoScript(phase_end=(3, 2, 4, 5, 6)))
    # nothing ran: states and streams are what they were
    for name, before in zip(env.state_names, state):
        assert torch.equal(getattr(env, name), before), name
    for i, (x, y) in enumerate(zip(streams, env.reset_streams.get_states())):
        assert_states_bit_equal(x, y, i)
    # ... and good calls do; a saved file reads back as the arrays
    episodes(script=SHORT)
    compact()
    assert not torch.equal(env.grip, state[0]) and 0 <= int(kept.item()) <= 3
    _, pm = twins("point", 2, 7, 20, step_scale=0.5)
    demos = generate_demos(pm, 3, round_waves=2, script=SHORT)
    path = str(tmp_path / "bmirobot_3_push_demo.npz")
    demos.save(path)
    back = np.load(path, allow_pickle=True)
    for key, a in zip(("obs", "ag", "g", "acs"), demos.numpy()):
        assert np.array_equal(bits(back[key]), bits(a)), key
    assert back["info"].shape == (3, 20) and back["info"][2, 19] == {"is_success": np.float32(1.0)}
