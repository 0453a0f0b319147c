"""The native pick-and-place environment on the device (PickPlaceEnvDev in csrc/env_device.h, its kernels instantiated in
csrc/env_pick_place.hip and csrc/demo_pick_place.hip, device_env.NativePickPlaceVecEnv) and the pick controller of
hp_demo_episodes_pick: the tensor twin against host twins, the native per-step form against the tensor twin, one launch per wave
against the per-step form on start states with open fingers inside the cube and with held blocks, all waves in one launch with
the reset on the device against the host reset, generated demonstrations against synthetic.scripted_demos, the refusals, and the
training state.  Every comparison is bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import bits
from gpu_common import ctx
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_CRITIC
from rl_arm_under_sparse_reward_amd.device_env import (DeviceEpisodes, NativePickPlaceVecEnv, PickPlaceVecEnv, _NativeEnv, generate_demos,
                                                       script_desc)
from rl_arm_under_sparse_reward_amd.replay_buffer import DeviceEpisodeBuffer
from rl_arm_under_sparse_reward_amd.synthetic import (PICK_FINGER_MAX, PICK_TOOL, DemoScript, PickPlaceGoalEnv, PickScript,
                                                      pick_scripted_action, scripted_demos, scripted_episode)
from rollout_common import (DEV, NAMES, agent_on as any_agent_on, assert_forms, assert_reset_streams_follow_host, assert_rows_equal,
                            assert_same_as_host, assert_states_bit_equal, assert_widened_states, collect_both, dev_ptr as p, twins)

pytestmark = pytest.mark.gpu
T = 12
agent_on = functools.partial(any_agent_on, T=T, env_seed=21)
SHORT = PickScript(phase_end=(1, 4, 6, 9, 10), open=0.5)      # all six phases inside T = 12
SHORT_PUSH = DemoScript(phase_end=(1, 2, 3, 4, 5))
WIDTHS = (3, 3, 3, 8)


# ----------------------------------------------------------------------------- 1., 2. the twins, per step: resets and steps
@pytest.mark.parametrize("cls", [PickPlaceVecEnv, NativePickPlaceVecEnv])
@pytest.mark.parametrize("n_envs", [1, 3, 5])
def test_the_twins_on_the_device_equal_the_host_twins_per_step(n_envs, cls):
    """Two waves: one of scripted actions (grasps and carried blocks), one of random ones; the tensor twin's torch kernels on the
    device -- the native class inherits its step -- against PickPlaceGoalEnv, and the native class's reset on the device
    (hp_env_reset, min_separation = 0.3: several attempts) against the host loop."""
    kw = dict(step_scale=0.6, max_timesteps=T, min_separation=0.3)
    hosts = [PickPlaceGoalEnv(seed=40 + i, **kw) for i in range(n_envs)]
    env = cls(n_envs, seed=40, device=DEV, **kw)
    native = cls is NativePickPlaceVecEnv
    if native:
        streams = env.enable_device_reset(ctx())
    rs, grasped, attempts = np.random.RandomState(1), 0, []
    for wave in range(2):
        ho, vo = [h.reset() for h in hosts], env.reset()
        attempts += [h.reset_attempts for h in hosts]
        if native:
            for i, h in enumerate(hosts):
                assert_states_bit_equal(h.rs.get_state(), streams.get_state(i), ("reset stream", wave, i))
        for t in range(1, T + 1):
            for key in vo:
                assert np.array_equal(bits(vo[key].cpu().numpy()), bits(np.stack([o[key] for o in ho]))), (wave, t, key)
            if wave == 0:
                acts = np.stack([pick_scripted_action(t, o['observation'], o['desired_goal'], SHORT) for o in ho])
            else:
                acts = rs.uniform(-0.7, 0.7, (n_envs, 4))
            acts = acts.astype(np.float32)
            out = [h.step(acts[i]) for i, h in enumerate(hosts)]
            ho = [o[0] for o in out]
            vo, reward, _, info = env.step(torch.from_numpy(acts).to(DEV))
            assert np.array_equal(info['is_success'].cpu().numpy(), np.array([o[3]['is_success'] for o in out], dtype=np.float32))
            assert np.array_equal(reward.cpu().numpy(), np.array([o[1] for o in out], dtype=np.float32))
        assert_rows_equal(env, hosts, n_envs, wave)
        if wave == 0:
            grasped = sum(int(h.held) for h in hosts)
    print("grasped in the scripted wave:", grasped, "of", n_envs, "attempts:", attempts)
    assert grasped >= 1 and max(attempts) > 1


# ------------------------------------------------------------------- 3. one launch per wave against the per-step form
class SeededPickPlaceVecEnv(PickPlaceVecEnv):
    """A reset that puts the environments into the states a random policy almost never reaches: environment i with i % 3 == 0
    has open fingers and the pads inside the cube (it grasps in the first step), i % 3 == 1 holds the block already, i % 3 == 2
    is as the reset left it.  Written through the state arrays, after the draws."""

    def reset(self, n_active=None):
        PickPlaceVecEnv.reset(self, n_active)
        k = self.active
        tool = torch.tensor(PICK_TOOL, dtype=torch.float64, device=self.device)
        rows = torch.arange(k, device=self.device)
        inside, held = rows % 3 == 0, rows % 3 == 1
        on_block = self.blk[:k] - tool
        on_block[:, 2] += 0.1                    # the block 10 cm below the pads' centre: inside a cube of half width 0.15
        seeded = inside | held
        self.grip[:k] = torch.where(seeded[:, None], on_block, self.grip[:k])
        self.aux[:k, 6] = torch.where(inside, torch.full_like(self.aux[:k, 6], PICK_FINGER_MAX), self.aux[:k, 6])
        self.aux[:k, 7] = held.to(torch.float64)
        return self._observation()


class NativeSeededPickPlaceVecEnv(_NativeEnv, SeededPickPlaceVecEnv):
    kind = _lib.ENV_PICK_PLACE


@pytest.mark.parametrize("explore", [False, True])
@pytest.mark.parametrize("n_envs,n_rollouts", [(1, 1), (3, 3), (5, 5), (5, 8)])
def test_fused_wave_equals_the_per_step_path_on_seeded_grasps(n_envs, n_rollouts, explore):
    """Two agents built identically, one on the tensor twin (two launches and the twin's kernels per timestep), one on the native
    environment (one launch per wave: hp_rollout_episodes), both reset on the host into seeded states.  step_scale = 0.01 keeps
    the pads inside the cube (half width 0.15), so environment 0 grasps in the first step and carries, environment 1 carries
    from the start, environment 2 never grasps; finger_scale = 0.1 lets the fourth action component show in the observation."""
    env_kw = dict(step_scale=0.01, half_width=0.15, finger_scale=0.1)
    plain, native = (agent_on(cls, n_envs, env_kw=env_kw, random_eps=0.3) for cls in (SeededPickPlaceVecEnv, NativeSeededPickPlaceVecEnv))
    before = native.explore_streams.get_states()
    (obs, ag, g, actions), flags = collect_both(plain, native, n_rollouts=n_rollouts, explore=explore)
    assert_forms(plain, native, "stepped", "fused")
    assert native.rollout_launches == -(-n_rollouts // n_envs)
    assert np.array_equal(ag, obs[:, :, 12:15]) and np.array_equal(obs[:, :, 18:21], obs[:, :, 12:15] - obs[:, :, 0:3])
    assert not obs[:, :, 3:6].any() and not obs[:, :, 11].any() and not obs[:, :, 15:18].any() and not obs[:, :, 24:27].any()
    moved = [not np.array_equal(x[1], y[1]) or x[2] != y[2] for x, y in zip(before, native.explore_streams.get_states())]
    assert moved == [explore and i < n_rollouts for i in range(n_envs)]
    held, finger, bvel, gvel = obs[:, :, 10], obs[:, :, 9], obs[:, 1:, 21:24], obs[:, 1:, 6:9]
    for e in range(n_rollouts):
        i = e % n_envs
        if i % 3 == 0:       # open fingers inside the cube: locked and grasped in the first step, carried from the second
            assert held[e, 0] == 0.0 and finger[e, 0] == PICK_FINGER_MAX and np.all(held[e, 1:] == 1.0) and finger[e, 1] == 0.0
            assert not bvel[e, 0].any() and np.allclose(bvel[e, 1:, :2], gvel[e, 1:, :2], rtol=0, atol=1e-15) and gvel[e, 1:].any()
        elif i % 3 == 1:     # held from the start: the block follows (z is clipped at the table), the fingers stay shut
            assert np.all(held[e] == 1.0) and not finger[e].any() and np.allclose(bvel[e, :, :2], gvel[e, :, :2], rtol=0, atol=1e-15)
            assert gvel[e].any()
    if explore:
        assert np.abs(actions).max() <= 0.5 and len({a.tobytes() for a in actions}) == n_rollouts


# ------------------------------------------------------------------- 4. all waves in one launch, the reset on the device
@pytest.mark.parametrize("min_separation,env_seed", [(0.3, 21), (0.5, 21)])
def test_all_waves_in_one_launch_equal_one_launch_per_wave(min_separation, env_seed):
    """Seven episodes on three environments, a partial last wave, exploring with streams: hp_rollout_waves with the rejection
    loop on the device against one launch per wave behind the host reset.  min_separation = 0.3: resets of several attempts;
    0.5: the loop runs out (100 attempts of ten words: every reset stream crosses its block more than once)."""
    env_kw = dict(min_separation=min_separation)
    A, B = (agent_on(NativePickPlaceVecEnv, 3, reset=reset, env_seed=env_seed, env_kw=env_kw, random_eps=0.3) for reset in (False, True))
    spent = []
    for n_rollouts in (7, 4):                                        # the second call continues every stream
        A.vec_env.reset_attempts = [0] * 3
        got, flags = collect_both(A, B, n_rollouts=n_rollouts)
        assert A.rollout_form == B.rollout_form == "fused" and B.rollout_launches == 1 and A.rollout_launches == -(-n_rollouts // 3)
        assert B.vec_env.active == (n_rollouts - 1) % 3 + 1
        assert_widened_states(B.vec_env, WIDTHS)
        assert_reset_streams_follow_host(A, B)
        spent += A.vec_env.reset_attempts
    print("attempts of the last reset of each environment:", spent)
    if min_separation == 0.5:
        assert spent == [100] * 6                                    # (on the host: every reset of seeds 21 .. 23 runs out)
    else:
        assert 1 < max(spent) < 100


# ------------------------------------------------------------------------------------------- 5. generated demonstrations
@pytest.mark.parametrize("n_envs,launch_cap,launches", [(1, None, 1), (5, None, 1), (5, T, 2)])
def test_pick_demos_equal_the_host_generator(n_envs, launch_cap, launches):
    """The short schedule at step_scale 0.6, T = 12, seeds from 0: rounds of two waves until four episodes are kept -- some are
    kept and some rejected on the way (the host says which) -- with the environment's own default script type; a launch cap of
    T timesteps makes two launches of every round."""
    hosts, env = twins("pick", n_envs, 0, T, step_scale=0.6, min_separation=0.3)
    assert isinstance(env.default_demo_script(), PickScript)
    want = scripted_demos(hosts, 4, 2, max_episodes=40, script=SHORT)
    demos = generate_demos(env, 4, round_waves=2, max_episodes=40, script=SHORT, launch_cap=launch_cap)
    assert_same_as_host(hosts, env, demos, want)
    rounds = want[5] // (2 * n_envs)
    print(f"{demos.kept} kept of {demos.attempted} attempted in {rounds} rounds, {demos.launches} launches")
    assert demos.kept == 4 and demos.attempted > 4 and demos.attempted == rounds * 2 * n_envs and demos.launches == rounds * launches
    obs, actions = demos.numpy()[0], demos.numpy()[3]
    assert np.all(obs[:, -1, 10] == 1.0) and np.all(actions[:, 5, 3] == 0.5) and np.all(actions[:, 9, 3] == -0.5)
    assert np.array_equal(actions[:, 0], np.tile(SHORT.lift, (4, 1)))


def test_the_default_script_of_the_environment_is_the_pick_schedule():
    """script=None on the new kind runs PickScript() (at T = 12: lift, then approach; nothing is kept), on the push block the
    push schedule as before"""
    hosts, env = twins("pick", 3, 5, T)
    want = scripted_demos(hosts, 2, 1, max_episodes=3, script=PickScript())
    demos = generate_demos(env, 2, round_waves=1, max_episodes=3)
    assert demos.kept == 0 and demos.attempted == 3 and demos.launches == 1
    assert_same_as_host(hosts, env, demos, want)
    hosts, env = twins("push", 3, 5, T)
    want = scripted_demos(hosts, 2, 1, max_episodes=3)
    demos = generate_demos(env, 2, round_waves=1, max_episodes=3)
    assert_same_as_host(hosts, env, demos, want)


@pytest.mark.parametrize("kind,script,kw", [("pick", SHORT_PUSH, dict(step_scale=0.6)),
                                            ("push", SHORT, dict(half_width=0.15, z_touch=0.6, step_scale=0.3))])
def test_either_controller_runs_on_either_kind(kind, script, kw):
    """The push schedule on the pick-and-place kind and the pick schedule on the push block, through the entry that matches the
    script's type: bit for bit the host's.  Kept or not, every attempted episode is compared: n_demos is out of reach."""
    hosts, env = twins(kind, 5, 21, T, **kw)
    c, n = ctx(), 8
    shape = DeviceEpisodeBuffer(1, T, 27, 3, 4, ctx=c)
    block = DeviceEpisodes(c, shape, n)
    success = torch.zeros(n, dtype=torch.float32, device=DEV)
    steps = torch.zeros((n, T), dtype=torch.float32, device=DEV)
    launches = C.c_int32()
    entry = c.lib.hp_demo_episodes_pick if isinstance(script, PickScript) else c.lib.hp_demo_episodes
    d = env.env_desc()
    with c.torch_bridge():
        _lib.check(entry(c.h, C.byref(d), env.reset_streams.h, C.byref(script_desc(script)), 5, 0, n, T, block.h, p(success), p(steps),
                         C.byref(launches)))
    assert launches.value == 1
    want = [scripted_episode(hosts[e % 5], script) for e in range(n)]
    for j, x in enumerate(block.numpy()):
        assert np.array_equal(bits(x), bits(np.array([w[j] for w in want]))), NAMES[j]
    assert np.array_equal(steps.cpu().numpy(), np.array([w[4] for w in want], dtype=np.float32))
    assert np.array_equal(success.cpu().numpy(), np.array([w[4][-1] for w in want], dtype=np.float32))
    states = env.reset_streams.get_states()
    for i, h in enumerate(hosts):
        assert_states_bit_equal(h.rs.get_state(), states[i], ("reset stream", i))
    assert_rows_equal(env, hosts, 5, "final state")


# -------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_carry_the_entrys_own_name():
    c, n = ctx(), 4
    lib = c.lib
    _, env = twins("pick", n, 21, T)
    shape = DeviceEpisodeBuffer(1, T, 27, 3, 4, ctx=c)
    block = DeviceEpisodes(c, shape, 8)
    success = torch.zeros(8, dtype=torch.float32, device=DEV)
    steps = torch.zeros((8, T), dtype=torch.float32, device=DEV)
    state = [getattr(env, name).clone() for name in env.state_names]
    streams = env.reset_streams.get_states()

    def desc(kind=None, null=None):
        d = env.env_desc()
        if kind is not None:
            d.kind = kind
        if null is not None:
            d.state_dev[null] = None
        return d

    def episodes(d=None, script=None, steps_T=T, streams_h=None):
        d = d or desc()
        sd = script if script is not None else script_desc(SHORT)
        with c.torch_bridge():
            _lib.check(lib.hp_demo_episodes_pick(c.h, C.byref(d), env.reset_streams.h if streams_h is None else streams_h, C.byref(sd), n, 0,
                                                 8, steps_T, block.h, p(success), p(steps), None))

    with pytest.raises(ValueError, match=r"hp_demo_episodes_pick: env->kind 7 is not an environment kind"):
        episodes(desc(kind=7))
    with pytest.raises(ValueError, match=r"hp_demo_episodes_pick: env->state_dev\[3\] is null"):
        episodes(desc(null=3))
    bad = script_desc(SHORT)
    bad.phase_end[2] = bad.phase_end[1]
    with pytest.raises(ValueError, match=r"hp_demo_episodes_pick: script->phase_end\[2\] = 4: the phase ends must be increasing"):
        episodes(script=bad)
    with pytest.raises(ValueError, match=r"hp_demo_episodes_pick: T = 11, the block has T = 12"):
        episodes(steps_T=11)
    with pytest.raises(ValueError, match=r"hp_demo_episodes_pick: null argument"):
        with c.torch_bridge():
            _lib.check(lib.hp_demo_episodes_pick(c.h, C.byref(desc()), None, C.byref(bad), n, 0, 8, T, block.h, p(success), p(steps), None))
    with pytest.raises(ValueError, match="must be increasing"):
        generate_demos(env, 1, script=PickScript(phase_end=(3, 2, 4, 5, 6)))
    # nothing ran: states and streams are what they were
    for name, before in zip(env.state_names, state):
        assert torch.equal(getattr(env, name), before), name
    for i, (x, y) in enumerate(zip(streams, env.reset_streams.get_states())):
        assert_states_bit_equal(x, y, i)
    episodes()                                                       # ... and a good call does
    assert not torch.equal(env.grip, state[0])


# ----------------------------------------------------------------------------------------------------- 7. the training state
def test_a_state_saved_mid_run_with_held_blocks_resumes_bit_for_bit(tmp_path):
    """Parameters under which a random policy grasps: a cube of half width 0.2, fingers that open in one step, every action
    uniform (random_eps = 1); with environments from seed 28 and exploration streams from 900 the host twin says environments 0
    and 1 end both of their episodes with the block in hand.  The state is saved after that cycle; the resumed run's next cycle
    is the original's."""
    n, kw = 3, dict(T=T, n_batches=3, buffer_episodes=20, seed=12, random_eps=1.0, env_seed=28)
    env_kw = dict(half_width=0.2, finger_scale=1.0, step_scale=0.5, min_separation=0.3)
    B = agent_on(NativePickPlaceVecEnv, n, reset=True, env_kw=env_kw, **kw)
    first = B.collect_episodes_device(n_rollouts=6)
    held = first.numpy()[0][:, -1, 10]
    print("held at the end of the six episodes:", held, "final aux:", B.vec_env.aux[:, 6:].cpu().numpy().tolist())
    assert held.any() and B.vec_env.aux[:, 7].any()                  # blocks in hand when the state is saved
    B.train_cycle(first)
    assert B.rollout_form == "fused" and B.rollout_launches == 1
    path = B.save_training_state(tmp_path / "mid.npz")
    flags_b, flags_r = [], []
    want = [x.copy() for x in B.collect_episodes_device(n_rollouts=5, success_out=flags_b).numpy()]
    B.train_cycle(B._rollouts[5])

    R = agent_on(NativePickPlaceVecEnv, n, reset=True, base=1, env_kw=env_kw, **dict(kw, env_seed=77))
    R.load_training_state(path)
    got = R.collect_episodes_device(n_rollouts=5, success_out=flags_r)
    for x, y in zip(got.numpy(), want):
        assert np.array_equal(bits(x), bits(y))
    assert torch.equal(flags_b[0], flags_r[0])
    R.train_cycle(got)
    for slot in (NET_ACTOR, NET_CRITIC):
        assert np.array_equal(bits(B._get_flat(slot)), bits(R._get_flat(slot))), slot
    for fam in ("reset_streams", "explore_streams"):
        x, y = (getattr(a.vec_env, fam) if fam == "reset_streams" else a.explore_streams for a in (R, B))
        for u, v in zip(x.get_arrays(), y.get_arrays()):
            assert np.array_equal(bits(u), bits(v)), fam
    for name in B.vec_env.state_names:
        assert np.array_equal(bits(getattr(B.vec_env, name).cpu().numpy()), bits(getattr(R.vec_env, name).cpu().numpy())), name
