"""Whole episodes in one launch (hp_rollout_episodes, k_rollout_episodes in csrc/rollout.hip, csrc/env_device.h,
device_env.NativePointMassVecEnv): every comparison is bit for bit against the per-step path of the same build -- two agents built
identically, one on PointMassVecEnv (two launches and a dozen torch kernels per timestep), one on the native environment (one
launch per wave) -- plus the closed loop against host workers, a training cycle on top, the fallbacks, the refusals and the
training state."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import bits
from gpu_common import ctx, fresh_rng, host_select_actions
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_CRITIC, ddpg_agent
from rl_arm_under_sparse_reward_amd.device_env import DeviceEpisodes, NativePointMassVecEnv, PointMassVecEnv, binomial1_qn
from rl_arm_under_sparse_reward_amd.random import DeviceRandomStreams
from rl_arm_under_sparse_reward_amd.replay_buffer import DeviceEpisodeBuffer
from rl_arm_under_sparse_reward_amd.synthetic import PointMassGoalEnv
from rollout_common import (DEV, agent_pair, assert_forms, assert_states_bit_equal, assert_wave_flags_equal, assert_whole_states_equal,
                            collect_both, dev_ptr as p, make, primed)

pytestmark = pytest.mark.gpu
# (agent on PointMassVecEnv, agent on NativePointMassVecEnv), built identically
pair = functools.partial(agent_pair, (PointMassVecEnv, NativePointMassVecEnv), env_seed=10)


def assert_waves_equal(plain, native, form, **kw):
    """collect_both, the forms, and what holds because both are reset on the host: per-wave flags, whole state tensors"""
    got, flags = collect_both(plain, native, **kw)
    assert_forms(plain, native, "stepped", form)
    assert_wave_flags_equal(flags)
    assert_whole_states_equal(plain, native)
    return got


# ------------------------------------------------------------------------------------- 1. exploring, per-environment streams
@pytest.mark.parametrize("epoch", [0, 100])
@pytest.mark.parametrize("n_envs,n_rollouts", [(1, None), (3, None), (4, None), (5, None), (9, None), (4, 7)])
def test_exploring_wave_equals_the_per_step_path(n_envs, n_rollouts, epoch):
    """Full and partial 4-row slabs; 50 steps of about 20 words cross a 624-word block in every stream, so the key is committed.
    Seven episodes on four environments: the second wave is partial and must leave stream 3 where the first wave left it."""
    T = 50
    plain, native = pair(n_envs, T)
    fresh = native.explore_streams.get_states()
    _, _, _, actions = assert_waves_equal(plain, native, "fused", n_rollouts=n_rollouts, epoch=epoch)
    after = native.explore_streams.get_states()
    assert all(not np.array_equal(a[1], b[1]) for a, b in zip(fresh, after))            # every key was rewritten
    assert np.abs(actions).max() <= (float(np.float32(0.15)) if epoch >= 100 else 0.5)     # the exploring clip is a float32 clip
    if n_rollouts:
        once = pair(n_envs, T)[1]
        once.collect_episodes_device(n_rollouts=n_envs, epoch=epoch)
        assert_states_bit_equal(once.explore_streams.get_state(3), after[3], "stream 3 after one wave")
        assert not np.array_equal(once.explore_streams.get_state(2)[1], after[2][1])


# ------------------------------------------------------------------------------------------------------------ 2. noise-free
@pytest.mark.parametrize("streams", [True, False])
@pytest.mark.parametrize("epoch", [0, 100])
def test_noise_free_wave_equals_the_per_step_path(streams, epoch):
    plain, native = pair(5, 20, streams=streams)
    before = native.explore_streams.get_states() if streams else None
    assert_waves_equal(plain, native, "fused", explore=False, epoch=epoch)
    if streams:
        for i, (x, y) in enumerate(zip(before, native.explore_streams.get_states())):
            assert_states_bit_equal(x, y, i)


@pytest.mark.parametrize("n_test", [3, 10])
def test_evaluation_returns_the_same_rate(n_test):
    plain, native = pair(4, 20, n_test_rollouts=n_test)
    rates = [a._eval_agent() for a in (plain, native)]
    assert native.rollout_form == "fused" and plain.rollout_form == "stepped"
    assert isinstance(rates[1], float) and rates[0] == rates[1], rates


# ----------------------------------------------------------------------------------------- 3. closed loop against host workers
def test_closed_loop_equals_one_host_worker_per_env():
    """test_gpu_explore_streams.test_closed_loop_equals_one_host_worker_per_env on the native environment: env i =
    PointMassGoalEnv(seed + i), its own RandomState(base + i), `agent.act` on its row and the host `_select_actions`.  Tolerance
    of a first cycle (2e-6: the policy's float32 outputs feed back through the environment); stream keys and positions exact."""
    n, n_rollouts, T, env_seed, base = 4, 7, 50, 10, 900
    torch.manual_seed(0)
    agent = make(NativePointMassVecEnv(n, seed=env_seed, device=DEV, max_timesteps=T), T=T, noise_eps=0.05)
    primed(agent)
    streams = agent.enable_explore_streams(base_seed=base)
    learner_before = agent.rng.get_state()
    got = agent.collect_episodes_device(n_rollouts=n_rollouts, explore=True).numpy()
    assert agent.rollout_form == "fused"
    assert_states_bit_equal(agent.rng.get_state(), learner_before, "learner stream")
    amax = agent.env_params["action_max"]
    envs = [PointMassGoalEnv(seed=env_seed + i, max_timesteps=T) for i in range(n)]
    host = [np.random.RandomState(base + i) for i in range(n)]
    want = [[], [], [], []]
    for first in (0, n):
        for i in range(min(n, n_rollouts - first)):
            o = envs[i].reset()
            ep = ([], [], [], [])
            for _ in range(T):
                pi = agent.act(o["observation"], o["desired_goal"])
                action = host_select_actions(host[i], pi, agent.args.noise_eps, agent.args.random_eps, amax, False)
                for dst, v in zip(ep, (o["observation"], o["achieved_goal"], o["desired_goal"], action)):
                    dst.append(np.array(v, dtype=np.float64))
                o = envs[i].step(action)[0]
            ep[0].append(np.array(o["observation"])); ep[1].append(np.array(o["achieved_goal"]))
            for dst, src in zip(want, ep):
                dst.append(np.array(src))
    for nm, a, b in zip(("obs", "ag", "g", "actions"), got, want):
        b = np.array(b)
        worst = float(np.abs(a - b).max())
        print(f"closed loop (fused) {nm}: worst absolute difference {worst:.3e}")
        assert a.shape == b.shape and worst <= 2e-6, (nm, worst)
    for i in range(n):
        sd, sn = streams.get_state(i), host[i].get_state()
        assert np.array_equal(sd[1], sn[1]) and sd[2] == sn[2] and sd[3] == sn[3], i


# ------------------------------------------------------------------------------------------------ 4. a training cycle on top
def test_training_cycles_on_fused_waves_leave_the_same_learner():
    T = 20
    plain, native = pair(3, T, n_batches=3, buffer_episodes=10)
    for _ in range(2):
        for a in (plain, native):
            a.train_cycle(a.collect_episodes_device(n_rollouts=2, epoch=0))
    assert plain.rollout_form == "stepped" and native.rollout_form == "fused"
    for slot in (NET_ACTOR, NET_CRITIC):
        assert np.array_equal(bits(plain._get_flat(slot)), bits(native._get_flat(slot))), slot
    stored = plain.buffer.current_size
    assert stored == native.buffer.current_size == 4
    for key in ("obs", "ag", "g", "actions"):
        assert np.array_equal(bits(plain.buffer._dev.read(key, 0, stored)), bits(native.buffer._dev.read(key, 0, stored))), key
    for na, nb in ((plain.o_norm, native.o_norm), (plain.g_norm, native.g_norm)):
        x, y = na._get(), nb._get()
        for key in x:
            assert np.array_equal(bits(x[key]), bits(y[key])), key
    sa, sb = plain.rng.get_state(), native.rng.get_state()
    assert np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    for i, (x, y) in enumerate(zip(plain.explore_streams.get_states(), native.explore_streams.get_states())):
        assert_states_bit_equal(x, y, i)


# ------------------------------------------------------------------------------------------------ 5. fallbacks and refusals
def test_the_single_shared_stream_stays_per_step():
    plain, native = pair(3, 20, streams=False)
    assert_waves_equal(plain, native, "stepped")
    assert "single shared stream" in native.rollout_reason
    sa, sb = plain.rng.get_state(), native.rng.get_state()
    assert np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


def test_an_agent_of_another_shape_stays_per_step():
    T = 10
    agents = []
    for cls in (PointMassVecEnv, NativePointMassVecEnv):
        torch.manual_seed(0)
        env = cls(3, seed=10, device=DEV, max_timesteps=T)
        a = ddpg_agent(Args(batch_size=256, buffer_size=20 * T), env, dict(env.env_params, hidden=128), rng=fresh_rng(3))
        primed(a)
        a.enable_explore_streams(base_seed=900)
        assert not a._slab_shaped()
        agents.append(a)
    assert_waves_equal(*agents, "stepped")
    assert "not slab-shaped" in agents[1].rollout_reason
    # ... and the library refuses it when asked directly
    native = agents[1]
    eps = native._rollouts[3]
    env = native.vec_env
    env.reset()
    desc, success = env_desc(env), torch.empty(3, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match=r"hp_rollout_episodes: the agent is not slab-shaped \(hidden 128"):
        episodes(native, eps, native.explore_streams.h, desc, 1, success)


def env_desc(env, kind=None):
    d = env.native_desc()
    desc = _lib.EnvDesc(kind=d["kind"] if kind is None else kind)
    for i, v in enumerate(d["params"]):
        desc.params[i] = v
    for i, t in enumerate(d["state"]):
        desc.state_dev[i] = t.data_ptr()
    return desc


def episodes(agent, eps, streams_h, desc, explore, success):
    with agent.ctx.torch_bridge():
        _lib.check(agent.lib.hp_rollout_episodes(eps.h, agent.h, agent.o_norm.h, agent.g_norm.h, streams_h, C.byref(desc), explore,
                                                 0.05, 0.3, binomial1_qn(0.3)[0], 0.0, p(success)))


def test_refusals_carry_the_librarys_message():
    T, n = 10, 4
    torch.manual_seed(0)
    env = NativePointMassVecEnv(n, seed=1, device=DEV, max_timesteps=T)
    agent = make(env, T=T)
    primed(agent)
    eps = DeviceEpisodes(agent.ctx, agent.buffer._dev, n)
    env.reset()
    success = torch.empty(n, dtype=torch.float32, device=DEV)
    narrow = DeviceRandomStreams(2, base_seed=1, ctx=agent.ctx)
    before, pos = narrow.get_arrays(), env.pos.clone()
    with pytest.raises(ValueError, match=r"hp_rollout_episodes: env->kind 7 is not an environment kind"):
        episodes(agent, eps, narrow.h, env_desc(env, kind=7), 0, success)
    with pytest.raises(ValueError, match=r"hp_rollout_episodes: explore != 0 needs `streams`"):
        episodes(agent, eps, None, env_desc(env), 1, success)
    with pytest.raises(ValueError, match=r"hp_rollout_episodes: a wave of 4 environments is wider than the array of 2 streams"):
        episodes(agent, eps, narrow.h, env_desc(env), 1, success)
    other = DeviceEpisodes(agent.ctx, DeviceEpisodeBuffer(8, T, 10, 2, 3, ctx=agent.ctx), n)
    with pytest.raises(ValueError, match=r"hp_rollout_episodes: agent / normalizer dimensions differ from the block's"):
        episodes(agent, other, None, env_desc(env), 0, success)
    assert all(np.array_equal(x, y) for x, y in zip(narrow.get_arrays(), before)) and torch.equal(env.pos, pos)   # nothing ran
    _lib.check(agent.lib.hp_rollout_begin(eps.h, 0, 2))             # a wave the array covers is accepted
    env.reset(2)
    episodes(agent, eps, narrow.h, env_desc(env), 1, success)
    assert narrow.get_state(0)[2] != 624 and narrow.get_state(1)[2] != 624


# ------------------------------------------------------------------------------------------------- 6. train-state round trip
def test_a_saved_state_continues_with_the_same_fused_wave(tmp_path):
    T, n = 10, 3

    def build():
        torch.manual_seed(0)
        a = make(NativePointMassVecEnv(n, seed=4, device=DEV, max_timesteps=T), T=T, seed=12, n_batches=3, buffer_episodes=20)
        primed(a)
        a.enable_explore_streams(base_seed=70)
        return a

    a = build()
    a.train_cycle(a.collect_episodes_device())
    assert a.rollout_form == "fused"
    path = a.save_training_state(tmp_path / "mid.npz")
    env_rs = [r.get_state() for r in a.vec_env.rs]
    flags_a, flags_b = [], []
    want = a.collect_episodes_device(success_out=flags_a).numpy()
    want_streams = a.explore_streams.get_arrays()

    b = build()
    b.explore_streams.seed(base_seed=1)
    b.load_training_state(path)
    for r, st in zip(b.vec_env.rs, env_rs):
        r.set_state(st)
    got = b.collect_episodes_device(success_out=flags_b).numpy()
    assert b.rollout_form == "fused"
    for x, y in zip(got, want):
        assert np.array_equal(bits(x), bits(y))
    assert torch.equal(flags_a[0], flags_b[0])
    for x, y in zip(b.explore_streams.get_arrays(), want_streams):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(bits(a.vec_env.pos.cpu().numpy()), bits(b.vec_env.pos.cpu().numpy()))
