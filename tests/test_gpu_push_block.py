"""The native push-block environment on the device (PushBlockEnvDev in csrc/env_device.h, the kernels of csrc/rollout_episodes.h
instantiated in csrc/env_push_block.hip, device_env.NativePushBlockVecEnv): the rejection loop of its reset against the host twin,
one launch per wave against the per-step form on the torch twin, all waves in one launch with the reset on the device against one
launch per wave with the host reset, the training state, and the refusals.  Every comparison is bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import bits
from gpu_common import fresh_rng
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd import train_state as ts
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_CRITIC, ddpg_agent
from rl_arm_under_sparse_reward_amd.device_env import DeviceEpisodes, NativePushBlockVecEnv, PushBlockVecEnv, binomial1_qn
from rollout_common import (CONTACT, DEV, agent_on as any_agent_on, agent_pair, assert_forms, assert_reset_streams_follow_host,
                            assert_states_bit_equal, assert_widened_states, collect_both, dev_ptr as p)

pytestmark = pytest.mark.gpu
T = 20
agent_on = functools.partial(any_agent_on, T=T, env_seed=21)
PARAMS = {"default": {}, "contact": CONTACT}
# Contact-heavy cases whose episodes miss a branch with the seeds of the others (environments from 21, networks from 0): what they
# are built with instead.  Keys: ("wave", n_envs, n_rollouts, explore, epoch).
SEEDS = {
    ("wave", 1, 1, True, 100): dict(env_seed=42),
    ("wave", 3, 3, True, 100): dict(env_seed=25),
    ("wave", 5, 3, True, 100): dict(env_seed=25),
    # noise-free, the policy alone steers: network 0 pushes the block along y in every step, network 5 comes in from the side once
    **{("wave", n, r, False, epoch): dict(net_seed=5) for n, r in ((1, 1), (3, 3), (5, 3)) for epoch in (0, 100)},
    ("wave", 4, 7, False, 0): dict(env_seed=32),
    ("wave", 4, 7, False, 100): dict(env_seed=32),
}


def setup(params, case):
    """(environment parameters, agent_on's arguments) of a case"""
    if params == "default":
        return {}, {"env_seed": 21}
    return CONTACT, dict({"env_seed": 21, "random_eps": 0.3}, **SEEDS.get(case, {}))


def assert_contact_coverage(obs):
    """The block's velocity (observation [21:24]) over the timesteps behind a step: pushed along x, pushed along y, left alone"""
    bvel = obs[:, 1:, 21:24]
    x, y, still = int((bvel[..., 0] != 0).sum()), int((bvel[..., 1] != 0).sum()), int((~bvel.any(axis=-1)).sum())
    print(f"contact coverage: {x} timesteps pushed along x, {y} along y, {still} without contact, of {bvel.shape[0] * bvel.shape[1]}")
    assert x > 0 and y > 0 and still > 0, (x, y, still)
    assert not bvel[..., 2].any()


# --------------------------------------------------------------------------------------------------- 1. the stand-alone reset
@pytest.mark.parametrize("n_envs", [1, 3, 5])
def test_reset_equals_the_host_reset(n_envs):
    """reset(k), full and partial, against PushBlockVecEnv.reset: state, observation rows and stream states; environments 21 .. 25
    take 1 to 4 attempts a reset, the streams behind k are untouched and a cached normal survives."""
    host, env = PushBlockVecEnv(n_envs, seed=21, device=DEV), NativePushBlockVecEnv(n_envs, seed=21, device=DEV)
    last = n_envs - 1
    cached = host.rs[last].get_state()
    cached = (cached[0], cached[1], cached[2], 1, 0.3125)
    host.rs[last].set_state(cached)
    env.rs[last].set_state(cached)
    streams = env.enable_device_reset()
    assert env.reset_streams is streams and len(streams) == n_envs and env.enable_device_reset() is streams
    attempts = []
    for k in (n_envs, max(1, n_envs - 2), n_envs, 1, n_envs, n_envs, n_envs, n_envs):
        before = streams.get_states()
        want, got = host.reset(k), env.reset(None if k == n_envs else k)
        attempts += host.reset_attempts[:k]
        assert env.active == k
        for key in want:
            assert got[key].shape == want[key].shape and np.array_equal(bits(got[key].cpu().numpy()), bits(want[key].cpu().numpy())), (k, key)
        for name, width in zip(env.state_names, (3, 3, 3, 6)):
            x, y = getattr(host, name), getattr(env, name)
            assert tuple(y.shape) == (n_envs, width) and np.array_equal(bits(x.cpu().numpy()), bits(y[:k].cpu().numpy())), (k, name)
        after = streams.get_states()
        for i in range(n_envs):
            assert_states_bit_equal(host.rs[i].get_state(), after[i], (k, i))
            if i >= k:
                assert_states_bit_equal(before[i], after[i], (k, i, "untouched"))
        assert after[last][3] == 1 and after[last][4] == 0.3125
    assert 1 in attempts and max(attempts) >= 2, attempts            # first-try and multi-try resets
    print("attempts:", attempts)
    # the per-step protocol on the first `active` rows
    host.reset(max(1, n_envs - 1)); env.reset(max(1, n_envs - 1))
    act = torch.from_numpy(np.random.RandomState(0).uniform(-0.7, 0.7, (env.active, 4)).astype(np.float32)).to(DEV)
    (oa, ra, _, ia), (ob, rb, _, ib) = host.step(act), env.step(act)
    for key in oa:
        assert np.array_equal(bits(oa[key].cpu().numpy()), bits(ob[key].cpu().numpy())), key
    assert torch.equal(ra, rb) and torch.equal(ia["is_success"], ib["is_success"])


def test_an_exhausted_reset_on_the_device_keeps_the_last_attempt():
    """min_separation = 10 accepts nothing: 100 attempts, 800 words, across a block regeneration to position 176; the second
    environment's stream starts at 618, so its first attempt straddles a block"""
    host, env = (cls(2, seed=21, device=DEV, min_separation=10.0) for cls in (PushBlockVecEnv, NativePushBlockVecEnv))
    for e in (host, env):
        st = e.rs[1].get_state()
        e.rs[1].set_state((st[0], st[1], 618, 0, 0.0))
    key0 = env.rs[0].get_state()[1].copy()
    streams = env.enable_device_reset()
    want, got = host.reset(), env.reset()
    assert host.reset_attempts == [100, 100]
    for key in want:
        assert np.array_equal(bits(got[key].cpu().numpy()), bits(want[key].cpu().numpy())), key
    for name in env.state_names:
        assert np.array_equal(bits(getattr(host, name).cpu().numpy()), bits(getattr(env, name).cpu().numpy())), name
    after = streams.get_states()
    for i in range(2):
        assert_states_bit_equal(host.rs[i].get_state(), after[i], i)
    assert after[0][2] == 176 and not np.array_equal(after[0][1], key0)


# -------------------------------------------------------------------------------- 2. one launch per wave against the per-step form
@pytest.mark.parametrize("params", sorted(PARAMS))
@pytest.mark.parametrize("epoch", [0, 100])
@pytest.mark.parametrize("explore", [False, True])
@pytest.mark.parametrize("n_envs,n_rollouts", [(1, 1), (3, 3), (5, 3), (4, 7)])
def test_fused_wave_equals_the_per_step_path(n_envs, n_rollouts, explore, epoch, params):
    """Two agents built identically, one on PushBlockVecEnv (two launches and the torch twin's kernels per timestep), one on the
    native environment (one launch per wave), both reset on the host: episodes, flags, final state, exploration streams."""
    env_kw, kw = setup(params, ("wave", n_envs, n_rollouts, explore, epoch))
    plain, native = (agent_on(cls, n_envs, env_kw=env_kw, **kw) for cls in (PushBlockVecEnv, NativePushBlockVecEnv))
    before = native.explore_streams.get_states()
    (obs, ag, g, actions), flags = collect_both(plain, native, n_rollouts=n_rollouts, explore=explore, epoch=epoch)
    assert_forms(plain, native, "stepped", "fused")
    assert len(flags[0]) == len(flags[1]) == -(-n_rollouts // n_envs)
    assert np.array_equal(ag, obs[:, :, 12:15]) and np.array_equal(obs[:, :, 18:21], obs[:, :, 12:15] - obs[:, :, 0:3])
    assert not obs[:, :, 3:6].any() and not obs[:, :, 9:12].any() and not obs[:, :, 15:18].any() and not obs[:, :, 24:27].any()
    moved = [not np.array_equal(x[1], y[1]) or x[2] != y[2] for x, y in zip(before, native.explore_streams.get_states())]
    assert moved == [explore and i < n_rollouts for i in range(n_envs)]
    if explore and epoch >= 100:
        assert np.abs(actions).max() <= float(np.float32(0.15))
    if params == "contact":
        assert_contact_coverage(obs)


# ------------------------------------------------------------------- 3. all waves in one launch, the reset on the device
# (A: host reset, one launch per wave; B: the same with enable_device_reset())
both = functools.partial(agent_pair, NativePushBlockVecEnv, T=T, env_seed=21)


def assert_calls_equal(A, B, launches=1, **kw):
    got, flags = collect_both(A, B, **kw)
    assert_forms(A, B, "fused", "fused")
    assert B.rollout_launches == launches and len(flags[1]) == 1, B.rollout_launches
    assert_widened_states(B.vec_env, (3, 3, 3, 6))
    assert_reset_streams_follow_host(A, B)
    return got


def reset_attempts(env, n_rollouts):
    """(attempts, resets) of a first call of n_rollouts episodes on fresh host generators: eight words an attempt"""
    words = sum(int(r.get_state()[2]) % 624 for r in env.rs)
    assert words % 8 == 0 and all(r.get_state()[2] < 624 for r in env.rs[:min(n_rollouts, env.n_envs)])
    return words // 8, n_rollouts


@pytest.mark.parametrize("params", sorted(PARAMS))
@pytest.mark.parametrize("epoch", [0, 100])
@pytest.mark.parametrize("n_envs,n_rollouts", [(4, 7), (9, 20), (2, 25)])
def test_all_waves_in_one_launch_equal_one_launch_per_wave(n_envs, n_rollouts, epoch, params):
    """Exploring with streams: the exploration stream of a row leaves its ring for as many reset draws as the row's rejection loop
    takes and must come back where it was; a partial last wave leaves the streams of the environments it leaves out alone."""
    env_kw, kw = setup(params, ("waves", n_envs, n_rollouts, epoch))
    A, B = both(n_envs, env_kw=env_kw, **kw)
    obs = assert_calls_equal(A, B, n_rollouts=n_rollouts, epoch=epoch)[0]
    assert B.vec_env.active == (n_rollouts - 1) % n_envs + 1
    attempts, resets = reset_attempts(A.vec_env, n_rollouts)
    print(f"{attempts} attempts in {resets} resets")
    assert attempts > resets                                       # multi-attempt detours happened
    if params == "contact":
        assert_contact_coverage(obs)
    assert_calls_equal(A, B, n_rollouts=n_envs + 1, epoch=epoch)     # a second call continues every stream


def test_noise_free_waves_equal():
    A, B = both(4)
    before = B.explore_streams.get_states()
    assert_calls_equal(A, B, explore=False, n_rollouts=7)
    for i, (x, y) in enumerate(zip(before, B.explore_streams.get_states())):
        assert_states_bit_equal(x, y, i)
    rates = [a._eval_agent() for a in (A, B)]
    assert isinstance(rates[1], float) and rates[0] == rates[1] and B.rollout_launches == 1, rates


@pytest.mark.parametrize("cap,launches", [(10, 2), (1, 3)])
def test_a_call_split_by_the_launch_cap_gives_the_same_bits(cap, launches):
    """T = 5, eight episodes on three environments = three waves; a cap of ten timesteps holds two waves, a cap below T one."""
    n, total = 3, 8
    A, B = both(n, T=5, env_kw=CONTACT, random_eps=0.3)
    B._rollouts[total] = DeviceEpisodes(B.ctx, B.buffer._dev, total)
    _lib.check(B.lib.hp_rollout_debug_set_launch_cap(B._rollouts[total].h, cap))
    assert_calls_equal(A, B, launches=launches, n_rollouts=total)
    attempts, resets = reset_attempts(A.vec_env, total)
    assert attempts > resets
    _lib.check(B.lib.hp_rollout_debug_set_launch_cap(B._rollouts[total].h, 0))
    assert_calls_equal(A, B, launches=1, n_rollouts=total)


# --------------------------------------------------------------------------------------- 4. a cycle on top, the training state
def test_a_state_saved_after_a_multi_attempt_wave_resumes_bit_for_bit(tmp_path):
    n, kw = 3, dict(T=10, n_batches=3, buffer_episodes=20, seed=12)
    B = agent_on(NativePushBlockVecEnv, n, reset=True, **kw)
    B.train_cycle(B.collect_episodes_device(n_rollouts=5))
    assert B.rollout_form == "fused" and B.rollout_launches == 1
    pos = B.vec_env.reset_streams.get_arrays()[1]
    assert int(pos.sum()) % 8 == 0 and int(pos.sum()) // 8 > 5, pos      # environments 21 .. 23: more attempts than resets
    path = B.save_training_state(tmp_path / "mid.npz")
    arrays, manifest = ts.read_state(path)
    assert manifest["reset_streams"]["n"] == n and manifest["explore_streams"]["n"] == n
    for name, a in zip(ts.RESET_STREAM_ARRAYS, B.vec_env.reset_streams.get_arrays()):
        assert np.array_equal(bits(arrays[name]), bits(a)), name
    ts.verify(path)
    flags_b, flags_r = [], []
    want = [x.copy() for x in B.collect_episodes_device(n_rollouts=5, success_out=flags_b).numpy()]
    B.train_cycle(B._rollouts[5])

    R = agent_on(NativePushBlockVecEnv, n, reset=True, env_seed=77, base=1, **kw)    # other reset generators, other exploration streams
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


# ------------------------------------------------------------------------------------------------------------ 5. refusals
def episodes(agent, eps, desc, success):
    with agent.ctx.torch_bridge():
        _lib.check(agent.lib.hp_rollout_episodes(eps.h, agent.h, agent.o_norm.h, agent.g_norm.h, None, C.byref(desc), 0,
                                                 0.05, 0.3, binomial1_qn(0.3)[0], 0.0, p(success)))


def test_refusals_carry_the_librarys_message():
    n = 4
    agent = agent_on(NativePushBlockVecEnv, n, T=10, streams=False)
    env = agent.vec_env
    eps = DeviceEpisodes(agent.ctx, agent.buffer._dev, n)
    env.reset()
    success = torch.empty(n, dtype=torch.float32, device=DEV)
    state = [getattr(env, name).clone() for name in env.state_names]

    def desc(kind=None, null=None):
        d = env.env_desc()
        if kind is not None:
            d.kind = kind
        if null is not None:
            d.state_dev[null] = None
        return d

    with pytest.raises(ValueError, match=r"hp_rollout_episodes: env->kind 7 is not an environment kind"):
        episodes(agent, eps, desc(kind=7), success)
    with pytest.raises(ValueError, match=r"hp_rollout_episodes: env->state_dev\[3\] is null"):
        episodes(agent, eps, desc(null=3), success)
    streams = env.enable_device_reset(agent.ctx)
    with pytest.raises(ValueError, match=r"hp_env_reset: env->state_dev\[3\] is null"):
        with agent.ctx.torch_bridge():
            _lib.check(agent.lib.hp_env_reset(agent.ctx.h, C.byref(desc(null=3)), streams.h, n))
    with pytest.raises(ValueError, match=r"hp_env_reset: env->kind 7 is not an environment kind"):
        with agent.ctx.torch_bridge():
            _lib.check(agent.lib.hp_env_reset(agent.ctx.h, C.byref(desc(kind=7)), streams.h, n))
    # a push-block descriptor on a block of other dimensions (with an agent of those dimensions)
    torch.manual_seed(0)
    small = ddpg_agent(Args(batch_size=256, buffer_size=200), None,
                       {'obs': 10, 'goal': 2, 'action': 3, 'action_max': 0.5, 'max_timesteps': 10}, rng=fresh_rng(3))
    other = DeviceEpisodes(small.ctx, small.buffer._dev, n)
    with pytest.raises(ValueError, match=r"hp_rollout_episodes: env->kind 2 has dimensions 27 / 3 / 4, the block has 10 / 2 / 3"):
        episodes(small, other, desc(), success)
    for name, before in zip(env.state_names, state):
        assert torch.equal(getattr(env, name), before), name                                                # nothing ran
    episodes(agent, eps, desc(), success)                                                                   # ... and a good call does
    assert not torch.equal(env.grip, state[0])
