"""Native environments reset on the device (hp_env_reset, k_env_reset) and all waves of a call in one launch (hp_rollout_waves, the
wave loop of k_rollout_episodes in csrc/rollout.hip; device_env.NativePointMassVecEnv.enable_device_reset).  Every comparison is
bit for bit between two agents built identically on NativePointMassVecEnv: A as it stands (host reset, one launch per wave), B with
`enable_device_reset()`."""
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
from rl_arm_under_sparse_reward_amd.device_env import (DeviceEpisodes, NativePointMassVecEnv, NativePushBlockVecEnv, PointMassVecEnv,
                                                       binomial1_qn, script_desc)
from rl_arm_under_sparse_reward_amd.random import DeviceRandomStreams
from rollout_common import (DEV, agent_on as any_agent_on, agent_pair, assert_forms, assert_reset_streams_follow_host,
                            assert_states_bit_equal, assert_widened_states, collect_both, dev_ptr as p, make, primed)

pytestmark = pytest.mark.gpu
agent_on = functools.partial(any_agent_on, NativePointMassVecEnv, env_seed=10)
# (A: host reset, one launch per wave; B: the same with enable_device_reset())
both = functools.partial(agent_pair, NativePointMassVecEnv, env_seed=10)


def assert_calls_equal(A, B, form="fused", launches=1, **kw):
    """collect_both, the form, and with the fused form one launch count and one tensor of n_rollouts flags; A's state tensors hold
    the last wave's rows alone, B's stay [n_envs, 3]; B's reset streams against A's host generators."""
    got, flags = collect_both(A, B, **kw)
    assert_forms(A, B, form, form)
    if form == "fused":
        assert B.rollout_launches == launches, B.rollout_launches
        assert len(flags[1]) == 1                                       # one tensor of n_rollouts flags
    assert B.vec_env.active == A.vec_env.pos.shape[0]
    assert_widened_states(B.vec_env, (3, 3, 3))
    assert_reset_streams_follow_host(A, B)
    return got


# --------------------------------------------------------------------------------------------------- 1. the stand-alone reset
@pytest.mark.parametrize("n_envs", [1, 3, 5])
def test_reset_equals_the_host_reset(n_envs):
    """reset(k), full and partial, against PointMassVecEnv.reset: state, observation rows and stream states; the streams behind k
    are untouched and a cached normal survives (the reset draws no normals)."""
    host, env = PointMassVecEnv(n_envs, seed=21, device=DEV), NativePointMassVecEnv(n_envs, seed=21, device=DEV)
    last = n_envs - 1
    cached = host.rs[last].get_state()
    cached = (cached[0], cached[1], cached[2], 1, 0.3125)
    host.rs[last].set_state(cached)
    env.rs[last].set_state(cached)
    streams = env.enable_device_reset()
    assert env.reset_streams is streams and len(streams) == n_envs and env.enable_device_reset() is streams
    for k in (n_envs, max(1, n_envs - 2), n_envs, 1):
        before = streams.get_states()
        want, got = host.reset(k), env.reset(None if k == n_envs else k)
        assert env.active == k
        for key in want:
            assert got[key].shape == want[key].shape and np.array_equal(bits(got[key].cpu().numpy()), bits(want[key].cpu().numpy())), (k, key)
        for name in ("pos", "vel", "goal"):
            x, y = getattr(host, name), getattr(env, name)
            assert tuple(y.shape) == (n_envs, 3) and np.array_equal(bits(x.cpu().numpy()), bits(y[:k].cpu().numpy())), (k, name)
        after = streams.get_states()
        for i in range(n_envs):
            assert_states_bit_equal(host.rs[i].get_state(), after[i], (k, i))
            if i >= k:
                assert_states_bit_equal(before[i], after[i], (k, i, "untouched"))
        assert after[last][3] == 1 and after[last][4] == 0.3125
    # the per-step protocol on the first `active` rows
    host.reset(max(1, n_envs - 1)); env.reset(max(1, n_envs - 1))
    act = torch.from_numpy(np.random.RandomState(0).uniform(-0.7, 0.7, (env.active, 4)).astype(np.float32)).to(DEV)
    (oa, ra, _, ia), (ob, rb, _, ib) = host.step(act), env.step(act)
    for key in oa:
        assert np.array_equal(bits(oa[key].cpu().numpy()), bits(ob[key].cpu().numpy())), key
    assert torch.equal(ra, rb) and torch.equal(ia["is_success"], ib["is_success"])


# ------------------------------------------------------------------------- 2. one launch, many waves, exploring with streams
@pytest.mark.parametrize("epoch", [0, 100])
@pytest.mark.parametrize("n_envs,n_rollouts", [(1, 1), (3, 3), (4, 7), (5, 3), (9, 20), (2, 25)])
def test_all_waves_in_one_launch_equal_one_launch_per_wave(n_envs, n_rollouts, epoch):
    """Full slabs, partial slabs and partial waves: a partial last wave leaves the streams of the environments it leaves out where
    the wave before left them (A's host generators and exploration streams say where that is)."""
    A, B = both(n_envs, 20)
    assert_calls_equal(A, B, n_rollouts=n_rollouts, epoch=epoch)
    assert B.vec_env.active == (n_rollouts - 1) % n_envs + 1


# ------------------------------------------------------------------------------------------------------------ 3. noise-free
@pytest.mark.parametrize("streams", [True, False])
def test_noise_free_waves_equal(streams):
    A, B = both(4, 20, streams=streams)
    before = B.explore_streams.get_states() if streams else None
    assert_calls_equal(A, B, explore=False, n_rollouts=7)
    if streams:
        for i, (x, y) in enumerate(zip(before, B.explore_streams.get_states())):
            assert_states_bit_equal(x, y, i)


@pytest.mark.parametrize("n_test", [3, 10])
def test_evaluation_returns_the_same_rate_in_one_launch(n_test):
    A, B = both(4, 20, n_test_rollouts=n_test)
    rates = [a._eval_agent() for a in (A, B)]
    assert A.rollout_form == B.rollout_form == "fused" and B.rollout_launches == 1
    assert isinstance(rates[1], float) and rates[0] == rates[1], rates
    for i, (r, y) in enumerate(zip(A.vec_env.rs, B.vec_env.reset_streams.get_states())):
        assert_states_bit_equal(r.get_state(), y, i)


# ------------------------------------------------------------------- 4. a block boundary in the reset stream inside a launch
@pytest.mark.parametrize("start_pos", [None, 618])
def test_the_reset_stream_crosses_a_block_inside_a_launch(start_pos):
    """Twelve words per reset: from a fresh stream the 624-word block ends after 52 resets, so the key is regenerated and committed
    mid-launch; from pos = 618 the very first reset straddles a block."""
    def shift(rs):
        if start_pos is not None:
            st = rs.get_state()
            rs.set_state((st[0], st[1], start_pos, 0, 0.0))

    A, B = both(1, 2, before_reset=lambda a: shift(a.vec_env.rs[0]))
    key0 = B.vec_env.reset_streams.get_state(0)[1].copy()
    assert_calls_equal(A, B, n_rollouts=60)
    host = np.random.RandomState(10)
    shift(host)
    for _ in range(60):
        host.uniform(0.0, 0.5, 3); host.uniform(0.0, 0.5, 3)
    got = B.vec_env.reset_streams.get_state(0)
    assert_states_bit_equal(host.get_state(), got, "60 resets")
    assert not np.array_equal(got[1], key0) and 0 < got[2] < 624


# -------------------------------------------------------------------------------------- 5. the per-step path with device reset
def test_the_shared_stream_stays_per_step_and_resets_on_the_device():
    A, B = both(3, 20, streams=False)
    assert_calls_equal(A, B, form="stepped", n_rollouts=5)
    assert "single shared stream" in B.rollout_reason and B.rollout_launches is None
    sa, sb = A.rng.get_state(), B.rng.get_state()
    assert np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


# ------------------------------------------------------------------------------------------------------ 6. enabling mid-run
def test_enabling_mid_run_continues_the_sequence():
    A, B = agent_on(3, 20), agent_on(3, 20)
    first = [a.collect_episodes_device(n_rollouts=2).numpy() for a in (A, B)]       # a partial wave on the host reset: [2, 3] tensors
    for x, y in zip(*first):
        assert np.array_equal(bits(x), bits(y))
    B.vec_env.enable_device_reset(B.ctx)
    assert tuple(B.vec_env.pos.shape) == (3, 3) and B.vec_env.active == 2
    assert np.array_equal(bits(A.vec_env.pos.cpu().numpy()), bits(B.vec_env.pos[:2].cpu().numpy()))
    assert_calls_equal(A, B, n_rollouts=3)
    assert_calls_equal(A, B, n_rollouts=4)


# ---------------------------------------------------------------------------------------------------------- 7. the launch cap
@pytest.mark.parametrize("cap,launches", [(10, 2), (1, 3)])
def test_a_call_split_by_the_launch_cap_gives_the_same_bits(cap, launches):
    """T = 5, eight episodes on three environments = three waves; a cap of ten timesteps holds two waves, a cap below T one."""
    T, n, total = 5, 3, 8
    A, B = both(n, T)
    B._rollouts[total] = DeviceEpisodes(B.ctx, B.buffer._dev, total)
    _lib.check(B.lib.hp_rollout_debug_set_launch_cap(B._rollouts[total].h, cap))
    assert_calls_equal(A, B, launches=launches, n_rollouts=total)
    _lib.check(B.lib.hp_rollout_debug_set_launch_cap(B._rollouts[total].h, 0))
    assert_calls_equal(A, B, launches=1, n_rollouts=total)


# --------------------------------------------------------------------------------------- 8. a cycle on top, the training state
def test_cycles_and_the_training_state(tmp_path):
    T, n, kw = 10, 3, dict(n_batches=3, buffer_episodes=20, seed=12)

    def same_learner(x, y):
        for slot in (NET_ACTOR, NET_CRITIC):
            assert np.array_equal(bits(x._get_flat(slot)), bits(y._get_flat(slot))), slot
        sa, sb = x.rng.get_state(), y.rng.get_state()
        assert np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]

    A, B = both(n, T, **kw)
    for a in (A, B):
        a.train_cycle(a.collect_episodes_device(n_rollouts=5))
    assert B.rollout_launches == 1 and A.buffer.current_size == B.buffer.current_size == 5
    same_learner(A, B)
    path = B.save_training_state(tmp_path / "mid.npz")
    arrays, manifest = ts.read_state(path)
    assert manifest["reset_streams"]["n"] == n and manifest["explore_streams"]["n"] == n
    for name, a in zip(ts.RESET_STREAM_ARRAYS, B.vec_env.reset_streams.get_arrays()):
        assert np.array_equal(bits(arrays[name]), bits(a)), name
    ts.verify(path)
    for a in (A, B):
        a.train_cycle(a.collect_episodes_device(n_rollouts=5))
    same_learner(A, B)

    R = agent_on(n, T, reset=True, env_seed=77, base=1, **kw)            # other reset generators, other exploration streams
    R.load_training_state(path)
    got = R.collect_episodes_device(n_rollouts=5)
    want = B._rollouts[5].numpy()
    for x, y in zip(got.numpy(), want):
        assert np.array_equal(bits(x), bits(y))
    R.train_cycle(got)
    same_learner(B, R)
    for x, y in zip(R.vec_env.reset_streams.get_arrays(), B.vec_env.reset_streams.get_arrays()):
        assert np.array_equal(bits(x), bits(y))
    # a delta carries them too
    delta = B.save_training_state(tmp_path / "d.npz", base=path)
    assert ts.read_manifest(delta)["reset_streams"]["n"] == n and ts.verify(delta, base=path)["kind"] == "delta"


# ------------------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_carry_the_librarys_message(tmp_path):
    T, n = 10, 4
    B = agent_on(n, T, reset=True)
    env, lib = B.vec_env, B.lib
    eps = DeviceEpisodes(B.ctx, B.buffer._dev, n)
    success = torch.empty(n, dtype=torch.float32, device=DEV)
    narrow = DeviceRandomStreams(2, base_seed=1, ctx=B.ctx)
    env.reset()
    state = (env.reset_streams.get_arrays(), narrow.get_arrays(), B.explore_streams.get_arrays(), env.pos.clone(), env.goal.clone())

    def waves(reset_h, desc, n_envs=n):
        with B.ctx.torch_bridge():
            _lib.check(lib.hp_rollout_waves(eps.h, B.h, B.o_norm.h, B.g_norm.h, B.explore_streams.h, reset_h, C.byref(desc), n_envs, 1,
                                            0.05, 0.3, binomial1_qn(0.3)[0], 0.0, p(success), None))

    def reset(reset_h, desc, rows):
        with B.ctx.torch_bridge():
            _lib.check(lib.hp_env_reset(B.ctx.h, C.byref(desc), reset_h, rows))

    def desc(kind=None, null=None):
        d = env.env_desc()
        if kind is not None:
            d.kind = kind
        if null is not None:
            d.state_dev[null] = None
        return d

    with pytest.raises(ValueError, match=r"hp_rollout_waves: 4 environments, but the array holds 2 reset streams"):
        waves(narrow.h, desc())
    with pytest.raises(ValueError, match=r"hp_env_reset: 3 environments, but the array holds 2 reset streams"):
        reset(narrow.h, desc(), 3)
    with pytest.raises(ValueError, match=r"hp_rollout_begin: episodes \[0, 5\) outside the block of 4"):
        _lib.check(lib.hp_rollout_begin(eps.h, 0, n + 1))
    with pytest.raises(ValueError, match=r"hp_rollout_waves: env->state_dev\[1\] is null"):
        waves(env.reset_streams.h, desc(null=1))
    with pytest.raises(ValueError, match=r"hp_env_reset: env->state_dev\[2\] is null"):
        reset(env.reset_streams.h, desc(null=2), n)
    with pytest.raises(ValueError, match=r"hp_rollout_waves: null argument"):
        waves(None, desc())
    with pytest.raises(ValueError, match=r"hp_env_reset: null argument"):
        reset(None, desc(), n)
    with pytest.raises(ValueError, match=r"hp_rollout_waves: env->kind 7 is not an environment kind"):
        waves(env.reset_streams.h, desc(kind=7))
    with pytest.raises(ValueError, match=r"hp_env_reset: env->kind 7 is not an environment kind"):
        reset(env.reset_streams.h, desc(kind=7), n)
    other = _lib.Context(0)
    foreign = DeviceRandomStreams(n, base_seed=1, ctx=other)
    with pytest.raises(ValueError, match=r"hp_rollout_waves: handles belong to different contexts"):
        waves(foreign.h, desc())
    with pytest.raises(ValueError, match=r"hp_env_reset: handles belong to different contexts"):
        reset(foreign.h, desc(), n)
    after = (env.reset_streams.get_arrays(), narrow.get_arrays(), B.explore_streams.get_arrays(), env.pos, env.goal)
    for x, y in zip(state[:3], after[:3]):
        assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(x, y))                                  # nothing ran
    assert torch.equal(state[3], after[3]) and torch.equal(state[4], after[4])
    waves(env.reset_streams.h, desc())                                                                     # ... and a good call does
    assert not torch.equal(state[4], env.goal)

    # the training state, both directions and the count
    A = agent_on(n, T, reset=False)
    with_streams, without = B.save_training_state(tmp_path / "b.npz"), A.save_training_state(tmp_path / "a.npz")
    with pytest.raises(ts.StateError, match=r"the state carries 4 per-environment reset streams .*call vec_env.enable_device_reset"):
        A.load_training_state(with_streams)
    with pytest.raises(ts.StateError, match=r"the agent's environment is reset on the device, but the state was saved without reset streams"):
        B.load_training_state(without)
    wide = agent_on(n + 1, T, reset=True)
    wide.explore_streams = B.explore_streams                     # (the exploration streams' own count check comes first)
    with pytest.raises(ts.StateError, match=r"array 'reset_stream_keys' holds 4 streams, the agent has 5 environments"):
        wide.load_training_state(with_streams)
    A.load_training_state(without)                               # a state without the field loads as before


@pytest.mark.parametrize("cls", [NativePointMassVecEnv, NativePushBlockVecEnv])
def test_the_row_of_a_kind_refuses_on_the_host(cls):
    """What the entries check against a kind's row of the library's table, for both kinds, where no other test does: dimensions
    other than the block's (both rollout entries) and a null LAST state array (both rollout entries; hp_env_reset and the unknown
    kind are covered above and in test_gpu_push_block.py).  5 environments = one full slab and one of a single row, 7 episodes =
    two waves, the second partial.  Nothing is launched: environments, streams and block keep their bytes."""
    T, n, total = 3, 5, 7
    torch.manual_seed(0)
    agent = make(cls(n, seed=10, device=DEV, max_timesteps=T), T=T, noise_eps=0.05)
    primed(agent)
    agent.enable_explore_streams(base_seed=900)
    env = agent.vec_env
    env.enable_device_reset(agent.ctx)
    env.reset()
    last = len(env.state_names) - 1
    eps = DeviceEpisodes(agent.ctx, agent.buffer._dev, total)
    success = torch.zeros(total, dtype=torch.float32, device=DEV)
    # an agent and a block of other dimensions, in the same context
    torch.manual_seed(0)
    small = ddpg_agent(Args(batch_size=256, buffer_size=200), None,
                       {'obs': 10, 'goal': 2, 'action': 3, 'action_max': 0.5, 'max_timesteps': T}, ctx=agent.ctx, rng=fresh_rng(3))
    other = DeviceEpisodes(small.ctx, small.buffer._dev, total)

    def snapshot():
        return ([getattr(env, name).clone() for name in env.state_names] + [success.clone()],
                [*env.reset_streams.get_arrays(), *agent.explore_streams.get_arrays(), *eps.numpy(), *other.numpy()])

    def desc(null=None):
        d = env.env_desc()
        if null is not None:
            d.state_dev[null] = None
        return d

    launches = C.c_int32(-1)

    def waves(a, block, d):
        with a.ctx.torch_bridge():
            _lib.check(a.lib.hp_rollout_begin(block.h, 0, total))
            _lib.check(a.lib.hp_rollout_waves(block.h, a.h, a.o_norm.h, a.g_norm.h, agent.explore_streams.h, env.reset_streams.h,
                                              C.byref(d), n, 1, 0.05, 0.3, binomial1_qn(0.3)[0], 0.0, p(success), C.byref(launches)))

    def episodes(a, block, d):
        with a.ctx.torch_bridge():
            _lib.check(a.lib.hp_rollout_begin(block.h, 0, n))
            _lib.check(a.lib.hp_rollout_episodes(block.h, a.h, a.o_norm.h, a.g_norm.h, agent.explore_streams.h, C.byref(d), 1, 0.05, 0.3,
                                                 binomial1_qn(0.3)[0], 0.0, p(success)))

    kind = env.kind
    tensors, arrays = snapshot()
    for entry, call in (("hp_rollout_waves", waves), ("hp_rollout_episodes", episodes)):
        with pytest.raises(ValueError, match=rf"{entry}: env->kind {kind} has dimensions 27 / 3 / 4, the block has 10 / 2 / 3"):
            call(small, other, desc())
        with pytest.raises(ValueError, match=rf"{entry}: env->state_dev\[{last}\] is null"):
            call(agent, eps, desc(null=last))
    after_t, after_a = snapshot()
    assert all(torch.equal(x, y) for x, y in zip(tensors, after_t))                                         # nothing ran
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(arrays, after_a)) and launches.value == -1
    waves(agent, eps, desc())                                                                               # ... and a good call does
    assert launches.value == 1
    assert not all(np.array_equal(bits(x), bits(y)) for x, y in zip(arrays, snapshot()[1]))


def test_the_shared_descriptor_check_keeps_every_entrys_order():
    """Two faults in one call, for every entry that reads a descriptor: the refusal is the one the first failing check gives, in
    the order every entry has had -- the kind's row first, then the state arrays, then the block's dimensions.  An unknown kind
    with a null state_dev[0] is refused for the kind; a null state_dev[0] with a block of other dimensions is refused for the
    array (hp_env_reset takes no block: there the array is the only fault).  4 environments, T = 4; everything is refused on the
    host: nothing is launched, and the environments keep their bytes."""
    T, n = 4, 4
    torch.manual_seed(0)
    agent = make(NativePushBlockVecEnv(n, seed=10, device=DEV, max_timesteps=T), T=T, noise_eps=0.05)
    primed(agent)
    agent.enable_explore_streams(base_seed=900)
    env = agent.vec_env
    env.enable_device_reset(agent.ctx)
    env.reset()
    eps = DeviceEpisodes(agent.ctx, agent.buffer._dev, n)
    torch.manual_seed(0)
    small = ddpg_agent(Args(batch_size=256, buffer_size=200), None,
                       {'obs': 10, 'goal': 2, 'action': 3, 'action_max': 0.5, 'max_timesteps': T}, ctx=agent.ctx, rng=fresh_rng(3))
    other = DeviceEpisodes(small.ctx, small.buffer._dev, n)
    success = torch.zeros(n, dtype=torch.float32, device=DEV)
    step_success = torch.zeros((n, T), dtype=torch.float32, device=DEV)
    launches, lib, ctx = C.c_int32(-1), agent.lib, agent.ctx
    script = script_desc()
    qn = binomial1_qn(0.3)[0]

    def episodes(a, block, d):
        _lib.check(lib.hp_rollout_begin(block.h, 0, n))
        _lib.check(lib.hp_rollout_episodes(block.h, a.h, a.o_norm.h, a.g_norm.h, agent.explore_streams.h, C.byref(d), 1, 0.05, 0.3, qn,
                                           0.0, p(success)))

    def waves(a, block, d):
        _lib.check(lib.hp_rollout_begin(block.h, 0, n))
        _lib.check(lib.hp_rollout_waves(block.h, a.h, a.o_norm.h, a.g_norm.h, agent.explore_streams.h, env.reset_streams.h, C.byref(d),
                                        n, 1, 0.05, 0.3, qn, 0.0, p(success), C.byref(launches)))

    def demos(a, block, d):
        _lib.check(lib.hp_demo_episodes(ctx.h, C.byref(d), env.reset_streams.h, C.byref(script), n, 0, n, T, block.h, p(success),
                                        p(step_success), C.byref(launches)))

    def reset(a, block, d):
        _lib.check(lib.hp_env_reset(ctx.h, C.byref(d), env.reset_streams.h, n))

    def desc(kind=None):
        d = env.env_desc()
        d.state_dev[0] = None
        if kind is not None:
            d.kind = kind
        return d

    before = [getattr(env, name).clone() for name in env.state_names], env.reset_streams.get_arrays()
    with ctx.torch_bridge():
        for entry, call in (("hp_rollout_episodes", episodes), ("hp_rollout_waves", waves), ("hp_demo_episodes", demos),
                            ("hp_env_reset", reset)):
            with pytest.raises(ValueError, match=rf"^{entry}: env->kind 99 is not an environment kind of this build$"):
                call(agent, eps, desc(kind=99))
            with pytest.raises(ValueError, match=rf"^{entry}: env->state_dev\[0\] is null$"):
                call(small, other, desc())
    assert launches.value == -1
    assert all(torch.equal(x, getattr(env, name)) for x, name in zip(before[0], env.state_names))
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(before[1], env.reset_streams.get_arrays()))
