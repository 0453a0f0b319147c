"""Helpers shared by the -m gpu rollout, environment and demonstration tests: agents built identically on a vectorised environment,
one collect_episodes_device call on two of them compared bit for bit, and generated demonstrations against host twins."""
import ctypes as C

import numpy as np
import torch

from conftest import bits
from gpu_common import ctx, fresh_rng
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
from rl_arm_under_sparse_reward_amd.device_env import (DeviceEpisodes, NativePickPlaceVecEnv, NativePointMassVecEnv,
                                                       NativePushBlockVecEnv)
from rl_arm_under_sparse_reward_amd.synthetic import PickPlaceGoalEnv, PointMassGoalEnv, PushBlockGoalEnv

DEV = "cuda:0"
NAMES = ("obs", "ag", "g", "actions", "info")
# push-block parameters under which a random policy touches the block every few steps (a 4 cm block is rarely touched at all)
CONTACT = dict(half_width=0.15, z_touch=0.6, step_scale=0.3)


def dev_ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def make(env, T=50, seed=3, **kw):
    """An agent on `env`: a host environment, a list of them, a vectorised device environment, or None (bmirobot-shaped)"""
    args = Args(batch_size=256, buffer_size=kw.pop("buffer_episodes", 200) * T, **kw)
    first = env[0] if isinstance(env, list) else env
    params = first.env_params if first is not None else PointMassGoalEnv(max_timesteps=T).env_params
    return ddpg_agent(args, env, params, rng=fresh_rng(seed))


def primed(agent, seed=0):
    rs = np.random.RandomState(seed)
    agent.o_norm.update(rs.normal(0.2, 0.3, size=(400, 27))); agent.o_norm.recompute_stats()
    agent.g_norm.update(rs.normal(0.25, 0.1, size=(400, 3))); agent.g_norm.recompute_stats()
    return rs


def assert_states_bit_equal(a, b, where):
    assert np.array_equal(a[1], b[1]) and a[2:4] == b[2:4] and np.float64(a[4]).tobytes() == np.float64(b[4]).tobytes(), where


# ------------------------------------------------------------------------------------------------------------------ agents
def agent_on(cls, n_envs, T, *, streams=True, reset=False, env_seed, base=900, env_kw=None, net_seed=0, before_reset=None, **kw):
    """A primed agent on cls(n_envs, seed=env_seed): networks from torch seed `net_seed`, exploration streams from `base`;
    `before_reset(agent)` runs between enabling the streams and enabling the device reset"""
    torch.manual_seed(net_seed)
    kw.setdefault("noise_eps", 0.05)
    a = make(cls(n_envs, seed=env_seed, device=DEV, max_timesteps=T, **(env_kw or {})), T=T, **kw)
    primed(a)
    if streams:
        a.enable_explore_streams(base_seed=base)
    if before_reset:
        before_reset(a)
    if reset:
        a.vec_env.enable_device_reset(a.ctx)
    return a


def agent_pair(cls, n_envs, T, **kw):
    """Two agents built identically.  `cls` a pair of classes: one agent on each, both reset on the host; one class: (A: host reset,
    one launch per wave; B: the same with enable_device_reset())"""
    if isinstance(cls, tuple):
        return tuple(agent_on(c, n_envs, T, **kw) for c in cls)
    return tuple(agent_on(cls, n_envs, T, reset=reset, **kw) for reset in (False, True))


# ----------------------------------------------------------------------------------------------- one call on two agents
def collect_both(X, Y, **kw):
    """One collect_episodes_device call on both agents: the learner's stream untouched, episode bytes, success flags, the
    environments stepped last and the exploration streams bit for bit.  -> (episodes of Y, (flag tensors of X, of Y))"""
    flags, got = ([], []), []
    for a, f in zip((X, Y), flags):
        learner = a.rng.get_state()
        got.append(a.collect_episodes_device(success_out=f, **kw).numpy())
        if a.explore_streams is not None or not kw.get("explore", True):
            assert_states_bit_equal(a.rng.get_state(), learner, "learner stream")
    for name, x, y in zip(NAMES, *got):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), name
    fx, fy = (torch.cat([f.reshape(-1) for f in fl]) for fl in flags)
    assert fx.dtype == fy.dtype == torch.float32 and fx.shape == fy.shape and torch.equal(fx, fy)
    k = Y.vec_env.active
    assert k == X.vec_env.active
    for name in X.vec_env.state_names:
        x, y = getattr(X.vec_env, name), getattr(Y.vec_env, name)
        assert np.array_equal(bits(x[:k].cpu().numpy()), bits(y[:k].cpu().numpy())), name
    if X.explore_streams is not None:
        for i, (x, y) in enumerate(zip(X.explore_streams.get_states(), Y.explore_streams.get_states())):
            assert_states_bit_equal(x, y, ("exploration stream", i))
    return got[1], flags


def assert_forms(X, Y, form_x, form_y):
    assert X.rollout_form == form_x and Y.rollout_form == form_y, (X.rollout_form, Y.rollout_form, Y.rollout_reason)


def assert_wave_flags_equal(flags):
    """Both agents handed out one flag tensor per wave, and wave by wave they are the same"""
    assert len(flags[0]) == len(flags[1]) > 0
    for x, y in zip(*flags):
        assert x.dtype == y.dtype == torch.float32 and x.shape == y.shape and torch.equal(x, y)


def assert_whole_states_equal(X, Y):
    """Both agents reset on the host: their state tensors hold the rows of the last wave and nothing else"""
    for name in X.vec_env.state_names:
        x, y = getattr(X.vec_env, name), getattr(Y.vec_env, name)
        assert x.shape[0] == y.shape[0] and np.array_equal(bits(x.cpu().numpy()), bits(y.cpu().numpy())), name


def assert_widened_states(env, widths):
    """An environment reset on the device keeps [n_envs, width] state tensors whatever the last wave's size"""
    for name, width in zip(env.state_names, widths):
        assert tuple(getattr(env, name).shape) == (env.n_envs, width), name


def assert_reset_streams_follow_host(A, B):
    """B's reset streams against the host generators of A, which is reset on the host"""
    for i, (r, y) in enumerate(zip(A.vec_env.rs, B.vec_env.reset_streams.get_states())):
        assert_states_bit_equal(r.get_state(), y, ("reset stream", i))


# ------------------------------------------------------------------------------------------------- demonstrations, host twins
KINDS = {"point": (PointMassGoalEnv, NativePointMassVecEnv), "push": (PushBlockGoalEnv, NativePushBlockVecEnv),
         "pick": (PickPlaceGoalEnv, NativePickPlaceVecEnv)}


def twins(kind, n_envs, seed, T, **kw):
    """(host environments, the native device environment with its reset on the device), seeded alike"""
    host_cls, dev_cls = KINDS[kind]
    hosts = [host_cls(seed=seed + i, max_timesteps=T, **kw) for i in range(n_envs)]
    env = dev_cls(n_envs, seed=seed, device=DEV, max_timesteps=T, **kw)
    env.enable_device_reset(ctx())
    return hosts, env


def host_state(h):
    """The state of a host environment under the names of its device twin's `state_names`"""
    if isinstance(h, PointMassGoalEnv):
        return {"pos": h.pos, "vel": h.vel, "goal": h.goal}
    if isinstance(h, PushBlockGoalEnv):
        return {"grip": h.grip, "blk": h.blk, "goal": h.goal, "vel": np.concatenate([h.gvel, h.bvel])}
    return {"grip": h.grip, "blk": h.blk, "goal": h.goal, "aux": np.concatenate([h.gvel, h.bvel, [h.finger, h.held]])}


def assert_rows_equal(env, hosts, k, where):
    for i, h in enumerate(hosts[:k]):
        for name, v in host_state(h).items():
            assert np.array_equal(bits(getattr(env, name)[i].cpu().numpy()), bits(v)), (where, i, name)


def assert_same_as_host(hosts, env, demos, want):
    """`demos` (DeviceDemos) against `want` (scripted_demos' tuple on `hosts`); every environment ran an episode"""
    *arrays, attempted = want
    assert demos.kept == arrays[0].shape[0] == len(demos) and demos.attempted == attempted
    got = demos.numpy()
    assert len(got) == 5
    for name, x, y in zip(NAMES, got, arrays):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(bits(x), bits(y)), name
    if demos.kept:
        assert isinstance(demos.episodes, DeviceEpisodes) and len(demos.episodes) == demos.kept
        assert demos.info.dtype == torch.float32 and tuple(demos.info.shape) == arrays[4].shape
        assert np.all(got[4][:, -1] == 1.0)
    else:
        assert demos.episodes is None
    states = env.reset_streams.get_states()
    for i, h in enumerate(hosts):
        assert_states_bit_equal(h.rs.get_state(), states[i], ("reset stream", i))
    assert_rows_equal(env, hosts, len(hosts), "final state")
