"""Helpers shared by the -m gpu parity tests (everything goes through the C ABI via ctypes)."""
import numpy as np

from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.random import DeviceRandomState
from rl_arm_under_sparse_reward_amd.replay_buffer import DeviceEpisodeBuffer

ENV_PARAMS = {"obs": 27, "goal": 3, "action": 4, "action_max": 0.5, "max_timesteps": 100}


def ctx():
    return _lib.Context.default()


def fresh_rng(seed=None):
    return DeviceRandomState(seed, ctx=ctx())


def state_equal(dev_rng, key, pos):
    st = dev_rng.get_state()
    return np.array_equal(st[1], np.asarray(key, dtype=np.uint32)) and st[2] == int(pos)


def make_shape_episodes(n_eps, obs_dim, goal_dim, act_dim, T, seed=4):
    """Random-walk episodes of any (obs, goal, action, T) shape: [obs, ag, g, actions] with the achieved goal in the first
    `goal_dim` observation columns (synthetic.make_episodes is bmirobot-shaped and needs obs >= 12 + goal)."""
    rs = np.random.RandomState(seed)
    obs = rs.uniform(-1, 1, (n_eps, T + 1, obs_dim))
    obs[:, :, :goal_dim] = rs.uniform(0, 0.5, (n_eps, 1, goal_dim)) + np.cumsum(rs.normal(0, 0.012, (n_eps, T + 1, goal_dim)), 1)
    return [obs, obs[:, :, :goal_dim].copy(), np.repeat(rs.uniform(0, 0.5, (n_eps, 1, goal_dim)), T, 1),
            rs.uniform(-0.5, 0.5, (n_eps, T, act_dim))]
