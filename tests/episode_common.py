"""Helpers shared by the -m gpu episode-audit tests (stats, critic, policy, actor signal, Bellman): the learner their learn() tests
run, the oracle's forward passes on rows prepared in numpy, the raw entries on uploaded arrays, and agents moved off their
initialisation."""
import os

import numpy as np
import pytest
import torch

from gpu_common import fresh_rng
from oracle import ddpg_update as oupd
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_ACTOR_TARGET, NET_CRITIC, NET_CRITIC_TARGET, ddpg_agent
from rl_arm_under_sparse_reward_amd.device_env import NativePointMassVecEnv
from rollout_common import DEV, dev_ptr as p, make, primed


def learner(tmp_path, name, reset, state_path=None, **kw):
    torch.manual_seed(0)
    np.random.seed(11)
    env = NativePointMassVecEnv(2, seed=10, device=DEV, max_timesteps=10, distance_threshold=0.15)
    a = make(env, T=10, seed=5, n_epochs=2, n_cycles=2, n_batches=2, n_test_rollouts=5, buffer_episodes=40, noise_eps=0.05,
             explore_streams=True, device_reset=reset, save_dir=str(tmp_path / name), env_name="pm", **kw)
    a.args.state_path = state_path
    primed(a)
    return a


def tree_bytes(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f), "rb").read()
    return out


def refused(status, text, code=-1):
    assert status == code, status
    with pytest.raises(ValueError if code == -1 else _lib.HpError, match=text):
        _lib.check(status)


# ------------------------------------------------------------------------------------------ the critic
def oracle_q(agent, obs, g, actions, target=False):
    """The oracle's critic on rows prepared in numpy from the agent's CURRENT parameters (hp_agent_get_params) and normalizer
    statistics (hp_norm_get): [n, T]"""
    n, T = g.shape[:2]
    co, cr = float(agent.args.clip_obs), float(agent.args.clip_range)
    parts = []
    for raw, nz in ((obs[:, :T], agent.o_norm), (g, agent.g_norm)):
        v = np.clip(np.asarray(raw, dtype=np.float64), -co, co)
        v = (v - nz.mean.astype(np.float64)) / nz.std.astype(np.float64)
        parts.append(np.clip(v, -cr, cr).astype(np.float32))
    x = np.concatenate(parts, axis=-1).reshape(n * T, -1)
    a = np.asarray(actions, dtype=np.float64).astype(np.float32).reshape(n * T, -1)
    net = agent.critic_target_network if target else agent.critic_network
    params = {k: v.detach().clone() for k, v in net.state_dict().items()}
    want = oupd.critic_forward(params, torch.from_numpy(x), torch.from_numpy(a), float(agent.env_params['action_max']))
    return want.numpy().reshape(n, T), x, a


def raw_q(agent, obs, g, actions, target=False):
    """hp_episode_q on uploaded arrays, into a poisoned tensor, in torch's stream order"""
    o, gg, a = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(DEV) for v in (obs, g, actions))
    n, T = g.shape[:2]
    q = torch.full((n, T), float("nan"), dtype=torch.float32, device=DEV)
    with agent.ctx.torch_bridge():
        _lib.check(agent.lib.hp_episode_q(agent.h, agent.o_norm.h, agent.g_norm.h, NET_CRITIC_TARGET if target else NET_CRITIC, p(o), p(gg),
                                          p(a), n, T, float(agent.args.clip_obs), p(q)))
    return q.cpu().numpy()


def shaped_agent(obs_dim, goal_dim, act_dim, amax, batch=64, T=20, **kw):
    """An agent of another shape with random statistics, an online critic moved away from its initialisation and a target made
    different from it by one soft update"""
    env = {"obs": obs_dim, "goal": goal_dim, "action": act_dim, "action_max": amax, "max_timesteps": T}
    torch.manual_seed(0)
    agent = ddpg_agent(Args(batch_size=batch, buffer_size=8 * T, **kw), None, env, rng=fresh_rng(5))
    rs = np.random.RandomState(obs_dim)
    agent.o_norm.set_stats(rs.normal(0.1, 0.3, obs_dim), rs.uniform(0.2, 1.5, obs_dim).astype(np.float32))
    agent.g_norm.set_stats(rs.normal(0.2, 0.1, goal_dim), rs.uniform(0.2, 1.5, goal_dim).astype(np.float32))
    flat = agent._get_flat(NET_CRITIC)
    agent._set_flat(NET_CRITIC, flat * 1.5 + rs.normal(0, 0.01, flat.size).astype(np.float32))
    agent._soft_update_target_network()
    assert not np.array_equal(agent._get_flat(NET_CRITIC), agent._get_flat(NET_CRITIC_TARGET))
    assert not np.array_equal(agent._get_flat(NET_CRITIC_TARGET), flat)
    return agent


# ------------------------------------------------------------------------------------------ the actor
def oracle_policy(agent, obs, g, target=False):
    """The oracle's actor, and its critic on that action, on rows prepared in numpy from the agent's CURRENT parameters
    (hp_agent_get_params) and normalizer statistics: (pi [n, T, act], q_pi [n, T])"""
    n, T = g.shape[:2]
    amax = float(agent.env_params['action_max'])
    _, x, _ = oracle_q(agent, obs, g, np.zeros((n, T, int(agent.env_params['action']))), target)
    actor = agent.actor_target_network if target else agent.actor_network
    critic = agent.critic_target_network if target else agent.critic_network
    pa = {k: v.detach().clone() for k, v in actor.state_dict().items()}
    pc = {k: v.detach().clone() for k, v in critic.state_dict().items()}
    xt = torch.from_numpy(x)
    pi = oupd.actor_forward(pa, xt, amax)
    q_pi = oupd.critic_forward(pc, xt, pi, amax)
    return pi.numpy().reshape(n, T, -1), q_pi.numpy().reshape(n, T), x


def raw_policy(agent, obs, g, target=False):
    """hp_episode_policy on uploaded arrays, into poisoned tensors, in torch's stream order"""
    o, gg = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(DEV) for v in (obs, g))
    n, T = g.shape[:2]
    pi = torch.full((n, T, int(agent.env_params['action'])), float("nan"), dtype=torch.float32, device=DEV)
    q_pi = torch.full((n, T), float("nan"), dtype=torch.float32, device=DEV)
    with agent.ctx.torch_bridge():
        _lib.check(agent.lib.hp_episode_policy(agent.h, agent.o_norm.h, agent.g_norm.h, 1 if target else 0, p(o), p(gg), n, T,
                                               float(agent.args.clip_obs), p(pi), p(q_pi)))
    return pi.cpu().numpy(), q_pi.cpu().numpy()


def move_actor(agent, seed):
    """An online actor moved away from its initialisation (far enough that some tanh saturate) and a target actor made different
    from it by one soft update"""
    rs = np.random.RandomState(seed)
    flat = agent._get_flat(NET_ACTOR)
    agent._set_flat(NET_ACTOR, flat * 1.5 + rs.normal(0, 0.01, flat.size).astype(np.float32))
    agent._soft_update_target_network()
    assert not np.array_equal(agent._get_flat(NET_ACTOR), agent._get_flat(NET_ACTOR_TARGET))
    assert not np.array_equal(agent._get_flat(NET_CRITIC), agent._get_flat(NET_CRITIC_TARGET))
    return agent
