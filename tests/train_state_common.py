"""Helpers shared by the -m gpu training-state tests: a learner without an environment, the cycles it trains on, and a fingerprint
of every piece of its state."""
import numpy as np
import torch

from gpu_common import ENV_PARAMS, fresh_rng, make_shape_episodes
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_ACTOR_TARGET, NET_CRITIC, NET_CRITIC_TARGET, ddpg_agent
from rl_arm_under_sparse_reward_amd.synthetic import make_episodes

N_BATCHES = 14          # >= 12 updates per sequence: batch 256 takes the split launch
EPS_PER_CYCLE = 2


def build(batch=256, ep=None, cap_eps=40, torch_seed=0, rng_seed=7, f32=False, n_batches=N_BATCHES):
    ep = dict(ep or ENV_PARAMS)
    args = Args(batch_size=batch, buffer_size=cap_eps * ep["max_timesteps"], n_batches=n_batches)
    torch.manual_seed(torch_seed)
    agent = ddpg_agent(args, None, ep, rng=fresh_rng(rng_seed))
    if f32:
        agent.buffer.enable_f32_rows()
    return agent


def episodes(ep, i):
    if ep is None or (ep["obs"], ep["goal"], ep["action"], ep["max_timesteps"]) == (27, 3, 4, 100):
        return make_episodes(EPS_PER_CYCLE, seed=100 + i, mode="walk")
    return make_shape_episodes(EPS_PER_CYCLE, ep["obs"], ep["goal"], ep["action"], ep["max_timesteps"], seed=100 + i)


def cycles(agent, ep, first, n):
    for i in range(first, first + n):
        agent.train_cycle(episodes(ep, i))


def fingerprint(agent):
    """Every piece of learner state, as host arrays."""
    fp = {}
    for name, slot in (("actor", NET_ACTOR), ("critic", NET_CRITIC), ("actor_target", NET_ACTOR_TARGET),
                       ("critic_target", NET_CRITIC_TARGET)):
        fp[name] = agent._get_flat(slot)
    for name, slot in (("actor", NET_ACTOR), ("critic", NET_CRITIC)):
        m, v, step = agent.get_adam_state(slot)
        fp[f"adam_{name}_m"], fp[f"adam_{name}_v"], fp[f"adam_{name}_step"] = m, v, np.array([step])
    for pre, nz in (("o_norm", agent.o_norm), ("g_norm", agent.g_norm)):
        for k, v in nz._get().items():
            fp[f"{pre}_{k}"] = v
    st = agent.rng.get_state()
    fp["rng_key"], fp["rng_pos"] = st[1], np.array([st[2]])
    _, cs, nts, _ = agent.buffer._dev.info()
    fp["buffer_counters"] = np.array([cs, nts])
    for k in ("obs", "ag", "g", "actions"):
        fp[f"buffer_{k}"] = agent.buffer._dev.read(k, 0, cs) if cs else np.empty(0)
    return fp


def assert_same(a, b, what=""):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)
