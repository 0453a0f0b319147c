#!/usr/bin/env python
"""The bits behind every policy call, as one line of sha256 per call (profiles/policy_call_refactor.txt): two trees that print the
same lines compute the same actions and Q values.

    python tools/policy_call_probe.py [--root TREE] [--engine layers]

Fixed seeds, the default shape (27 / 3 / 4, hidden 256), primed normalizers.  On the slab engine: agent.act and act_device at rows 1,
5 and 64 (both nets, clip_obs 0 and 0.5), actor_network(x), critic_network(x, a), hp_agent_act_snapshot at rows 1, 5 and 9, one
fused rollout of two native point-mass environments (exploring, a stream per environment), and hp_episode_q_block /
hp_episode_policy_block (both parameter sets) on the block it left.  --engine layers runs the calls that exist on the layer-per-launch
engine: act, act_device, actor_network, critic_network.  --root TREE imports the package from another checkout (the parent commit,
built), so that one script probes both.
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 20


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:24]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--root", default=None)
    p.add_argument("--engine", default="", choices=["", "layers"])
    a = p.parse_args()
    sys.path.insert(0, os.path.abspath(a.root) if a.root else REPO)
    if a.engine:
        os.environ["RLARM_ENGINE"] = a.engine
    import torch

    from rl_arm_under_sparse_reward_amd import _lib
    from rl_arm_under_sparse_reward_amd.arguments import Args
    from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
    from rl_arm_under_sparse_reward_amd.device_env import NativePointMassVecEnv
    from rl_arm_under_sparse_reward_amd.random import DeviceRandomState

    ctx = _lib.Context(0)
    torch.manual_seed(0)
    env = NativePointMassVecEnv(2, seed=1, device="cuda:0", max_timesteps=T)
    agent = ddpg_agent(Args(batch_size=64, buffer_size=8 * T, num_rollouts_per_mpi=2), env, env.env_params, ctx=ctx,
                       rng=DeviceRandomState(1, ctx=ctx))
    rs = np.random.RandomState(0)
    agent.o_norm.update(rs.normal(0.2, 0.3, size=(400, 27))); agent.o_norm.recompute_stats()
    agent.g_norm.update(rs.normal(0.25, 0.1, size=(400, 3))); agent.g_norm.recompute_stats()
    tag = a.engine or "slab8"
    obs = rs.normal(0.2, 0.6, size=(64, 27)); obs[0, :3] = [40.0, -40.0, 0.2]      # past the +-5 clip
    g = rs.normal(0.25, 0.2, size=(64, 3))
    for rows in (1, 5, 64):
        o, gg = obs[:rows], g[:rows]
        ot, gt = torch.from_numpy(o).to("cuda:0"), torch.from_numpy(gg).to("cuda:0")
        for target in (False, True):
            for clip in (0.0, 0.5):
                print(f"{tag} act rows={rows} target={int(target)} clip_obs={clip}: {sha(agent.act(o, gg, target=target, clip_obs=clip))}")
                dev = agent.act_device(ot, gt, target=target, clip_obs=clip).cpu().numpy()
                print(f"{tag} act_device rows={rows} target={int(target)} clip_obs={clip}: {sha(dev)}")
    x = np.concatenate([agent.o_norm.normalize(obs), agent.g_norm.normalize(g)], axis=1).astype(np.float32)
    acts = rs.uniform(-0.5, 0.5, size=(64, 4)).astype(np.float32)
    for rows in (1, 5, 33, 64):
        print(f"{tag} actor_network rows={rows}: {sha(np.asarray(agent.actor_network(x[:rows])))}")
        print(f"{tag} actor_target_network rows={rows}: {sha(np.asarray(agent.actor_target_network(x[:rows])))}")
        print(f"{tag} critic_network rows={rows}: {sha(np.asarray(agent.critic_network(x[:rows], acts[:rows])))}")
        print(f"{tag} critic_target_network rows={rows}: {sha(np.asarray(agent.critic_target_network(x[:rows], acts[:rows])))}")
    if a.engine:
        return
    agent.policy_snapshot()
    for rows in (1, 5, 9):
        for clip in (0.0, 0.5):
            out = np.empty((rows, 4), np.float32)
            _lib.check(agent.lib.hp_agent_act_snapshot(agent.h, _lib.ptr(obs, C.c_double), _lib.ptr(g, C.c_double), rows, clip,
                                                       _lib.ptr(out, C.c_float)))
            print(f"{tag} act_snapshot rows={rows} clip_obs={clip}: {sha(out)}")
    agent.enable_explore_streams(base_seed=5)
    eps = agent.collect_episodes_device(n_rollouts=2, explore=True)
    assert agent.rollout_form == "fused", (agent.rollout_form, agent.rollout_reason)
    print(f"{tag} fused rollout 2 x T={T}: {sha(*eps.numpy())}")
    for target in (False, True):
        print(f"{tag} episode_q target={int(target)}: {sha(agent.episode_q(eps, target=target).cpu().numpy())}")
        pi, q_pi = agent.episode_policy(eps, target=target)
        print(f"{tag} episode_policy target={int(target)}: {sha(pi.cpu().numpy(), q_pi.cpu().numpy())}")


if __name__ == "__main__":
    main()
