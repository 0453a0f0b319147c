#!/usr/bin/env python
"""What learn() leaves behind on each of its paths, as one line of sha256 per item (profiles/agent_loop_refactor.txt): two trees that
print the same lines run the same epochs, cycles, rollouts, evaluations, audits and saves.

    python tools/agent_loop_probe.py [--root TREE]

Fixed seeds; batch 64, T 20, 2 epochs of 2 cycles of 2 updates, 3 rollouts per cycle, 3 test rollouts; eval_metrics, eval_critic,
audit_policy, audit_actor_signal on; a training state after every epoch with state_full_every 2 (one full state, one delta).  Three
runs of learn(): `host` on a list of two PointMassGoalEnv (the last wave of three episodes is short), `device` on a
NativePointMassVecEnv(2), `device+reset+streams` the same with device_reset and explore_streams.  Each run prints success_rates, the
four audit lists, the parameters of the four nets, both normalizers, the device stream's and numpy's state, the buffer, the arrays
of the saved state files and what the run printed (without the elapsed times and the date).  After them, on the host agent:
collect_episodes(3, epoch=100), collect_episodes(3, explore=False) and _eval_agent().  --root TREE imports the package from another
checkout (the parent commit, built), so that one script probes both.
"""
import argparse
import contextlib
import hashlib
import io
import json
import os
import sys
import tempfile

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


def sha_text(text):
    return hashlib.sha256(text.encode()).hexdigest()[:24]


def stream_arrays(state):
    """A RandomState's get_state() tuple as arrays"""
    return [np.asarray(state[1]), np.array(state[2:], dtype=np.float64)]


def printed_lines(text):
    """What a run printed, without the elapsed-time lines (a bare float) and the date in front of an epoch's line"""
    keep = []
    for line in text.splitlines():
        try:
            float(line)
        except ValueError:
            keep.append(line.split("] ", 1)[-1] if line.startswith("[") else line)
    return "\n".join(keep)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--root", default=None)
    a = p.parse_args()
    sys.path.insert(0, os.path.abspath(a.root) if a.root else REPO)
    import torch

    from rl_arm_under_sparse_reward_amd import _lib
    from rl_arm_under_sparse_reward_amd.arguments import Args
    from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
    from rl_arm_under_sparse_reward_amd.device_env import NativePointMassVecEnv
    from rl_arm_under_sparse_reward_amd.random import DeviceRandomState
    from rl_arm_under_sparse_reward_amd.synthetic import PointMassGoalEnv

    ctx = _lib.Context(0)
    host_agent = None
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)       # relative names below: whatever a state file records of its own name is the same in every run
        for tag, extra in (("host", None), ("device", {}), ("device+reset+streams", dict(device_reset=True, explore_streams=True))):
            where = tag
            os.makedirs(where)
            args = Args(batch_size=64, buffer_size=40 * T, n_epochs=2, n_cycles=2, n_batches=2, n_test_rollouts=3, num_rollouts_per_mpi=3,
                        eval_metrics=True, eval_critic=True, audit_policy=True, audit_actor_signal=True, state_full_every=2,
                        save_dir=where, env_name="probe", **(extra or {}))
            args.state_path = os.path.join(where, "state.npz")
            np.random.seed(11)
            torch.manual_seed(0)
            if extra is None:
                env = [PointMassGoalEnv(seed=3 + i, max_timesteps=T) for i in range(2)]
                env_params = env[0].env_params
            else:
                env = NativePointMassVecEnv(2, seed=3, device="cuda:0", max_timesteps=T)
                env_params = env.env_params
            agent = ddpg_agent(args, env, env_params, ctx=ctx, rng=DeviceRandomState(5, ctx=ctx))
            out = io.StringIO()
            with contextlib.redirect_stdout(out):
                agent.learn()
            print(f"{tag} success_rates: {sha(np.array(agent.success_rates))}")
            for name in ("eval_metrics", "eval_critic", "policy_audit", "actor_signal_audit"):
                rows = getattr(agent, name)
                print(f"{tag} {name} x {len(rows)}: {sha_text(json.dumps([sorted((k, repr(v)) for k, v in r.items()) for r in rows]))}")
            for slot, net in enumerate(("actor", "critic", "actor_target", "critic_target")):
                print(f"{tag} params {net}: {sha(agent._get_flat(slot))}")
            print(f"{tag} normalizers: {sha(agent.o_norm.mean, agent.o_norm.std, agent.g_norm.mean, agent.g_norm.std)}")
            print(f"{tag} rng.get_state: {sha(*stream_arrays(agent.rng.get_state()))}")
            print(f"{tag} np.random.get_state: {sha(*stream_arrays(np.random.get_state()))}")
            keys = sorted(agent.buffer.buffers.keys())
            print(f"{tag} buffer {keys} current_size={agent.buffer.current_size}: {sha(*(agent.buffer.buffers[k] for k in keys))}")
            for name in sorted(f for f in os.listdir(where) if f.endswith(".npz")):
                with np.load(os.path.join(where, name), allow_pickle=False) as z:
                    print(f"{tag} state file {name} ({len(z.files)} arrays): {sha(*(z[k] for k in sorted(z.files)))}")
            print(f"{tag} printed: {sha_text(printed_lines(out.getvalue()))}")
            if extra is None:
                host_agent = agent
        np.random.seed(12)
        print(f"host collect_episodes(3, epoch=100): {sha(*host_agent.collect_episodes(3, epoch=100))}")
        print(f"host collect_episodes(3, explore=False): {sha(*host_agent.collect_episodes(3, explore=False))}")
        print(f"host np.random after them: {sha(*stream_arrays(np.random.get_state()))}")
        n = [len(host_agent.eval_metrics), len(host_agent.eval_critic)]
        rate = host_agent._eval_agent()
        rows = host_agent.eval_metrics[n[0]:] + host_agent.eval_critic[n[1]:]
        print(f"host _eval_agent: {sha(np.array([rate]))} {sha_text(json.dumps([sorted((k, repr(v)) for k, v in r.items()) for r in rows]))}")


if __name__ == "__main__":
    main()
