"""Time per timestep of a rollout wave (ddpg_agent.collect_episodes_device, T = 100, exploring with one stream per environment) for
the push-block environment against the point mass on the same box and in the same run: the fused form with the reset on the device
(one launch: hp_rollout_waves) for both kinds, and the per-step form of the push block on its torch twin (two launches and the
twin's kernels per timestep).  One process; the cases alternate over `--rounds` rounds of `--reps` timed calls each, the device idle
(synchronised) when a timed call begins; a timestep's time is the host clock around the call + one device synchronise, over T.
Reports the median and min .. max per case, and the launch cap's budget: HP_ROLLOUT_MAX_LAUNCH_TIMESTEPS x the slowest fused
timestep of each kind against half a second.

    python tools/ubench/rollout_push_block.py --out profiles/rollout_push_block.json
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
T = 100
CASES = [("point_mass", "fused", 64), ("push_block", "fused", 64), ("point_mass", "fused", 1024), ("push_block", "fused", 1024),
         ("push_block", "stepped", 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from rl_arm_under_sparse_reward_amd import _lib
    from rl_arm_under_sparse_reward_amd.arguments import Args
    from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
    from rl_arm_under_sparse_reward_amd.device_env import NativePointMassVecEnv, NativePushBlockVecEnv, PushBlockVecEnv
    from rl_arm_under_sparse_reward_amd.random import DeviceRandomState

    assert torch.cuda.is_available(), "this measures the MI355X; there is no CPU form of it"
    ctx = _lib.Context(0)
    agents = {}
    for kind, form, n in CASES:
        torch.manual_seed(0)
        cls = NativePointMassVecEnv if kind == "point_mass" else (NativePushBlockVecEnv if form == "fused" else PushBlockVecEnv)
        env = cls(n, seed=1, device="cuda:0", max_timesteps=T)
        agent = ddpg_agent(Args(buffer_size=8 * T), env, env.env_params, ctx=ctx, rng=DeviceRandomState(1, ctx=ctx))
        rs = np.random.RandomState(0)
        agent.o_norm.update(rs.normal(0.2, 0.3, size=(400, 27))); agent.o_norm.recompute_stats()
        agent.g_norm.update(rs.normal(0.25, 0.1, size=(400, 3))); agent.g_norm.recompute_stats()
        agent.enable_explore_streams(base_seed=5)
        if form == "fused":
            env.enable_device_reset(ctx)
        for _ in range(2):                                   # warm-up: code objects, allocator
            agent.collect_episodes_device()
        torch.cuda.synchronize()
        assert agent.rollout_form == form, (agent.rollout_form, agent.rollout_reason)
        agents[(kind, form, n)] = agent
    samples = {c: [] for c in CASES}
    for _ in range(a.rounds):
        for c in CASES:                                      # alternate the cases
            for _ in range(a.reps):
                t0 = time.perf_counter()
                agents[c].collect_episodes_device()
                torch.cuda.synchronize()
                samples[c].append((time.perf_counter() - t0) * 1e6 / T)
    result = {"device": ctx.name, "T": T, "rounds": a.rounds, "reps_per_round": a.reps,
              "unit": "us per timestep of one wave: (host clock around the call + one device synchronise) / T", "cases": []}
    for c in CASES:
        v = samples[c]
        entry = {"kind": c[0], "form": c[1], "n_envs": c[2], "median": statistics.median(v), "min": min(v), "max": max(v),
                 "samples": len(v)}
        result["cases"].append(entry)
        print(f"{c[0]:10s} {c[1]:8s} n_envs {c[2]:5d}: {entry['median']:8.2f} us per timestep [{entry['min']:.2f} .. {entry['max']:.2f}]",
              flush=True)
    cap = _lib.ROLLOUT_MAX_LAUNCH_TIMESTEPS
    result["launch_cap"] = {"timesteps": cap, "budget_s": 0.5}
    for kind in ("point_mass", "push_block"):
        slowest = max(e["max"] for e in result["cases"] if e["kind"] == kind and e["form"] == "fused")
        result["launch_cap"][kind] = {"slowest_fused_timestep_us": slowest, "longest_launch_s": cap * slowest * 1e-6}
        print(f"launch cap, {kind}: {cap} x {slowest:.2f} us = {cap * slowest * 1e-6:.3f} s (budget 0.5 s)", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
