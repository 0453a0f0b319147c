"""Time of a rollout call (ddpg_agent.collect_episodes_device / _eval_agent_device, T = 100) on NativePointMassVecEnv with the reset
on the host and one launch per wave (the form before device reset existed: do not enable it) against the reset on the device and
all waves in one launch (`enable_device_reset()`: hp_env_reset inside hp_rollout_waves), on the same box in alternating rounds.

Cases: the noise-free evaluation of 25 episodes on 2 environments (13 waves), an exploring wave with one stream per environment at
n_envs 2, 64 and 1024, and the rollout half of a cycle at num_rollouts_per_mpi = 2 on 2 environments (one wave, as learn() issues
it).  Every (round, form) is a child process of its own under its own `timeout`: it warms the code path up, then times `--reps`
calls per case, twice over: `enqueue_ms`, the host clock around the call alone -- how long the host is held before it can go on
enqueueing (the host reset blocks on an upload per wave; the device form should not block at all) -- and `wall_ms`, host clock
around the call + one device synchronise.  The device is idle (synchronised) when a timed call begins.  The parent alternates the
forms, stops at the first child that does not end cleanly, and reports per case and form the median and the min .. max over all
rounds' repetitions.  A form counts as faster only if its slowest sample beats the other's fastest.  RLARM_LIB selects the build.

    python tools/ubench/rollout_device_reset.py --out profiles/rollout_device_reset.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
T = 100
CASES = [("eval25", 2), ("explore", 2), ("explore", 64), ("explore", 1024), ("cycle2", 2)]
FORMS = ("host_reset", "device_reset")


def child(form, reps):
    import numpy as np
    import torch

    from rl_arm_under_sparse_reward_amd import _lib
    from rl_arm_under_sparse_reward_amd.arguments import Args
    from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
    from rl_arm_under_sparse_reward_amd.device_env import NativePointMassVecEnv
    from rl_arm_under_sparse_reward_amd.random import DeviceRandomState

    assert torch.cuda.is_available(), "this measures the MI355X; there is no CPU form of it"
    ctx = _lib.Context(0)
    out = {"form": form, "device": ctx.name, "cases": []}
    for kind, n in CASES:
        torch.manual_seed(0)
        env = NativePointMassVecEnv(n, seed=1, device="cuda:0", max_timesteps=T)
        agent = ddpg_agent(Args(buffer_size=8 * T, n_test_rollouts=25, num_rollouts_per_mpi=2), env, env.env_params, ctx=ctx,
                           rng=DeviceRandomState(1, ctx=ctx))
        rs = np.random.RandomState(0)
        agent.o_norm.update(rs.normal(0.2, 0.3, size=(400, 27))); agent.o_norm.recompute_stats()
        agent.g_norm.update(rs.normal(0.25, 0.1, size=(400, 3))); agent.g_norm.recompute_stats()
        agent.enable_explore_streams(base_seed=5)
        if form == "device_reset":
            env.enable_device_reset(ctx)
        if kind == "explore":
            work = lambda: agent.collect_episodes_device()
        elif kind == "cycle2":
            work = lambda: agent.collect_episodes_device(n_rollouts=agent.args.num_rollouts_per_mpi, epoch=0)
        else:
            # _eval_agent_device up to its download of the flags (that copy would be a synchronise inside the enqueue time)
            def work():
                flags, remaining = [], 25
                while remaining > 0:
                    k = remaining if env.reset_streams is not None else min(n, remaining)
                    agent.collect_episodes_device(n_rollouts=k, explore=False, success_out=flags)
                    remaining -= k
                return flags
        for _ in range(2):                                   # warm-up: code objects, allocator, both wave widths of eval25
            work()
        torch.cuda.synchronize()
        assert agent.rollout_form == "fused", (agent.rollout_form, agent.rollout_reason)
        launches = agent.rollout_launches
        enqueue, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            work()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            enqueue.append((t1 - t0) * 1e3)
            wall.append((t2 - t0) * 1e3)
        out["cases"].append({"case": kind, "n_envs": n, "enqueue_ms": enqueue, "wall_ms": wall, "launches_last_call": launches})
        del agent, env
    print("RESULT " + json.dumps(out), flush=True)
    return 0


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "samples": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per case, round and form")
    ap.add_argument("--timeout", type=int, default=150, help="seconds one (round, form) child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=FORMS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    samples = {(k, n, f): {"enqueue_ms": [], "wall_ms": []} for k, n in CASES for f in FORMS}
    device, launches = None, {}
    for r in range(a.rounds):
        for form in FORMS:                                   # alternate the two forms
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", form, "--reps", str(a.reps)]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if done.returncode != 0:
                print(f"round {r} form {form}: the child ended with status {done.returncode}; nothing further is started", flush=True)
                return 1
            rec = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            device = rec["device"]
            for c in rec["cases"]:
                launches[(c["case"], c["n_envs"], form)] = c["launches_last_call"]
                for key in ("enqueue_ms", "wall_ms"):
                    samples[(c["case"], c["n_envs"], form)][key] += c[key]
            print(f"round {r} form {form}: done", flush=True)
    result = {"device": device, "T": T, "rounds": a.rounds, "reps_per_round": a.reps,
              "unit": "ms per call: enqueue_ms = host clock around the call, wall_ms = the same + one device synchronise",
              "cases": []}
    for k, n in CASES:
        entry = {"case": k, "n_envs": n, "launches_last_call": {f: launches[(k, n, f)] for f in FORMS}}
        for key in ("enqueue_ms", "wall_ms"):
            h, d = spread(samples[(k, n, "host_reset")][key]), spread(samples[(k, n, "device_reset")][key])
            entry[key] = {"host_reset": h, "device_reset": d, "host_over_device": h["median"] / d["median"],
                          "device_faster_beyond_spread": bool(d["max"] < h["min"]),
                          "host_faster_beyond_spread": bool(h["max"] < d["min"])}
            print(f"{k:8s} n_envs {n:5d} {key:10s}: host reset {h['median']:8.3f} ms [{h['min']:.3f} .. {h['max']:.3f}] | "
                  f"device reset {d['median']:8.3f} ms [{d['min']:.3f} .. {d['max']:.3f}] | ratio {entry[key]['host_over_device']:.2f}",
                  flush=True)
        result["cases"].append(entry)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
