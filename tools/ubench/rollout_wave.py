"""Time of ONE whole rollout wave (ddpg_agent.collect_episodes_device, T = 100): the per-step form (PointMassVecEnv: per timestep
the policy launch, the draw + record launch and the torch kernels of the environment) against the one-launch form
(NativePointMassVecEnv: hp_rollout_episodes), on the same box in alternating rounds.

Cases: an exploring wave with one stream per environment at n_envs 2, 64 and 1024, and the noise-free evaluation of 25 episodes
(`_eval_agent_device`'s loop) on 2 and on 25 environments.  Every (round, form) is a child process of its own under its own
`timeout`: it warms both code paths up, then times `--reps` waves per case -- host clock around the call and a device synchronise
(what a training loop waits for; includes the host-side reset) and device events around the same work.  The parent alternates the
forms, stops at the first child that does not end cleanly, and reports per case and form the median and the min .. max over all
rounds' repetitions.  A form counts as faster only if its slowest sample beats the other's fastest.  RLARM_LIB selects the build.

    python tools/ubench/rollout_wave.py --out profiles/rollout_fused_wave.json
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
CASES = [("explore", 2), ("explore", 64), ("explore", 1024), ("eval25", 2), ("eval25", 25)]
FORMS = {"stepped": "PointMassVecEnv", "fused": "NativePointMassVecEnv"}


def child(form, reps):
    import numpy as np
    import torch

    from rl_arm_under_sparse_reward_amd import _lib, device_env
    from rl_arm_under_sparse_reward_amd.arguments import Args
    from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
    from rl_arm_under_sparse_reward_amd.random import DeviceRandomState

    assert torch.cuda.is_available(), "this measures the MI355X; there is no CPU form of it"
    ctx = _lib.Context(0)
    out = {"form": form, "device": ctx.name, "cases": []}
    for kind, n in CASES:
        torch.manual_seed(0)
        env = getattr(device_env, FORMS[form])(n, seed=1, device="cuda:0", max_timesteps=T)
        agent = ddpg_agent(Args(buffer_size=8 * T, n_test_rollouts=25), env, env.env_params, ctx=ctx, rng=DeviceRandomState(1, ctx=ctx))
        rs = np.random.RandomState(0)
        agent.o_norm.update(rs.normal(0.2, 0.3, size=(400, 27))); agent.o_norm.recompute_stats()
        agent.g_norm.update(rs.normal(0.25, 0.1, size=(400, 3))); agent.g_norm.recompute_stats()
        agent.enable_explore_streams(base_seed=5)
        work = (lambda: agent.collect_episodes_device()) if kind == "explore" else (lambda: agent._eval_agent_device())
        for _ in range(2):                                   # warm-up: code objects, allocator, both wave widths of eval25
            work()
        torch.cuda.synchronize()
        assert agent.rollout_form == form, (agent.rollout_form, agent.rollout_reason)
        wall, dev = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            work()
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
        out["cases"].append({"case": kind, "n_envs": n, "wall_ms": wall, "device_ms": dev})
        del agent, env
    print("RESULT " + json.dumps(out), flush=True)
    return 0


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "samples": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="timed waves per case, round and form")
    ap.add_argument("--timeout", type=int, default=150, help="seconds one (round, form) child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=sorted(FORMS))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    samples = {(k, n, f): {"wall_ms": [], "device_ms": []} for k, n in CASES for f in FORMS}
    device = None
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
                for key in ("wall_ms", "device_ms"):
                    samples[(c["case"], c["n_envs"], form)][key] += c[key]
            print(f"round {r} form {form}: done", flush=True)
    result = {"device": device, "T": T, "rounds": a.rounds, "reps_per_round": a.reps,
              "unit": "ms per wave (explore) / per 25-episode evaluation (eval25)", "cases": []}
    for k, n in CASES:
        entry = {"case": k, "n_envs": n}
        for key in ("wall_ms", "device_ms"):
            s, f = spread(samples[(k, n, "stepped")][key]), spread(samples[(k, n, "fused")][key])
            entry[key] = {"stepped": s, "fused": f, "stepped_over_fused": s["median"] / f["median"],
                          "fused_faster_beyond_spread": bool(f["max"] < s["min"]),
                          "stepped_faster_beyond_spread": bool(s["max"] < f["min"])}
        w = entry["wall_ms"]
        print(f"{k:8s} n_envs {n:5d}: stepped {w['stepped']['median']:9.3f} ms [{w['stepped']['min']:.3f} .. {w['stepped']['max']:.3f}] | "
              f"fused {w['fused']['median']:8.3f} ms [{w['fused']['min']:.3f} .. {w['fused']['max']:.3f}] | ratio {w['stepped_over_fused']:.2f} "
              f"(host clock + synchronise)", flush=True)
        result["cases"].append(entry)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
