"""Device time of ONE exploring rollout step (csrc/rollout.hip): the single shared stream (hp_rollout_step: one wave walks the
environments in turn) against one stream per environment (hp_rollout_step_streams: one wave per environment), by n_envs, with the
policy launch excluded (teacher-forced form: the draw + record launch alone) and included.

Each figure is the time between two device events around `--steps` steps enqueued back to back, divided by the steps; the two
forms alternate, `--rounds` times each, after a warm-up of both, and the spread reported is min .. max over the rounds.  The new
form counts as faster at a width only if its slowest round beats the single stream's fastest.  RLARM_LIB selects the build.

    python tools/ubench/explore_step.py --out profiles/explore_step_streams.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
from rl_arm_under_sparse_reward_amd.device_env import DeviceEpisodes, binomial1_qn
from rl_arm_under_sparse_reward_amd.random import DeviceRandomState, DeviceRandomStreams

OBS, GOAL, ACT, T = 27, 3, 4, 100            # the reference's dims


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", default="1,64,1024,4096")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=0, help="steps per timed window (0: 400 up to 64 envs, 100 up to 1024, 40 beyond)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the MI355X; there is no CPU form of it"
    ctx = _lib.Context(0)
    lib = ctx.lib
    torch.manual_seed(0)
    params = {"obs": OBS, "goal": GOAL, "action": ACT, "action_max": 0.5, "max_timesteps": T}
    agent = ddpg_agent(Args(buffer_size=8 * T), None, params, ctx=ctx, rng=DeviceRandomState(1, ctx=ctx))
    rs = np.random.RandomState(0)
    agent.o_norm.update(rs.normal(0.2, 0.3, size=(400, OBS))); agent.o_norm.recompute_stats()
    agent.g_norm.update(rs.normal(0.25, 0.1, size=(400, GOAL))); agent.g_norm.recompute_stats()
    noise_eps, random_eps = 0.2, 0.3
    qn = binomial1_qn(random_eps)[0]
    p = lambda t: C.c_void_p(t.data_ptr())
    result = {"device": ctx.name, "dims": [OBS, GOAL, ACT], "rounds": a.rounds, "unit": "us per step (device events)", "widths": []}
    for n in [int(x) for x in a.n_envs.split(",")]:
        steps = a.steps or (400 if n <= 64 else 100 if n <= 1024 else 40)
        eps = DeviceEpisodes(ctx, agent.buffer._dev, n)
        _lib.check(lib.hp_rollout_set_action_max(eps.h, 0.5))
        single = DeviceRandomState(7, ctx=ctx)
        streams = DeviceRandomStreams(n, base_seed=7, ctx=ctx)
        o, ag, g = (torch.from_numpy(rs.uniform(-1, 1, (n, d))).to("cuda:0") for d in (OBS, GOAL, GOAL))
        act = torch.from_numpy(rs.uniform(-0.5, 0.5, (n, ACT)).astype(np.float32)).to("cuda:0")
        forms = {"single_stream": (lib.hp_rollout_step, single.h), "per_env_streams": (lib.hp_rollout_step_streams, streams.h)}

        def window(form, with_policy, k):
            fn, h = forms[form]
            handles = (agent.h, agent.o_norm.h, agent.g_norm.h) if with_policy else (None, None, None)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with ctx.torch_bridge():
                e0.record()
                for i in range(k):
                    _lib.check(fn(eps.h, *handles, h, i % T, p(o), p(ag), p(g), 1, noise_eps, random_eps, qn, 0.0, p(act)))
                e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / k

        entry = {"n_envs": n, "steps_per_window": steps}
        for with_policy in (False, True):
            for form in forms:
                window(form, with_policy, max(8, steps // 4))                       # warm-up: code objects, both shapes
            times = {form: [] for form in forms}
            for _ in range(a.rounds):
                for form in forms:                                                     # alternate the two forms
                    times[form].append(window(form, with_policy, steps))
            rec = {form: {"median": statistics.median(v), "min": min(v), "max": max(v)} for form, v in times.items()}
            s, e = rec["single_stream"], rec["per_env_streams"]
            rec["single_over_streams"] = s["median"] / e["median"]
            rec["streams_faster_beyond_spread"] = bool(e["max"] < s["min"])
            rec["single_faster_beyond_spread"] = bool(s["max"] < e["min"])
            entry["policy_included" if with_policy else "policy_excluded"] = rec
            print(f"n_envs {n:5d} policy {'included' if with_policy else 'excluded'}: single stream {s['median']:9.2f} us "
                  f"[{s['min']:.2f} .. {s['max']:.2f}] | per-env streams {e['median']:8.2f} us [{e['min']:.2f} .. {e['max']:.2f}] | "
                  f"ratio {rec['single_over_streams']:.2f}", flush=True)
        result["widths"].append(entry)
        del eps, streams, single
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
