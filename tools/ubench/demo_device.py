"""Time of generating 1000 scripted demonstrations on `NativePushBlockVecEnv` (T = 100, the reference's schedule): the device
form (device_env.generate_demos: hp_demo_episodes + hp_demo_compact per round, one 4-byte read per round) against the host
generator (synthetic.scripted_demos on host twins seeded alike) on the same box, at n_envs 64 and 1024.

Every (round, form) is a child process of its own under its own `timeout`; the parent alternates the forms, stops at the first
child that does not end cleanly, and reports per case and form the median and the min .. max over the rounds, with the episodes
attempted and -- device form -- the launches.  The device child generates once untimed first (code objects, allocator) on an
environment of its own, then times one whole call on a fresh environment: host clock around the call, which ends with the last
round's synchronising read.  The host child times one whole call.  Both forms return the same bits (tests/test_gpu_scripted_demos.py);
the comparison is with the host generator on this box, never with the kernel itself.  RLARM_LIB selects the build.

    python tools/ubench/demo_device.py --out profiles/demo_device.json
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
T, N_DEMOS, SEED = 100, 1000, 0
CASES = [64, 1024]
FORMS = ("device", "host")


def child(form, n_envs):
    from rl_arm_under_sparse_reward_amd import device_env
    from rl_arm_under_sparse_reward_amd.synthetic import PushBlockGoalEnv, scripted_demos

    waves = device_env.default_round_waves(N_DEMOS, n_envs)
    out = {"form": form, "n_envs": n_envs, "round_waves": waves}
    if form == "host":
        envs = [PushBlockGoalEnv(seed=SEED + i, max_timesteps=T) for i in range(n_envs)]
        t0 = time.perf_counter()
        *arrays, attempted = scripted_demos(envs, N_DEMOS, waves)
        out.update(ms=(time.perf_counter() - t0) * 1e3, kept=int(arrays[0].shape[0]), attempted=int(attempted))
    else:
        import torch

        from rl_arm_under_sparse_reward_amd import _lib

        assert torch.cuda.is_available(), "this measures the MI355X; there is no CPU form of it"
        ctx = _lib.Context(0)
        out["device"] = ctx.name

        def fresh():
            env = device_env.NativePushBlockVecEnv(n_envs, seed=SEED, device="cuda:0", max_timesteps=T)
            env.enable_device_reset(ctx)
            return env

        device_env.generate_demos(fresh(), N_DEMOS, ctx=ctx)      # warm-up
        env = fresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        demos = device_env.generate_demos(env, N_DEMOS, ctx=ctx)
        torch.cuda.synchronize()
        out.update(ms=(time.perf_counter() - t0) * 1e3, kept=demos.kept, attempted=demos.attempted, launches=demos.launches)
    print("RESULT " + json.dumps(out), flush=True)
    return 0


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "samples": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=400, help="seconds one (round, form, n_envs) child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=FORMS)
    ap.add_argument("--n-envs", type=int, default=CASES[0])
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.n_envs)
    recs = {(n, f): [] for n in CASES for f in FORMS}
    device = None
    for r in range(a.rounds):
        for n in CASES:
            for form in FORMS:                                   # alternate the two forms
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", form, "--n-envs", str(n)]
                done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                if done.returncode != 0:
                    print(f"round {r} n_envs {n} form {form}: the child ended with status {done.returncode}; nothing further is started",
                          flush=True)
                    return 1
                rec = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
                device = rec.get("device", device)
                recs[(n, form)].append(rec)
                print(f"round {r} n_envs {n} form {form}: {rec['ms']:.1f} ms, kept {rec['kept']} of {rec['attempted']}", flush=True)
    result = {"device": device, "T": T, "n_demos": N_DEMOS, "rounds": a.rounds, "unit": "ms per generate_demos / scripted_demos call",
              "cases": []}
    for n in CASES:
        d, h = recs[(n, "device")], recs[(n, "host")]
        assert {(x["kept"], x["attempted"]) for x in d} == {(x["kept"], x["attempted"]) for x in h}, "the two forms disagree"
        sd, sh = spread([x["ms"] for x in d]), spread([x["ms"] for x in h])
        entry = {"n_envs": n, "round_waves": d[0]["round_waves"], "kept": d[0]["kept"], "attempted": d[0]["attempted"],
                 "launches": d[0]["launches"], "device_ms": sd, "host_ms": sh, "host_over_device": sh["median"] / sd["median"],
                 "device_faster_beyond_spread": bool(sd["max"] < sh["min"])}
        print(f"n_envs {n:5d}: device {sd['median']:9.2f} ms [{sd['min']:.2f} .. {sd['max']:.2f}] | host {sh['median']:10.1f} ms "
              f"[{sh['min']:.1f} .. {sh['max']:.1f}] | ratio {entry['host_over_device']:.0f} | attempted {entry['attempted']}, "
              f"launches {entry['launches']}", flush=True)
        result["cases"].append(entry)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
