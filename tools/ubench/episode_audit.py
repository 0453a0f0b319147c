"""What an audit of recorded episodes costs: `--audit metrics` (args.eval_metrics: hp_episode_stats_block +
hp_episode_stats_summary behind the rollout), `--audit critic` (args.eval_critic: hp_episode_q_block + hp_episode_returns_block,
then hp_episode_critic_summary) or `--audit policy` (args.audit_policy: hp_episode_q_block + hp_episode_policy_block +
hp_episode_policy_stats_block, then hp_episode_policy_summary) or `--audit signal` (args.audit_actor_signal:
hp_episode_action_grad_block + hp_episode_signal_stats_block, then hp_episode_signal_summary) or `--audit bellman`
(args.audit_bellman: hp_episode_bellman_block + hp_episode_bellman_stats, then hp_episode_bellman_summary).  The block is the noise-free evaluation of 25 episodes of T = 100 on
2 native point-mass environments with the reset on the device (one rollout launch), in three forms on the same box in alternating
rounds:

    off    the collection of _eval_agent_device as it is without the option (the `eval25` / device_reset row of
           tools/ubench/rollout_device_reset.py: up to, not including, the download of the flags)
    on     the same with the audit, nothing read.  metrics: stats_out and the summary launch (two more small launches); critic:
           three more launches (Q of the 2500 steps, returns + critic columns, summary); policy: four more (Q(s, a), pi and
           Q(s, pi(s)) of the 2500 steps, the columns, the summary); signal: three more (pi, Q(s, pi(s)) and dQ/du of the 2500
           steps, the columns, the summary)
    host   the alternative the kernels replace: the collection, then DeviceEpisodes.numpy() (synchronises, four float64 arrays to
           the host) and the host twins of synthetic.  critic: clip / normalise / scale in numpy, critic_network(x, a) through
           hp_agent_critic_forward (two uploads, seven launches, a download, a wait) in front of them; policy: agent.act on the
           T + 1-strided rows (upload, one launch, download, wait) and critic_network(x, a), critic_network(x, pi); signal:
           the weights pulled to the host (state_dict), the actor and the critic in torch on the CPU, autograd for dQ/du;
           bellman: the weights of all four networks pulled to the host, the target actor and both critics in torch on the CPU
    composed   (bellman alone) what the entries that existed before compose on the device: a copy of the block's observations
           shifted by one step through episode_policy(target=True), episode_q on the block, reward and target as torch
           operations, then the columns and the summary -- no host wait, but a copy, two network launches over three passes'
           worth of input gathers, and a dozen small torch launches

Every (round, form) is a child process of its own under its own `timeout`: it warms the path up, then times `--reps` calls:
`enqueue_ms`, the host clock around the call alone, and `wall_ms`, the same + one device synchronise.  The device is idle when a
timed call begins.  The parent alternates the forms, stops at the first child that does not end cleanly, and reports the median
and min .. max over all rounds' repetitions.  No time is fixed in advance: `on` is compared with `off` of the same build in the
same run.  Not measured here: the kernels alone (they are a few microseconds inside a call of milliseconds), large n, exploring
collections (the audits' launches do not depend on them).

    python tools/ubench/episode_audit.py --audit metrics --out profiles/episode_stats.json
    python tools/ubench/episode_audit.py --audit critic --out profiles/episode_critic.json
    python tools/ubench/episode_audit.py --audit policy --out profiles/episode_policy.json
    python tools/ubench/episode_audit.py --audit signal --out profiles/episode_action_grad.json
    python tools/ubench/episode_audit.py --audit bellman --out profiles/episode_bellman.json

The signal audit's yardstick is the policy audit's forward half: record `--audit policy` of the same run on the same box beside it.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
T, N_ENVS, N_TEST = 100, 2, 25
FORMS = ("off", "on", "host")
AUDITS = {"metrics": ("EPISODE_SUMMARY", "hp_episode_stats_summary", "evaluation"),     # summary width, summary entry, the unit's noun
          "critic": ("CRITIC_STATS", "hp_episode_critic_summary", "evaluation"),
          "policy": ("POLICY_STATS", "hp_episode_policy_summary", "block"),
          "signal": ("SIGNAL_STATS", "hp_episode_signal_summary", "block"),
          "bellman": ("BELLMAN_STATS", "hp_episode_bellman_summary", "block")}
EXTRA_FORMS = {"bellman": ("composed",)}


def forms_of(audit):
    return FORMS + EXTRA_FORMS.get(audit, ())


def child(audit, form, reps):
    import numpy as np
    import torch

    from rl_arm_under_sparse_reward_amd import _lib
    from rl_arm_under_sparse_reward_amd.arguments import Args
    from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
    from rl_arm_under_sparse_reward_amd.device_env import NativePointMassVecEnv
    from rl_arm_under_sparse_reward_amd.random import DeviceRandomState
    from rl_arm_under_sparse_reward_amd import synthetic as syn

    assert torch.cuda.is_available(), "this measures the MI355X; there is no CPU form of it"
    ctx = _lib.Context(0)
    torch.manual_seed(0)
    env = NativePointMassVecEnv(N_ENVS, seed=1, device="cuda:0", max_timesteps=T)
    agent = ddpg_agent(Args(buffer_size=8 * T, n_test_rollouts=N_TEST, num_rollouts_per_mpi=2), env, env.env_params, ctx=ctx,
                       rng=DeviceRandomState(1, ctx=ctx))
    rs = np.random.RandomState(0)
    agent.o_norm.update(rs.normal(0.2, 0.3, size=(400, 27))); agent.o_norm.recompute_stats()
    agent.g_norm.update(rs.normal(0.25, 0.1, size=(400, 3))); agent.g_norm.recompute_stats()
    agent.enable_explore_streams(base_seed=5)
    env.enable_device_reset(ctx)
    width, summary_entry, _ = AUDITS[audit]
    summary = torch.empty(getattr(_lib, width), dtype=torch.float64, device="cuda:0")

    def summarise(stats):
        with ctx.torch_bridge():
            _lib.check(getattr(ctx.lib, summary_entry)(ctx.h, C.c_void_p(stats.data_ptr()), N_TEST, C.c_void_p(summary.data_ptr())))

    def work_metrics():
        flags, stats = [], ([] if form == "on" else None)
        eps = agent.collect_episodes_device(n_rollouts=N_TEST, explore=False, success_out=flags, stats_out=stats)
        if form == "on":
            summarise(stats[0])
        elif form == "host":
            _, ag, g, _ = eps.numpy()
            return syn.episode_stats_summary(syn.episode_stats(ag, g, env.distance_threshold)[0])
        return flags

    def work_critic():
        flags = []
        eps = agent.collect_episodes_device(n_rollouts=N_TEST, explore=False, success_out=flags)
        if form == "on":
            summarise(agent.episode_critic_stats(eps)[0])
        elif form == "host":
            obs, ag, g, actions = eps.numpy()
            o, gg = agent._preproc_og(obs[:, :T], g)
            x = np.concatenate([agent.o_norm.normalize(o), agent.g_norm.normalize(gg)], axis=-1).astype(np.float32).reshape(N_TEST * T, -1)
            q = agent.critic_network(x, actions.astype(np.float32).reshape(N_TEST * T, -1)).reshape(N_TEST, T)
            G = syn.episode_returns(ag, g, env.distance_threshold, agent.args.gamma, agent.args.reward_type, "persist")
            return syn.episode_critic_summary(syn.episode_critic_stats(q, G, agent.args.gamma))
        return flags

    def work_policy():
        flags = []
        eps = agent.collect_episodes_device(n_rollouts=N_TEST, explore=False, success_out=flags)
        if form == "on":
            summarise(agent.episode_policy_stats(eps)[0])
        elif form == "host":
            obs, ag, g, actions = eps.numpy()
            o, gg = agent._preproc_og(obs[:, :T], g)
            x = np.concatenate([agent.o_norm.normalize(o), agent.g_norm.normalize(gg)], axis=-1).astype(np.float32).reshape(N_TEST * T, -1)
            pi = agent.act(obs[:, :T].reshape(N_TEST * T, -1), g.reshape(N_TEST * T, -1)).astype(np.float32)
            q = agent.critic_network(x, actions.astype(np.float32).reshape(N_TEST * T, -1)).reshape(N_TEST, T)
            q_pi = agent.critic_network(x, pi).reshape(N_TEST, T)
            return syn.episode_policy_summary(syn.episode_policy_stats(pi.reshape(N_TEST, T, -1), q_pi, actions, env.env_params['action_max'], q=q))
        return flags

    def work_signal():
        flags = []
        eps = agent.collect_episodes_device(n_rollouts=N_TEST, explore=False, success_out=flags)
        if form == "on":
            summarise(agent.episode_signal_stats(eps)[0])
        elif form == "host":
            import torch.nn.functional as F
            obs, ag, g, actions = eps.numpy()
            o, gg = agent._preproc_og(obs[:, :T], g)
            x = torch.from_numpy(np.concatenate([agent.o_norm.normalize(o), agent.g_norm.normalize(gg)], axis=-1).astype(np.float32)
                                 .reshape(N_TEST * T, -1))
            pa, pc = agent.actor_network.state_dict(), agent.critic_network.state_dict()       # downloads the weights
            amax = float(env.env_params['action_max'])

            def trunk(p, h):
                for k in ("fc1", "fc2", "fc3"):
                    h = F.relu(F.linear(h, p[k + ".weight"], p[k + ".bias"]))
                return h

            with torch.no_grad():
                pi = amax * torch.tanh(F.linear(trunk(pa, x), pa["action_out.weight"], pa["action_out.bias"]))
            u = (pi / amax).requires_grad_(True)
            q = F.linear(trunk(pc, torch.cat([x, u], dim=1)), pc["q_out.weight"], pc["q_out.bias"])
            (dq_du,) = torch.autograd.grad(q.sum(), u)
            return syn.episode_signal_summary(syn.episode_signal_stats(pi.numpy().reshape(N_TEST, T, -1), dq_du.numpy().reshape(N_TEST, T, -1),
                                                                       actions, amax, action_l2=agent.args.action_l2))
        return flags

    class RawBlock:
        """A rollout block's device memory as torch sees it (no copy)"""
        def __init__(self, ptr, elems):
            self.__cuda_array_interface__ = {"shape": (int(elems),), "typestr": "<f8", "data": (int(ptr), False), "version": 2}

    def block_arrays(eps):
        """The four float64 arrays of a block as device tensors over its own memory"""
        ptr, n, offsets, elems = C.c_void_p(), C.c_int64(), (C.c_int64 * 4)(), C.c_int64()
        _lib.check(ctx.lib.hp_rollout_block(eps.h, C.byref(ptr), C.byref(n), offsets, C.byref(elems)))
        flat = torch.as_tensor(RawBlock(ptr.value, elems.value), device="cuda:0")
        d = eps.dims
        shapes = ((N_TEST, T + 1, d["obs"]), (N_TEST, T + 1, d["ag"]), (N_TEST, T, d["g"]), (N_TEST, T, d["actions"]))
        return [flat[o:o + s[0] * s[1] * s[2]].view(s) for o, s in zip(offsets, shapes)]

    def work_bellman():
        flags = []
        eps = agent.collect_episodes_device(n_rollouts=N_TEST, explore=False, success_out=flags)
        gamma32, clip32 = syn.bellman_constants(agent.args.gamma)
        if form == "on":
            summarise(agent.episode_bellman_stats(eps)[0])
        elif form == "composed":
            obs, ag, g, actions = block_arrays(eps)
            q_next = agent._policy(None, 0, N_TEST, T, True, torch.roll(obs, -1, dims=1), g)[1]
            q = agent._q(None, 0, N_TEST, T, False, obs, g, actions)
            diff = ag[:, 1:] - g
            r = -(torch.sqrt((diff * diff).sum(dim=-1)) > env.distance_threshold).to(torch.float32)
            y = torch.clamp(r + float(gamma32) * q_next, -float(clip32), 0.0)
            summarise(agent._bellman_columns(q, q_next, r, y))
        elif form == "host":
            import torch.nn.functional as F
            obs, ag, g, actions = eps.numpy()
            amax = float(env.env_params['action_max'])

            def rows(o):
                o, gg = agent._preproc_og(o, g)
                return torch.from_numpy(np.concatenate([agent.o_norm.normalize(o), agent.g_norm.normalize(gg)], axis=-1).astype(np.float32)
                                        .reshape(N_TEST * T, -1))

            def trunk(p, h):
                for k in ("fc1", "fc2", "fc3"):
                    h = F.relu(F.linear(h, p[k + ".weight"], p[k + ".bias"]))
                return h

            pa, pt, pc = (net.state_dict() for net in (agent.actor_target_network, agent.critic_target_network, agent.critic_network))
            with torch.no_grad():
                x, x_next = rows(obs[:, :T]), rows(obs[:, 1:])
                u = torch.tanh(F.linear(trunk(pa, x_next), pa["action_out.weight"], pa["action_out.bias"]))
                q_next = F.linear(trunk(pt, torch.cat([x_next, u], dim=1)), pt["q_out.weight"], pt["q_out.bias"])
                a = torch.from_numpy(actions.astype(np.float32).reshape(N_TEST * T, -1)) / np.float32(amax)
                q = F.linear(trunk(pc, torch.cat([x, a], dim=1)), pc["q_out.weight"], pc["q_out.bias"])
            q, q_next = (v.numpy().reshape(N_TEST, T) for v in (q, q_next))
            r = -(np.linalg.norm(ag[:, 1:] - g, axis=-1) > env.distance_threshold).astype(np.float32)
            y = syn.episode_bellman_targets(q_next, r, gamma32, clip32)
            return syn.episode_bellman_summary(syn.episode_bellman_stats(q, q_next, r, y, gamma32))
        return flags

    work = {"metrics": work_metrics, "critic": work_critic, "policy": work_policy, "signal": work_signal, "bellman": work_bellman}[audit]
    for _ in range(2):
        work()
    torch.cuda.synchronize()
    assert agent.rollout_form == "fused" and agent.rollout_launches == 1, (agent.rollout_form, agent.rollout_launches)
    enqueue, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        work()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        enqueue.append((t1 - t0) * 1e3)
        wall.append((t2 - t0) * 1e3)
    print("RESULT " + json.dumps({"form": form, "device": ctx.name, "enqueue_ms": enqueue, "wall_ms": wall}), flush=True)
    return 0


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "samples": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per round and form")
    ap.add_argument("--timeout", type=int, default=120, help="seconds one (round, form) child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--audit", required=True, choices=tuple(AUDITS))
    ap.add_argument("--child", default=None, choices=FORMS + tuple(f for extra in EXTRA_FORMS.values() for f in extra))
    a = ap.parse_args()
    if a.child:
        return child(a.audit, a.child, a.reps)
    forms = forms_of(a.audit)
    samples = {f: {"enqueue_ms": [], "wall_ms": []} for f in forms}
    device = None
    for r in range(a.rounds):
        for form in forms:                                   # alternate the forms
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--audit", a.audit, "--child", form,
                   "--reps", str(a.reps)]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if done.returncode != 0:
                print(f"round {r} form {form}: the child ended with status {done.returncode}; nothing further is started", flush=True)
                return 1
            rec = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            device = rec["device"]
            for key in ("enqueue_ms", "wall_ms"):
                samples[form][key] += rec[key]
            print(f"round {r} form {form}: done", flush=True)
    result = {"device": device, "T": T, "n_envs": N_ENVS, "episodes": N_TEST, "rounds": a.rounds, "reps_per_round": a.reps,
              "unit": f"ms per {AUDITS[a.audit][2]}: enqueue_ms = host clock around the call, wall_ms = the same + one device synchronise",
              "forms": {}}
    for form in forms:
        result["forms"][form] = {key: spread(samples[form][key]) for key in ("enqueue_ms", "wall_ms")}
        for key in ("enqueue_ms", "wall_ms"):
            s = result["forms"][form][key]
            print(f"{form:5s} {key:10s}: {s['median']:8.3f} ms [{s['min']:.3f} .. {s['max']:.3f}]", flush=True)
    w = {f: result["forms"][f]["wall_ms"] for f in forms}
    result["on_cheaper_than_host_beyond_spread"] = bool(w["on"]["max"] < w["host"]["min"])
    result["on_minus_off_wall_ms_median"] = w["on"]["median"] - w["off"]["median"]
    if "composed" in w:
        result["on_cheaper_than_composed_beyond_spread"] = bool(w["on"]["max"] < w["composed"]["min"])
        result["composed_minus_off_wall_ms_median"] = w["composed"]["median"] - w["off"]["median"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
