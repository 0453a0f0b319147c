#!/usr/bin/env python
"""What the episode audits that run a network over a block compute and refuse, as one line of sha256 per output tensor and one line
per refusal message (profiles/episode_nets_refactor.txt): two trees that print the same lines store the same bits and refuse the
same calls in the same words and the same order.

    python tools/episode_audit_probe.py [--root TREE]

Fixed seeds, one process.  Per act_dim (4 and 1) a freshly initialised agent and one moved off its initialisation (online actor
and critic scaled and perturbed, the targets made different by one soft update, random normalizer statistics); per agent the
shapes n x T = 3 x 5 (15 rows: a dead row in the last slab, slabs that straddle episodes), 2 x 70 (the column walk wraps past 64)
and 1 x 1; per shape clip_obs 0 (none) and 0.8 (live).  Every case runs hp_episode_q and hp_episode_policy with both `target`
values, hp_episode_action_grad with `at` 0 and 1, hp_episode_bellman under both goal modes with sparse and dense reward, and
the three column entries on what those stored -- each through the plain entry on uploaded arrays and through the *_block entry
on episodes [1, 1 + n) of a block of n + 1, whose episode 0 is other data.  Then the agent-side methods of `episode_audit` on
one case, and one call per refusal each entry can make, two arguments wrong at once among them.

--root TREE imports the package from another checkout (the parent commit, built), so that one script probes both.
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 5), (2, 70), (1, 1)]
DIMS = {4: (27, 3, 4, 0.5), 1: (29, 3, 1, 2.0)}      # act_dim -> obs, goal, act, max_action
THR = 0.05


def sha(a):
    import numpy as np
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(str((a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()[:24]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=None)
    root = ap.parse_args().root
    sys.path.insert(0, os.path.abspath(root) if root else REPO)
    import numpy as np
    import torch

    from rl_arm_under_sparse_reward_amd import _lib
    from rl_arm_under_sparse_reward_amd.arguments import Args
    from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_CRITIC, NET_CRITIC_TARGET, ddpg_agent
    from rl_arm_under_sparse_reward_amd.device_env import DeviceEpisodes, wave_layout
    from rl_arm_under_sparse_reward_amd.normalizer import normalizer
    from rl_arm_under_sparse_reward_amd.random import DeviceRandomState
    from rl_arm_under_sparse_reward_amd.replay_buffer import DeviceEpisodeBuffer

    ctx = _lib.Context.default()
    lib, dev = ctx.lib, torch.device("cuda", ctx.device_id)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    f32 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)

    def call(fn, *a):
        with ctx.torch_bridge():
            _lib.check(fn(*a))

    def make_agent(ad, moved, hidden=None):
        od, gd, _, amax = DIMS[ad]
        env = {"obs": od, "goal": gd, "action": ad, "action_max": amax, "max_timesteps": 20}
        if hidden:
            env["hidden"] = hidden
        torch.manual_seed(0)
        agent = ddpg_agent(Args(batch_size=64, buffer_size=160), None, env, ctx=ctx, rng=DeviceRandomState(5, ctx=ctx))
        if moved:
            rs = np.random.RandomState(od + ad)
            agent.o_norm.set_stats(rs.normal(0.1, 0.3, od), rs.uniform(0.2, 1.5, od).astype(np.float32))
            agent.g_norm.set_stats(rs.normal(0.2, 0.1, gd), rs.uniform(0.2, 1.5, gd).astype(np.float32))
            for net in (NET_ACTOR, NET_CRITIC):
                flat = agent._get_flat(net)
                agent._set_flat(net, flat * 1.5 + rs.normal(0, 0.01, flat.size).astype(np.float32))
            agent._soft_update_target_network()
        return agent

    def episodes(ad, n, T, seed):
        """(obs, ag, g, actions) of n + 1 episodes, float64 host arrays: episode 0 is the block's other data"""
        od, gd, _, amax = DIMS[ad]
        rs = np.random.RandomState(seed)
        obs = rs.normal(0, 1.5, (n + 1, T + 1, od))
        g = rs.normal(0, 0.04, (n + 1, T, gd))
        ag = rs.normal(0, 0.04, (n + 1, T + 1, gd))
        return obs, ag, g, rs.uniform(-amax, amax, (n + 1, T, ad))

    def block_of(ad, n, T, batch):
        """a DeviceEpisodes of n + 1 episodes holding `batch`"""
        od, gd = DIMS[ad][:2]
        shape = DeviceEpisodeBuffer(1, T, od, gd, ad, ctx=ctx)       # T and the dimensions of the block
        eps = DeviceEpisodes(ctx, shape, n + 1)
        eps.shape_of = shape
        lay = wave_layout(n + 1, T, od, gd, ad)
        flat = torch.as_tensor(_lib.DevicePointer(eps.block, lay["elems"], "<f8"), device=dev)
        for key, a in zip(("obs", "ag", "g", "actions"), batch):
            flat[lay[key]:lay[key] + a.size].copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()))
        return eps

    def pair(tag, outs, plain, plain_args, block, block_args):
        """one entry pair into fresh poisoned `outs()`: a line per output tensor of each form"""
        kept = None
        for form, fn, args in (("plain", plain, plain_args), ("block", block, block_args)):
            o = outs()
            call(fn, *args(o))
            ctx.synchronize()
            torch.cuda.synchronize()
            for name, t in o.items():
                print(f"{tag} {form} {name}: {'-' if t is None else sha(t.cpu().numpy())}")
            kept = kept or o
        return kept

    def sweep(atag, agent, ad, n, T, clip):
        tag = f"{atag} ad{ad} n{n} T{T} clip{clip:g}"
        batch = episodes(ad, n, T, seed=100 * n + T + ad)
        eps = block_of(ad, n, T, batch)
        obs, ag, g, act = (torch.from_numpy(np.ascontiguousarray(a[1:])).to(dev) for a in batch)
        amax = DIMS[ad][3]
        h = (agent.h, agent.o_norm.h, agent.g_norm.h)
        q_of = {}
        for target in (0, 1):
            net = NET_CRITIC_TARGET if target else NET_CRITIC
            q_of[target] = pair(f"{tag} q target{target}", lambda: {"q": f32(n * T + 4)},
                                lib.hp_episode_q, lambda o: (*h, net, p(obs), p(g), p(act), n, T, clip, p(o["q"])),
                                lib.hp_episode_q_block, lambda o: (eps.h, *h, net, 1, n, clip, p(o["q"])))["q"]
            o = pair(f"{tag} policy target{target}", lambda: {"pi": f32(n * T * ad + 4), "q_pi": f32(n * T + 4)},
                     lib.hp_episode_policy, lambda o: (*h, target, p(obs), p(g), n, T, clip, p(o["pi"]), p(o["q_pi"])),
                     lib.hp_episode_policy_block, lambda o: (eps.h, *h, target, 1, n, clip, p(o["pi"]), p(o["q_pi"])))
            for with_q in (True, False):
                q = q_of[target] if with_q else None
                pair(f"{tag} policy_stats target{target} q{int(with_q)}", lambda: {"stats": f64(n + 1, 6)},
                     lib.hp_episode_policy_stats,
                     lambda s: (ctx.h, p(o["pi"]), p(o["q_pi"]), p(act), p(q), n, T, ad, amax, 0.99, p(s["stats"])),
                     lib.hp_episode_policy_stats_block, lambda s: (eps.h, p(o["pi"]), p(o["q_pi"]), p(q), 1, n, amax, 0.99, p(s["stats"])))
        for at in (0, 1):
            o = pair(f"{tag} action_grad at{at}",
                     lambda: {"pi": f32(n * T * ad + 4) if at == 0 else None, "q": f32(n * T + 4), "dq_du": f32(n * T * ad + 4)},
                     lib.hp_episode_action_grad,
                     lambda o: (*h, 0, at, p(obs), p(g), p(act), n, T, clip, p(o["pi"]), p(o["q"]), p(o["dq_du"])),
                     lib.hp_episode_action_grad_block, lambda o: (eps.h, *h, 0, at, 1, n, clip, p(o["pi"]), p(o["q"]), p(o["dq_du"])))
            if at == 0:
                pair(f"{tag} signal_stats", lambda: {"stats": f64(n + 1, 6)},
                     lib.hp_episode_signal_stats,
                     lambda s: (ctx.h, p(o["pi"]), p(o["dq_du"]), p(act), n, T, ad, amax, 1.0, 1e-3, p(s["stats"])),
                     lib.hp_episode_signal_stats_block, lambda s: (eps.h, p(o["pi"]), p(o["dq_du"]), 1, n, amax, 1.0, 1e-3, p(s["stats"])))
        for mode in (0, 1):
            for kind in (0, 1):
                names = ("q", "q_next", "r", "y")
                o = pair(f"{tag} bellman goal{mode} reward{kind}", lambda: {k: f32(n * T + 4) for k in names},
                         lib.hp_episode_bellman,
                         lambda o: (*h, mode, p(obs), p(ag), p(g), p(act), n, T, THR, kind, clip, *(p(o[k]) for k in names)),
                         lib.hp_episode_bellman_block, lambda o: (eps.h, *h, mode, 1, n, THR, kind, clip, *(p(o[k]) for k in names)))
                s = f64(n + 1, 6)
                call(lib.hp_episode_bellman_stats, ctx.h, *(p(o[k]) for k in names), n, T, 0.98, p(s))
                print(f"{tag} bellman_stats goal{mode} reward{kind}: {sha(s.cpu().numpy())}")
        return batch, eps

    def methods(atag, agent, batch, eps, n):
        """the agent-side methods on the same case: the host path on episodes [1, 1 + n), the block path on the same span"""
        host = tuple(a[1:] for a in batch)
        lines = {
            "critic_stats_host": lambda: agent.episode_critic_stats_host(host, THR),
            "critic_stats": lambda: agent.episode_critic_stats(eps, distance_threshold=THR, first=1, n=n),
            "policy_stats_host": lambda: agent.episode_policy_stats_host(host, target=True),
            "policy_stats": lambda: agent.episode_policy_stats(eps, target=True, first=1, n=n),
            "signal_stats_host": lambda: agent.episode_signal_stats_host(host),
            "signal_stats": lambda: agent.episode_signal_stats(eps, first=1, n=n),
            "action_grad recorded": lambda: [v for v in agent.episode_action_grad(eps, at="recorded", first=1) if v is not None],
            "bellman_stats_host": lambda: agent.episode_bellman_stats_host(host, THR, goal="final"),
            "bellman_stats": lambda: agent.episode_bellman_stats(eps, goal="final", distance_threshold=THR, first=1, n=n),
        }
        for name, fn in lines.items():
            out = [v.cpu().numpy() if isinstance(v, torch.Tensor) else v for v in fn()]
            print(f"{atag} method {name}: {' '.join(sha(v) for v in out)}")
        agent._policy_audit_pending = agent._actor_signal_pending = agent._bellman_pending = host      # the host path of an epoch's audits
        agent.args.audit_bellman = "final"
        agent._record_policy_audit()
        agent._record_actor_signal_audit()
        agent._record_bellman_audit()
        left = (agent._policy_audit_pending, agent._actor_signal_pending, agent._bellman_pending)
        for name, onto in (("policy_audit", agent.policy_audit), ("actor_signal_audit", agent.actor_signal_audit),
                           ("bellman_audit", agent.bellman_audit)):
            print(f"{atag} method {name}: {[(k, float(v).hex()) for k, v in onto[-1].items()]} pending {all(v is None for v in left)}")

    def refusals(a):
        narrow = make_agent(4, False, hidden=128)
        small = make_agent(1, False)
        other = _lib.Context(ctx.device_id)                          # a second context on the same device
        foreign = normalizer(27, default_clip_range=5, ctx=other)
        n, T = 3, 5
        batch = episodes(4, n - 1, T, seed=7)
        eps = block_of(4, n - 1, T, batch)
        obs, ag, g, act = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in batch)
        q, qn, r, y, pi, dq = f32(n * T), f32(n * T), f32(n * T), f32(n * T), f32(n * T * 4), f32(n * T * 4)
        stats = f64(n, 6)
        h, on, gn = a.h, a.o_norm.h, a.g_norm.h
        nh, sh = (narrow.h, narrow.o_norm.h, narrow.g_norm.h), (small.h, small.o_norm.h, small.g_norm.h)

        def refuse(name, good, what, **swap):
            args = [swap.get(f"a{i}", v) for i, v in enumerate(good)]
            try:
                _lib.check(getattr(lib, name)(*args))
                print(f"refusal {name} {what}: accepted")
            except Exception as e:
                print(f"refusal {name} {what}: {type(e).__name__}: {e}")

        def shared(name, good, k_a, k_n, k_T, block):
            """what every network entry refuses; k_*: positions of the agent, n and T (T: plain entries)"""
            for i, v in enumerate(good):
                if isinstance(v, C.c_void_p) or i in (k_a, k_a + 1, k_a + 2) or (block and i == 0):
                    refuse(name, good, f"null {i}", **{f"a{i}": None})
            refuse(name, good, "foreign normalizer", **{f"a{k_a + 1}": foreign.h})
            refuse(name, good, "narrow agent", **{f"a{k_a}": nh[0], f"a{k_a + 1}": nh[1], f"a{k_a + 2}": nh[2]})
            refuse(name, good, "normalizer sizes", **{f"a{k_a + 1}": gn})
            refuse(name, good, "normalizer sizes and n 0", **{f"a{k_a + 1}": gn, f"a{k_n}": 0})
            if block:
                refuse(name, good, "block dimensions", **{f"a{k_a}": sh[0], f"a{k_a + 1}": sh[1], f"a{k_a + 2}": sh[2]})
                for first, m in ((0, 4), (2, 2), (-1, 2), (0, 0)):
                    refuse(name, good, f"range {first} {m}", **{f"a{k_n - 1}": first, f"a{k_n}": m})
                refuse(name, good, "range and narrow agent", **{f"a{k_n}": 9, f"a{k_a}": nh[0], f"a{k_a + 1}": nh[1], f"a{k_a + 2}": nh[2]})
            else:
                refuse(name, good, "n 0", **{f"a{k_n}": 0})
                refuse(name, good, "n 2^24", **{f"a{k_n}": 1 << 24})
                refuse(name, good, "T 0", **{f"a{k_T}": 0})
                refuse(name, good, "n 0 and T 0", **{f"a{k_n}": 0, f"a{k_T}": 0})
                refuse(name, good, "2^31 rows", **{f"a{k_n}": 1 << 23, f"a{k_T}": 1 << 20})

        good = [h, on, gn, NET_CRITIC, p(obs), p(g), p(act), n, T, 200.0, p(q)]
        shared("hp_episode_q", good, 0, 7, 8, False)
        for net in (NET_ACTOR, 7):
            refuse("hp_episode_q", good, f"net {net}", a3=net)
        refuse("hp_episode_q", good, "net 7 and n 0", a3=7, a7=0)
        good = [eps.h, h, on, gn, NET_CRITIC, 0, n, 200.0, p(q)]
        shared("hp_episode_q_block", good, 1, 6, None, True)
        refuse("hp_episode_q_block", good, "net 7", a4=7)

        good = [h, on, gn, 0, p(obs), p(g), n, T, 200.0, p(pi), p(q)]
        shared("hp_episode_policy", good, 0, 6, 7, False)
        refuse("hp_episode_policy", good, "target 2", a3=2)
        refuse("hp_episode_policy", good, "target 2 and narrow agent", a3=2, a0=nh[0], a1=nh[1], a2=nh[2])
        good = [eps.h, h, on, gn, 0, 0, n, 200.0, p(pi), p(q)]
        shared("hp_episode_policy_block", good, 1, 6, None, True)
        refuse("hp_episode_policy_block", good, "target -1", a4=-1)

        good = [h, on, gn, 0, 0, p(obs), p(g), p(act), n, T, 200.0, p(pi), p(q), p(dq)]
        shared("hp_episode_action_grad", good, 0, 8, 9, False)
        refuse("hp_episode_action_grad", good, "target 2", a3=2)
        refuse("hp_episode_action_grad", good, "at 2", a4=2)
        refuse("hp_episode_action_grad", good, "target 2 and at 2", a3=2, a4=2)
        refuse("hp_episode_action_grad", good, "at 1 without actions", a4=1, a7=None)
        refuse("hp_episode_action_grad", good, "at 0 without pi", a11=None)
        refuse("hp_episode_action_grad", good, "at 1 without pi", a4=1, a11=None)
        refuse("hp_episode_action_grad", good, "target 1", a3=1)
        refuse("hp_episode_action_grad", good, "target 1 and normalizer sizes", a3=1, a1=gn)
        refuse("hp_episode_action_grad", good, "target 1 and narrow agent", a3=1, a0=nh[0], a1=nh[1], a2=nh[2])
        good = [eps.h, h, on, gn, 0, 0, 0, n, 200.0, p(pi), p(q), p(dq)]
        shared("hp_episode_action_grad_block", good, 1, 7, None, True)
        refuse("hp_episode_action_grad_block", good, "at 0 without pi", a9=None)
        refuse("hp_episode_action_grad_block", good, "target 1", a4=1)
        refuse("hp_episode_action_grad_block", good, "target 1 and block dimensions", a4=1, a1=sh[0], a2=sh[1], a3=sh[2])

        good = [h, on, gn, 0, p(obs), p(ag), p(g), p(act), n, T, THR, 0, 200.0, p(q), p(qn), p(r), p(y)]
        shared("hp_episode_bellman", good, 0, 8, 9, False)
        for mode in (2, -1):
            refuse("hp_episode_bellman", good, f"goal_mode {mode}", a3=mode)
        refuse("hp_episode_bellman", good, "reward_type 2", a11=2)
        refuse("hp_episode_bellman", good, "goal_mode 5 and reward_type 2", a3=5, a11=2)
        refuse("hp_episode_bellman", good, "goal_mode 5 and n 0", a3=5, a8=0)
        good = [eps.h, h, on, gn, 0, 0, n, THR, 0, 200.0, p(q), p(qn), p(r), p(y)]
        shared("hp_episode_bellman_block", good, 1, 6, None, True)
        refuse("hp_episode_bellman_block", good, "goal_mode 7", a4=7)
        refuse("hp_episode_bellman_block", good, "reward_type -1", a8=-1)

        good = [ctx.h, p(pi), p(q), p(act), p(qn), n, T, 4, 0.5, 0.99, p(stats)]
        for i in (0, 1, 2, 3, 10):
            refuse("hp_episode_policy_stats", good, f"null {i}", **{f"a{i}": None})
        for what, swap in (("n 0", {"a5": 0}), ("T 0", {"a6": 0}), ("act_dim 0", {"a7": 0}), ("act_dim 257", {"a7": 257}),
                           ("max_action 0", {"a8": 0.0}), ("sat 2", {"a9": 2.0}), ("n 0 and sat 2", {"a5": 0, "a9": 2.0})):
            refuse("hp_episode_policy_stats", good, what, **swap)
        good = [eps.h, p(pi), p(q), p(qn), 0, n, 0.5, 0.99, p(stats)]
        for i in (0, 1, 2, 8):
            refuse("hp_episode_policy_stats_block", good, f"null {i}", **{f"a{i}": None})
        refuse("hp_episode_policy_stats_block", good, "range 2 2", a4=2, a5=2)
        refuse("hp_episode_policy_stats_block", good, "sat -1", a7=-1.0)
        good = [ctx.h, p(pi), p(dq), p(act), n, T, 4, 0.5, 1.0, 1e-3, p(stats)]
        for i in (0, 1, 2, 3, 10):
            refuse("hp_episode_signal_stats", good, f"null {i}", **{f"a{i}": None})
        for what, swap in (("n 0", {"a4": 0}), ("T 0", {"a5": 0}), ("act_dim 257", {"a6": 257}), ("max_action -1", {"a7": -1.0}),
                           ("action_l2 -1", {"a8": -1.0}), ("flat -1", {"a9": -1.0}), ("action_l2 -1 and flat -1", {"a8": -1.0, "a9": -1.0})):
            refuse("hp_episode_signal_stats", good, what, **swap)
        good = [eps.h, p(pi), p(dq), 0, n, 0.5, 1.0, 1e-3, p(stats)]
        for i in (0, 1, 2, 8):
            refuse("hp_episode_signal_stats_block", good, f"null {i}", **{f"a{i}": None})
        refuse("hp_episode_signal_stats_block", good, "range 0 4", a3=0, a4=4)
        refuse("hp_episode_signal_stats_block", good, "flat -1", a7=-1.0)
        good = [ctx.h, p(q), p(qn), p(r), p(y), n, T, 0.98, p(stats)]
        for i in (0, 1, 2, 3, 4, 8):
            refuse("hp_episode_bellman_stats", good, f"null {i}", **{f"a{i}": None})
        for what, swap in (("n 0", {"a5": 0}), ("T 0", {"a6": 0}), ("gamma 1.5", {"a7": 1.5}), ("T 0 and gamma 1.5", {"a6": 0, "a7": 1.5})):
            refuse("hp_episode_bellman_stats", good, what, **swap)
        ctx.synchronize()
        torch.cuda.synchronize()

    for ad in (4, 1):
        for moved in (False, True):
            atag = f"{'moved' if moved else 'fresh'}"
            agent = make_agent(ad, moved)
            for n, T in SHAPES:
                for clip in (0.0, 0.8):
                    batch, eps = sweep(atag, agent, ad, n, T, clip)
                    if (ad, n, clip) == (4, 3, 0.0):
                        methods(f"{atag} ad{ad} n{n} T{T}", agent, batch, eps, n)
            if ad == 4 and moved:
                refusals(agent)
    return 0


if __name__ == "__main__":
    sys.exit(main())
