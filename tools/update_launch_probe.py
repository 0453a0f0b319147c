#!/usr/bin/env python
"""What the learner's update sequences leave behind in each launch form, as one line of sha256 per item
(profiles/update_launch_refactor.txt): two trees that print the same lines enqueue the same launches with the same arguments.

    python tools/update_launch_probe.py [--root TREE] [--only NAME]

Fixed seeds; a buffer of 32 episodes of T 50 (15 stored up front).  Every form runs in a fresh child process -- the switches are
read at hp_agent_create -- one after another, each under its own time limit; the script stops at the first child that ends
abnormally.  A form prints the launch log of its sequence (hp_agent_update_kernels), then the parameters of the four nets, Adam's
m / v / step of both optimizers, the last losses and the sampler stream's state.  The forms:

    updates    `_update_network(n)`: batch 256 x 40 (split launch + prologue), 256 x 4 (two launches), 512 and 1024 x 40 (riders
               behind the tiles, `_u` and not), 2048 x 40 (16-row slabs + dw64), 4096 x 4 (slab32); RLARM_ENGINE=layers,
               RLARM_FUSE_ADAM=0 (256 and 1024), RLARM_SPLIT=1 with one update, RLARM_DW_KSPLIT=2 at 1024,
               RLARM_ENGINE=chain_wt / chain_plain at 256 x 40
    cycle      one `train_cycle` of 4 updates at 256 (polyak folded into the last update) and one of 40 (the same behind a split
               sequence)
    minibatch  two `update_on_minibatch` calls at 256 (staged inputs: no sequence), with and without RLARM_FUSE_ADAM=0
    world1     the transports of a 1-rank group that test_rccl_path_world1_equals_single_rank_bitwise drives, three cycles of 4
               updates each, host-driven or as one graph

--root TREE imports the package from another checkout (the parent commit, built), so that one script probes both.
"""
import argparse
import hashlib
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N_EPS = 50, 32
LIMIT_S = 180       # per form: a form takes seconds; importing torch and creating the context is most of it

UPDATES = [("", 256, 40), ("", 256, 4), ("", 512, 40), ("", 1024, 40), ("", 2048, 40), ("", 4096, 4),
           ("RLARM_ENGINE=layers", 256, 4), ("RLARM_FUSE_ADAM=0", 256, 4), ("RLARM_FUSE_ADAM=0", 1024, 4), ("RLARM_SPLIT=1", 256, 1),
           ("RLARM_DW_KSPLIT=2", 1024, 4), ("RLARM_ENGINE=chain_wt", 256, 40), ("RLARM_ENGINE=chain_plain", 256, 40)]
WORLD1 = [("torch", False, "sum"), ("native", False, "sum"), ("native", True, "sum"), ("torch", False, "mean"), ("native", True, "mean"),
          ("peer", False, "sum"), ("peer", True, "sum"), ("peer", True, "mean"), ("native+dw64", True, "sum"), ("peer+dw64", True, "sum"),
          ("peer+2phase", True, "sum"), ("peer+2phase", False, "mean"), ("peer+notiles", True, "sum"), ("peer+notiles", False, "mean"),
          ("peer+split", True, "sum"), ("peer+split", False, "mean"), ("native+split", True, "sum"), ("native+split", False, "mean"),
          ("peer+notiles+split", True, "sum"), ("peer+2phase+split", True, "sum")]
# a suffix of a world-1 transport -> the switch it stands for (tests/test_gpu_update.py)
WORLD1_SWITCH = {"+split": ("RLARM_SPLIT", "1"), "+2phase": ("RLARM_PEER_PHASES", "2"), "+notiles": ("RLARM_PEER_TILES", "0"),
                 "+dw64": ("RLARM_DW64", "s3")}


def forms():
    """(name, environment switches, what the child runs)"""
    out = []
    for switch, batch, n in UPDATES:
        out.append((f"updates {switch or 'default'} batch {batch} x {n}", dict([switch.split("=")] if switch else []), ("updates", batch, n)))
    out.append(("cycle batch 256 x 4", {}, ("cycle", 256, 4)))
    out.append(("cycle batch 256 x 40", {}, ("cycle", 256, 40)))
    out.append(("minibatch batch 256", {}, ("minibatch", 256, 2)))
    out.append(("minibatch RLARM_FUSE_ADAM=0 batch 256", {"RLARM_FUSE_ADAM": "0"}, ("minibatch", 256, 2)))
    for transport, graph, reduce in WORLD1:
        env, base = {}, transport
        for suffix, (k, v) in WORLD1_SWITCH.items():
            if suffix in base:
                base = base.replace(suffix, "")
                env[k] = v
        env["RLARM_COMM"] = base
        out.append((f"world1 {transport} {'graph' if graph else 'host'} {reduce}", env, ("world1", base, int(graph), reduce)))
    return out


def sha(*arrays):
    import numpy as np
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:24]


def report(tag, agent, rng, n_losses):
    import numpy as np
    for slot, net in enumerate(("actor", "critic", "actor_target", "critic_target")):
        print(f"{tag} params {net}: {sha(agent._get_flat(slot))}")
    for slot, net in enumerate(("actor", "critic")):
        m, v, step = agent.get_adam_state(slot)
        print(f"{tag} adam {net}: m {sha(m)} v {sha(v)} step {step}")
    print(f"{tag} last_losses({n_losses}): {sha(agent.last_losses(n_losses))}")
    st = rng.get_state()
    print(f"{tag} rng.get_state: {sha(np.asarray(st[1]), np.array(st[2:], dtype=np.float64))}")


def run_form(tag, what, root):
    sys.path.insert(0, os.path.abspath(root) if root else REPO)
    import numpy as np
    import torch

    from rl_arm_under_sparse_reward_amd import _lib
    from rl_arm_under_sparse_reward_amd.arguments import Args
    from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
    from rl_arm_under_sparse_reward_amd.random import DeviceRandomState
    from rl_arm_under_sparse_reward_amd.synthetic import ENV_PARAMS, make_episodes

    kind, batch = what[0], int(what[1]) if what[0] != "world1" else 256
    env_params = dict(ENV_PARAMS, max_timesteps=T)
    ctx = _lib.Context.default()

    def make(comm=None, **kw):
        torch.manual_seed(0)
        rng = DeviceRandomState(21, ctx=ctx)
        agent = ddpg_agent(Args(batch_size=batch, buffer_size=N_EPS * T, **kw), None, env_params, rng=rng, **({"comm": comm} if comm else {}))
        agent.buffer.store_episode(make_episodes(15, seed=9, T=T, mode="walk"))
        return agent, rng

    if kind == "updates":
        n = int(what[2])
        agent, rng = make()
        agent._update_normalizer()
        k = agent.update_kernels(n)
        print(f"{tag} kernels: open {k['open']} prologue {k['prologue']} close {k['close']} updates "
              f"{[(u, sum(1 for w in k['updates'] if w == u)) for i, u in enumerate(k['updates']) if u not in k['updates'][:i]]}")
        agent._update_network(n)
        agent._update_network(n)       # a second sequence: the input sets, Q' sets and counter sets start where the first left them
        report(tag, agent, rng, min(2 * n, 8))
    elif kind == "cycle":
        n = int(what[2])
        agent, rng = make()
        for cycle in range(2):
            agent.train_cycle(make_episodes(2, seed=200 + cycle, T=T, mode="walk"), n)
        report(tag, agent, rng, min(2 * n, 8))
    elif kind == "minibatch":
        agent, rng = make()
        rs = np.random.RandomState(4)
        for _ in range(int(what[2])):
            x, xn = rs.uniform(-1, 1, (batch, 30)).astype(np.float32), rs.uniform(-1, 1, (batch, 30)).astype(np.float32)
            losses = agent.update_on_minibatch(x, xn, rs.uniform(-0.5, 0.5, (batch, 4)).astype(np.float32),
                                               -rs.randint(0, 2, batch).astype(np.float32))
            print(f"{tag} losses: {sha(np.asarray(losses, dtype=np.float64))}")
        print(f"{tag} grads: {sha(agent.get_flat_grads(0), agent.get_flat_grads(1))}")
        report(tag, agent, rng, 2)
    else:
        import socket

        import torch.distributed as dist

        from rl_arm_under_sparse_reward_amd.utils import Communicator
        transport, graph, reduce = what[1], bool(int(what[2])), what[3]
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        comm = Communicator(0, force=True)
        try:
            agent, rng = make(comm=comm, grad_reduce=reduce)
            for cycle in range(3):
                eps = make_episodes(2, seed=200 + cycle, T=T, mode="walk")
                if graph:
                    agent.train_cycle(eps, 4)
                else:
                    agent.buffer.store_episode(eps)
                    agent._update_normalizer(eps)
                    agent._update_network(4)
                    agent._soft_update_target_network()
            k = agent.update_kernels(4)
            print(f"{tag} kernels: open {k['open']} prologue {k['prologue']} close {k['close']} update {k['updates'][-1]} x {len(k['updates'])}")
            report(tag, agent, rng, 8)
            ctx.synchronize()
            torch.cuda.synchronize()
            agent.close_comm()
            del agent
        finally:
            comm.close()
            ctx.set_stream(None)
            dist.destroy_process_group()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--root", default=None)
    p.add_argument("--only", default=None, help="run the forms whose name contains this")
    p.add_argument("--form", default=None, help=argparse.SUPPRESS)      # (a child: run this one form)
    a = p.parse_args()
    if a.form is not None:
        name, what = a.form.split("|")
        run_form(name, what.split(","), a.root)
        return 0
    for name, env, what in forms():
        if a.only and a.only not in name:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--form", name + "|" + ",".join(str(w) for w in what)]
        if a.root:
            cmd += ["--root", a.root]
        sys.stdout.flush()
        try:
            rc = subprocess.run(cmd, env=dict(os.environ, **env), timeout=LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            rc = "time limit"
        if rc != 0:
            print(f"{name}: ended abnormally ({rc}); stopping")
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
