"""Store policy of the chains' outputs (csrc/slab8.h, "store policy"): the default build of an agent -- ordinary stores for every
actor-side output of the split launch, published by the kernel boundary -- against the same agent with RLARM_ENGINE=chain_wt, which
stores them write-through as before (a value of the engine switch: DESIGN.md section 4 keeps its list of switch NAMES at 15, which
tests/test_abi.py holds it to).  The switch is read by hp_agent_create, so each policy runs in a fresh child process
(this file, run as a script); the children share nothing but their inputs.

Every case runs four sequences of 12 updates back to back (12 = SPLIT_MIN_UPDATES, the shortest sequence that takes the split
launch) with RLARM_KEEP_GRADS=1 and compares, after EVERY sequence and bit for bit: the kept actor and critic gradients, all four
parameter vectors, Adam m / v of both networks and the loss log.  A publication the consumer launch does not see shows as stale
operands of the actor's weight-gradient tiles, i.e. other bits in the actor's gradients from the first sequence on.

Cases (the launches each one takes are asserted from the library's own launch log):
  batch 4     rows are padded to 32, below the 64 the in-launch tiles need: the sequence takes k_fb_slab8 + k_gemm_lds_adam
  batch 36    64 padded rows, 16 chains per role: k_fb_split8<0>, chains wrap past one per XCD of their half
  batch 256   k_fb_split8<0> with all 64 actor-side chains resident at once on XCDs 0-3
  batch 36 through k_fb_split8<2> (one-rank RCCL group, RLARM_COMM=native as tests/test_gpu_update.py sets it up)
  batch 36 with RLARM_SPLIT=0: k_fb_slab8
k_fb_slab8 stores write-through by default, so in the cases that run it the default build and RLARM_ENGINE=chain_wt are the same
code; there the first child runs RLARM_ENGINE=chain_plain, the ordinary-store instantiation of that kernel."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_UPDATES, N_SEQ = 12, 4
# name: (batch, extra environment, world-1 RCCL group, kernels of one update)
CASES = {
    "b4": (4, {}, False, ["k_fb_slab8", "k_gemm_lds_adam"]),
    "b36": (36, {}, False, ["k_fb_split8<0>", "k_gemm_lds_adam"]),
    "b256": (256, {}, False, ["k_fb_split8<0>", "k_gemm_lds_adam"]),
    "b36_rccl": (36, {"RLARM_COMM": "native"}, True, ["k_fb_split8<2>", "k_gemm_lds", "rccl:ncclAllReduce", "k_adam_frag4"]),
    "b36_slab8": (36, {"RLARM_SPLIT": "0"}, False, ["k_fb_slab8", "k_gemm_lds_adam"]),
}
SWITCHES = ("RLARM_ENGINE", "RLARM_SPLIT", "RLARM_COMM", "RLARM_KEEP_GRADS")


def _child(policy, out_path):
    """policy: 'default' | 'wt'.  Writes every compared array of every case into one .npz and the launch logs beside it."""
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    from gpu_common import ENV_PARAMS, fresh_rng
    from rl_arm_under_sparse_reward_amd import _lib
    from rl_arm_under_sparse_reward_amd.arguments import Args
    from rl_arm_under_sparse_reward_amd.ddpg_agent import (NET_ACTOR, NET_ACTOR_TARGET, NET_CRITIC, NET_CRITIC_TARGET,
                                                            ddpg_agent)
    from rl_arm_under_sparse_reward_amd.synthetic import make_episodes

    out, logs = {}, {}
    eps = make_episodes(8, seed=9, mode="walk")      # one set of inputs for every case

    def sequences(name, agent):
        agent.buffer.store_episode(eps)
        agent._update_normalizer(eps)
        logs[name] = agent.update_kernels(N_UPDATES)
        for s in range(N_SEQ):
            agent._update_network(N_UPDATES)
            ma, va, _ = agent.get_adam_state(NET_ACTOR)
            mc, vc, _ = agent.get_adam_state(NET_CRITIC)
            got = {"grad_actor": agent.get_flat_grads(NET_ACTOR), "grad_critic": agent.get_flat_grads(NET_CRITIC),
                   "actor": agent._get_flat(NET_ACTOR), "critic": agent._get_flat(NET_CRITIC),
                   "actor_target": agent._get_flat(NET_ACTOR_TARGET), "critic_target": agent._get_flat(NET_CRITIC_TARGET),
                   "m_actor": ma, "v_actor": va, "m_critic": mc, "v_critic": vc,
                   "losses": agent.last_losses((s + 1) * N_UPDATES)}
            for k, v in got.items():
                out[f"{name}/{s}/{k}"] = np.asarray(v)
            agent._soft_update_target_network()       # (the targets move between sequences, as in a training cycle)

    for name, (batch, env, rccl, per_update) in CASES.items():
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ["RLARM_KEEP_GRADS"] = "1"
        os.environ.update(env)
        on_slab8 = per_update[0] == "k_fb_slab8"      # write-through is that kernel's default: compare its other instantiation
        if policy == "wt":
            os.environ["RLARM_ENGINE"] = "chain_wt"
        elif on_slab8:
            os.environ["RLARM_ENGINE"] = "chain_plain"
        torch.manual_seed(0)
        args = Args(batch_size=batch, buffer_size=8 * 100)
        if not rccl:
            sequences(name, ddpg_agent(args, None, dict(ENV_PARAMS), rng=fresh_rng(21)))
            continue
        import socket
        import torch.distributed as dist
        from rl_arm_under_sparse_reward_amd.utils import Communicator
        if not (dist.is_available() and dist.is_nccl_available()):
            logs[name] = "skipped: torch.distributed has no nccl backend"
            continue
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        comm = None
        try:
            comm = Communicator(0, force=True)
            agent = ddpg_agent(args, None, dict(ENV_PARAMS), comm=comm, rng=fresh_rng(21))
            assert comm.native is not None
            sequences(name, agent)
            _lib.Context.default().synchronize()
            torch.cuda.synchronize()
            agent.close_comm()
            del agent
        finally:
            if comm is not None:
                comm.close()
            _lib.Context.default().set_stream(None)
            dist.destroy_process_group()
    np.savez(out_path, **out)
    with open(out_path + ".json", "w") as fh:
        json.dump(logs, fh)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Both children, one after the other (the split launch wants the device to itself: its in-launch waits assume that the whole
    launch is resident); each result is computed once and shared by the cases."""
    d = tmp_path_factory.mktemp("chain_store_policy")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES + ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    res = {}
    for p in ("default", "wt"):
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", p, str(d / f"{p}.npz")], cwd=REPO, env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert proc.returncode == 0, f"child '{p}' ended with status {proc.returncode}:\n{proc.stdout[-3000:]}"
        with open(d / f"{p}.npz.json") as fh:
            res[p] = (np.load(d / f"{p}.npz"), json.load(fh))
    return res


@pytest.mark.parametrize("case", list(CASES))
def test_plain_and_write_through_chain_stores_give_the_same_bits(case, runs):
    (got, glog), (want, wlog) = runs["default"], runs["wt"]
    if isinstance(glog[case], str) or isinstance(wlog[case], str):
        pytest.skip(str(glog[case]))
    per_update = CASES[case][3]
    for log in (glog[case], wlog[case]):       # the launches the case is about
        assert len(log["updates"]) == N_UPDATES and all(u == per_update for u in log["updates"]), log
    keys = sorted(k for k in want.files if k.startswith(case + "/"))
    assert len(keys) == N_SEQ * 11 and sorted(k for k in got.files if k.startswith(case + "/")) == keys
    for k in keys:
        a, b = want[k], got[k]
        assert a.shape == b.shape and a.dtype == b.dtype and np.all(np.isfinite(a)), k
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), k
    assert np.any(want[f"{case}/0/grad_actor"] != 0) and np.any(want[f"{case}/0/grad_critic"] != 0)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2], sys.argv[3])
