#!/usr/bin/env python3
"""bench.py -- HER-relabelled transitions sampled+updated per second on MI355X.

Metric (BASELINE.json): transitions/s = B x (completed `_update_network` equivalents) / wall time,
steady state, replay buffer resident in HBM, PyBullet excluded.  A "step" is one pass of the hot
path over one minibatch: draw B indices, gather + relabel + reward + clip + normalise, 5 forwards,
3 backwards, Adam x2.  Every 40 steps (one training cycle, ddpg_agent.py:143-150) the cycle
boundary work is included in the timed region: store 2 fresh episodes (random-slot overwrite of a
full buffer), normalizer update + recompute, polyak update of both targets.

Workload at N=1 = BASELINE.json configs[1]: push task, buffer 5e5 (5000 episodes x 100 steps),
batch 256, replay_k=4.  N>1 (launched by torchrun, one rank per GPU): every rank owns a 5000-episode
shard and its own sampler stream (seed + rank, train.py:36); per step the gradients are all-reduced
(SUM, utils.py:47) between backward and Adam, per cycle the normalizer statistics are all-reduced
(mean, normalizer.py:60-64).  Weak scaling: global batch = N x 256.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR] [--full [--no-cpu-baseline]]

A plain run sets up, warms up, times the K steps and prints the headline line.  --full adds everything else the line
has carried: the CPU baseline, the per-kernel profile and roofline, the calibration probes, the cycle-inclusive estimate
of a short timed region and, at N > 1, the replica fingerprints, device ids and the timed pass over the other exchanges.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

N_BATCHES = 40            # arguments.py:77
ROLLOUTS_PER_CYCLE = 2    # arguments.py:100
FLOP_PER_TRANSITION = 2.0 * 1_382_912   # minimal algorithm, SURVEY.md section 8(d): 5 fwd + 3 bwd
FP32_MFMA_PEAK_TFLOPS = 157.3           # MI355X_MICROARCH.md, v_mfma_f32_16x16x4_f32 (no TF32 on gfx950)
HBM_PEAK_GBPS = 8000.0
# sample kernel algorithmic bytes / transition with this build's float64 storage:
#   reads  64 f64 (obs 27 + obs_next 27 + ag_next 3 + g-or-future-ag 3 + action 4) + one 16 B index record
#   writes 95 f32 (x 30 -> critic input and actor input, x' 30, a/max_action 4, reward 1)
SAMPLE_BYTES_PER_TRANSITION = 64 * 8 + 16 + 95 * 4

def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=400)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--episodes", type=int, default=5000, help="episodes resident per GPU (buffer 5e5)")
    ap.add_argument("--replay-k", type=int, default=4)
    ap.add_argument("--feeder-episodes", type=int, default=0,
                    help="config 5 of BASELINE.json: a host feeder thread stores this many extra episodes per cycle while "
                         "the cycles run (not part of the default bench line)")
    ap.add_argument("--feeder-envs", type=int, default=0,
                    help="config 5 of BASELINE.json with REAL rollouts: this many stand-in GoalEnvs stepped by worker "
                         "processes (rl_arm_under_sparse_reward_amd/feeder.py) on the snapshot policy while the cycles run; "
                         "every finished wave is stored into the shard by DMA out of the shared ring (not the default line)")
    ap.add_argument("--feeder-workers", type=int, default=8)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, run every other measurement and check the line has carried (see the module doc)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU baseline")
    ap.add_argument("--no-profile", action="store_true", help="with --full: leave out the per-kernel profile and roofline")
    ap.add_argument("--cpu-seconds", type=float, default=20.0)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step left to its caller as DIR/<name>.npy")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return a


class Runner:
    """Builds the device-side state for one rank and advances it in units of steps."""

    def __init__(self, a, rank, world, force_dp=False):
        import torch

        from rl_arm_under_sparse_reward_amd import _lib
        from rl_arm_under_sparse_reward_amd.arguments import Args
        from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
        from rl_arm_under_sparse_reward_amd.random import DeviceRandomState
        from rl_arm_under_sparse_reward_amd.synthetic import ENV_PARAMS, make_episodes
        from rl_arm_under_sparse_reward_amd.utils import Communicator

        self.torch = torch
        self.world = world
        local = int(os.environ.get("RLARM_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(local)
        self.ctx = _lib.Context(local)
        args = Args(batch_size=a.batch, buffer_size=a.episodes * 100, replay_k=a.replay_k, seed=125 + rank)
        self.rng = DeviceRandomState(args.seed, ctx=self.ctx)
        torch.manual_seed(0)                 # same initial networks on every rank (plus the broadcast)
        self.agent = ddpg_agent(args, None, dict(ENV_PARAMS), comm=Communicator(local, force=force_dp), ctx=self.ctx,
                                rng=self.rng)
        # resident shard (BASELINE.md section 3 recipe)
        eps = make_episodes(a.episodes, seed=1 + rank)
        self.agent.buffer.store_episode(eps)
        self.agent._update_normalizer()      # prime the normalizer (on the staged episodes' first T samples)
        self.pool = [make_episodes(ROLLOUTS_PER_CYCLE, seed=10_000 + 977 * rank + i) for i in range(16)]
        self.cycle = 0
        self.in_cycle = 0                    # steps done in the current cycle
        self.opens = self.closes = 0         # cycle boundaries issued: store + normalizer refresh / polyak
        self.feeder = None
        if a.feeder_episodes > 0:
            # host feeder: one batch of episodes per cycle from a second thread; the library's
            # per-context lock orders its stores with the cycles on the stream.  The thread is released right BEHIND a cycle's
            # launches (its host-side staging overlaps the cycle running on the device) and the next cycle's launches wait for
            # that CALL to have been made: which cycle samples which episodes must not depend on which thread wins the lock
            # (it did, in about one run of ten on a loaded box: same replicas on every rank, other losses than the run before)
            import threading
            self.feed_pool = [make_episodes(a.feeder_episodes, seed=20_000 + 31 * rank + i) for i in range(4)]
            self.feed_sem = threading.Semaphore(0)
            self.feed_stop = False
            self.fed = 0
            self._releases = 0

            def feed():
                while True:
                    self.feed_sem.acquire()
                    if self.feed_stop:
                        return
                    self.agent.buffer.store_episode(self.feed_pool[self.fed % len(self.feed_pool)])
                    self.fed += 1

            self.feeder = threading.Thread(target=feed, daemon=True)
            self.feeder.start()
        self.env_feeder = None
        if getattr(a, "feeder_envs", 0) > 0:
            import threading

            from rl_arm_under_sparse_reward_amd.feeder import EpisodeFeeder
            from rl_arm_under_sparse_reward_amd.synthetic import PointMassGoalEnv
            specs = [(PointMassGoalEnv, dict(seed=1000 * rank + i, max_timesteps=100)) for i in range(a.feeder_envs)]
            self.agent.policy_snapshot()
            self.env_feeder = EpisodeFeeder(self.agent, specs, n_workers=a.feeder_workers, n_slots=3, seed=77 + rank,
                                            snapshot_policy=True)
            self.env_stop = False
            self.env_waves = 0

            def roll():
                while not self.env_stop:
                    slot = self.env_feeder.collect_wave(explore=True)
                    self.env_feeder.store_wave(slot)
                    self.env_waves += 1

            self.env_thread = threading.Thread(target=roll, daemon=True)
        self.ctx.synchronize()

    def _open_cycle_eager(self):
        ag = self.agent
        ag.buffer.store_episode(self.pool[self.cycle % len(self.pool)])
        ag._update_normalizer()

    def run_steps(self, k):
        """Advance exactly k steps, including every cycle boundary crossed."""
        ag = self.agent
        while k > 0:
            if self.in_cycle == 0 and self.feeder is not None:
                self._feeder_wait()          # the previous cycle's batch has been stored (stream order: behind that cycle)
            if self.in_cycle == 0 and self.env_feeder is not None:
                ag.policy_snapshot()         # the rollout workers' policy follows the learner one cycle behind
            if self.in_cycle == 0 and k >= N_BATCHES and (self.world == 1 or ag._native_comm is not None
                                                          or ag._peer is not None):
                ag.train_cycle(self.pool[self.cycle % len(self.pool)], N_BATCHES)   # one hipGraph launch
                self._feeder_release()
                self.cycle += 1
                self.opens += 1
                self.closes += 1
                k -= N_BATCHES
                continue
            if self.in_cycle == 0:
                self._open_cycle_eager()
                self.opens += 1
            n = min(k, N_BATCHES - self.in_cycle)
            ag._update_network(n)
            self.in_cycle += n
            k -= n
            if self.in_cycle == N_BATCHES:
                ag._soft_update_target_network()
                self._feeder_release()
                self.in_cycle = 0
                self.cycle += 1
                self.closes += 1

    def _feeder_release(self):
        if self.feeder is not None:          # one feeder batch per cycle, staged while the device runs the cycle
            self.feed_sem.release()
            self._releases += 1

    def _feeder_wait(self):
        import time
        while self.fed < self._releases:
            if not self.feeder.is_alive():
                raise RuntimeError("bench: the host feeder thread died (its store_episode raised)")
            time.sleep(0.0001)

    def sync(self):
        if self.feeder is not None:          # the feeder's stores belong to the cycles that released them
            self._feeder_wait()
        self.ctx.synchronize()
        self.torch.cuda.synchronize()


def barrier(world):
    if world > 1:
        import torch.distributed as dist

        dist.barrier()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, r: Runner):
    """--dump-outputs: what the timed path hands its caller after its last step -- that step's (actor, critic) losses, the
    four networks and the two normalizers' statistics -- one DIR/<name>.npy each.  The inputs (episodes, initial networks,
    sampler stream) are seeded, so two builds run with the same arguments can be compared file for file."""
    from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_ACTOR_TARGET, NET_CRITIC, NET_CRITIC_TARGET

    ag = r.agent
    arrays = {"losses_last_step": ag.last_losses(1)[0],
              "actor_params": ag._get_flat(NET_ACTOR), "critic_params": ag._get_flat(NET_CRITIC),
              "actor_target_params": ag._get_flat(NET_ACTOR_TARGET), "critic_target_params": ag._get_flat(NET_CRITIC_TARGET),
              "o_norm_mean": ag.o_norm.mean, "o_norm_std": ag.o_norm.std,
              "g_norm_mean": ag.g_norm.mean, "g_norm_std": ag.g_norm.std}
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    assert all(v.dtype in (np.float32, np.float64) for v in arrays.values()), {k: v.dtype for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise RuntimeError(f"bench: --dump-outputs would write {total} bytes, more than {DUMP_LIMIT_BYTES}")
    os.makedirs(path, exist_ok=True)
    for name, v in arrays.items():
        np.save(os.path.join(path, name + ".npy"), v)


def profile_kernels(r: Runner, cycles=3):
    """Per-kernel-family device time measured with HIP events on the launch stream (eager launches,
    one event pair per launch; csrc/agent.hip ProfScope)."""
    import ctypes as C

    from rl_arm_under_sparse_reward_amd import _lib

    ag = r.agent
    _lib.check(ag.lib.hp_agent_profile(ag.h, 1))
    steps = 0
    for _ in range(cycles):
        r._open_cycle_eager()
        ag._update_network(N_BATCHES)
        ag._soft_update_target_network()
        r.cycle += 1
        steps += N_BATCHES
    r.sync()
    out = (C.c_double * 14)()
    _lib.check(ag.lib.hp_agent_profile_read(ag.h, out, 14))
    _lib.check(ag.lib.hp_agent_profile(ag.h, 0))
    names = ("sample", "forward", "backward_dx", "loss_head", "adam_polyak", "index_plan", "weight_grad")
    prof = {}
    for i, nm in enumerate(names):
        ms, cnt = out[2 * i], out[2 * i + 1]
        prof[nm] = {"ms_per_step": ms / steps, "launches_per_step": cnt / steps, "avg_us": (1e3 * ms / cnt) if cnt else 0.0}
    # calibration: what an event pair reads with NOTHING between the records on this stream -- the bracketing
    # overhead inside every per-launch measurement above (rocprofv3 kernel durations do not contain it)
    ctx = ag.ctx
    us = C.c_double()
    _lib.check(ctx.lib.hp_ctx_event_pair_us(ctx.h, 50, C.byref(us)))
    prof["_event_pair_empty_us"] = us.value
    return prof


# what hp_ctx_calibrate read on the boxes of the pool where the headline is 39-40 us/update (profiles/r04_calibration.txt)
CALIBRATION_TYPICAL = {"launch_floor_us": 1.57, "lds_dma_GBps_per_cu": 152.6, "mfma4x4_dependent_cycles": 14.7}


def baseline_metric_name(a):
    """BASELINE.json's metric string for its headline shape (batch 256, replay_k 4); the other shapes say what they are."""
    name = "HER-relabelled transitions sampled+updated /sec"
    try:
        with open(os.path.join(REPO, "BASELINE.json")) as fh:
            headline = json.load(fh)["metric"]
    except (OSError, KeyError, ValueError):
        headline = name + ", batch 256, 1/2/4/8 MI355X"
    if a.batch == 256 and a.replay_k == 4:
        return headline
    return f"{name}, batch {a.batch}, replay_k {a.replay_k} (not the BASELINE headline shape)"


def cpu_baseline(a, seconds):
    """The oracle ("port": numpy sampler + torch-CPU update, the reference's own arithmetic) on the
    host cores, same workload, bounded sample.  Checker code used as a timed baseline only."""
    import torch

    from oracle import ddpg_update as oupd
    from oracle.her_replay import EpisodeStore, future_probability
    from oracle.running_norm import RunningNorm, update_normalizers
    from rl_arm_under_sparse_reward_amd.synthetic import make_episodes

    n_eps = a.episodes
    eps = make_episodes(n_eps, seed=1)
    rs = np.random.RandomState(125)
    st = EpisodeStore(100, 27, 3, 4, n_eps * 100)
    st.store_episode(eps, rs)
    fp = future_probability("future", a.replay_k)
    on, gn = RunningNorm(27, default_clip_range=5), RunningNorm(3, default_clip_range=5)
    update_normalizers(on, gn, [x[:2] for x in eps], fp, rs)
    res = {}
    cores = os.cpu_count() or 1
    tried = sorted({1, min(8, cores), min(32, cores)})   # torch intra-op threads; best one is reported
    for threads in tried:
        torch.set_num_threads(threads)
        learner = oupd.DDPGLearner(oupd.init_actor(27, 3, 4, 0), oupd.init_critic(27, 3, 4, 1))
        for _ in range(5):
            tr, _ = st.sample(a.batch, fp, rs)
            learner.update(*oupd.minibatch_tensors(tr, on, gn))
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds / len(tried):
            tr, _ = st.sample(a.batch, fp, rs)
            learner.update(*oupd.minibatch_tensors(tr, on, gn))
            n += 1
            if n % N_BATCHES == 0:
                learner.soft_update()
        dt = time.perf_counter() - t0
        res[threads] = (n * a.batch / dt, n, dt)
    best = max(res, key=lambda k: res[k][0])
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    # BASELINE.json configs[0]: the reference's own CPU-runnable case -- buffer 1e4 (100 episodes), batch 256, replay_k 4,
    # ONE worker thread.  Timed beside the headline workload's figure, same oracle.
    torch.set_num_threads(1)
    eps1 = make_episodes(100, seed=1)
    rs1 = np.random.RandomState(125)
    st1 = EpisodeStore(100, 27, 3, 4, 100 * 100)
    st1.store_episode(eps1, rs1)
    fp1 = future_probability("future", 4)
    on1, gn1 = RunningNorm(27, default_clip_range=5), RunningNorm(3, default_clip_range=5)
    update_normalizers(on1, gn1, [x[:2] for x in eps1], fp1, rs1)
    learner = oupd.DDPGLearner(oupd.init_actor(27, 3, 4, 0), oupd.init_critic(27, 3, 4, 1))
    for _ in range(3):
        tr, _ = st1.sample(256, fp1, rs1)
        learner.update(*oupd.minibatch_tensors(tr, on1, gn1))
    n1, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < max(2.0, seconds / 4):
        tr, _ = st1.sample(256, fp1, rs1)
        learner.update(*oupd.minibatch_tensors(tr, on1, gn1))
        n1 += 1
        if n1 % N_BATCHES == 0:
            learner.soft_update()
    dt1 = time.perf_counter() - t0
    config1 = {"value": round(n1 * 256 / dt1, 1), "unit": "transitions/s", "cores": 1, "kind": "port",
               "sample": f"{n1} sample+update steps at batch 256, replay_k 4 on a 100-episode buffer (buffer_size 1e4), 1 torch thread "
                         f"({dt1:.1f} s): BASELINE.json configs[0]"}
    return {
        "value": round(res[best][0], 1), "unit": "transitions/s", "cores": best, "kind": "port", "config1": config1,
        "sample": f"{res[best][1]} sample+update steps at batch {a.batch} on a {n_eps}-episode buffer "
                  f"({res[best][2]:.1f} s), oracle = numpy legacy-RNG sampler + torch-CPU update",
        "value_by_threads": {str(k): round(v[0], 1) for k, v in res.items()}, "host_cpu": model, "host_cores": cores,
    }


def self_launch(a):
    """`python bench.py --gpus N` from a plain shell: re-exec under torch.distributed.run, one rank per GPU (the form
    the contract names: --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1).  Rank 0 of the child job prints the
    JSON line; this parent only relays the exit status."""
    import socket
    import subprocess

    port = os.environ.get("MASTER_PORT")
    if not port:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = str(sk.getsockname()[1])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")    # dmabuf IPC (RCCL / peer memory across processes)
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.call(cmd, env=env)


def first_cycle_or_fallback(a, rank, world, force_dp, shared):
    """Build the rank's state and run the first full cycle (graph capture, exchange set-up).  At N > 1 the ranks then agree
    that it went through everywhere; if the peer-memory exchange failed on any rank (a bounded wait of its kernels gave up,
    an IPC mapping the self-check did not catch) ALL ranks rebuild on the next transport down -- library-side RCCL, then
    torch.distributed -- instead of leaving the scaling run without a line.  config.exchange names what ran."""
    order = ["auto", "rccl", "torch"]
    forced = os.environ.get("RLARM_COMM")
    if forced in order:
        order = order[order.index(forced):]
    elif forced:
        order = [forced]
    last, failures = None, []
    for mode in order:
        if mode != "auto" or forced:
            os.environ["RLARM_COMM"] = mode
        ok, r = 1, None
        try:
            r = Runner(a, rank, world, force_dp)
            r.run_steps(N_BATCHES)
            r.sync()
            r.agent.check_exchange()     # a wait that timed out inside the cycle (peer.h: fatal, sticky) fails this transport
            if os.environ.get("RLARM_BENCH_FAIL_FIRST") == str(rank) and mode == order[0]:   # test hook: one rank's first
                raise RuntimeError("injected failure (RLARM_BENCH_FAIL_FIRST)")                # transport "fails"
        except Exception as e:          # noqa: BLE001 -- any failure of this rank must reach the agreement below
            ok, last = 0, e
            print(f"[bench rank {rank}] exchange '{mode}' failed in the first cycle: {e}", file=sys.stderr, flush=True)
        if world > 1:
            import torch
            import torch.distributed as dist
            t = torch.tensor([ok], dtype=torch.int32, device="cpu" if shared else "cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            all_ok = int(t.item())
        else:
            all_ok = ok
        if all_ok:
            # what was tried and dropped on the way to the transport that ran (rank 0's view): a peer exchange the ranks refused
            # at attach time (IPC mapping, self-check), transports whose first cycle failed
            refused = getattr(r.agent.comm, "peer_refused", None)
            r.fallbacks = failures + ([{"exchange": "peer-memory", "refused_at_attach": refused}] if refused else [])
            return r
        failures.append({"exchange": mode, "first_cycle_error": str(last) if not ok else "failed on another rank"})
        if r is not None:               # free the exchange memory / communicator of the transport that is being dropped
            try:
                r.agent.close_comm()
            except Exception:           # noqa: BLE001
                pass
        if world == 1:
            break
    raise RuntimeError(f"no exchange transport completed the first cycle: {last}")


def exchange_name(agent):
    """What actually carries the gradient exchange of this agent: (transport, peer phases or None)."""
    import ctypes as C
    if agent._peer is not None:
        ph = C.c_int32()
        agent.lib.hp_peer_phases(agent._peer, C.byref(ph))
        return "peer-memory", ph.value
    return ("rccl" if agent._native_comm is not None else "torch.distributed"), None


def replicas_identical(r, world, shared):
    """Data-parallel replicas must hold the SAME networks bit for bit: every rank fingerprints its online + target
    parameters, all ranks learn whether all fingerprints agree."""
    import zlib

    import torch
    import torch.distributed as dist
    crc = [zlib.crc32(r.agent._get_flat(slot).tobytes()) for slot in (0, 1, 2, 3)]
    mine = torch.tensor(crc, dtype=torch.int64, device="cpu" if shared else "cuda")
    every = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    return all(bool(torch.equal(e, every[0])) for e in every)


def time_exchange_alternatives(a, rank, world, shared, ran, done, deadline, n_cycles=10):
    """N > 1 only, after the timed region (there may be exactly one multi-GPU run): a short timed pass on
    each exchange transport that did NOT carry the headline -- library-side RCCL inside the cycle graph (what north_star names),
    the peer-memory exchange in its other form(s), torch.distributed from a host loop -- with us/update and whether the replicas
    stayed bit-identical.  Every step is agreed on by all ranks BEFORE any collective kernel of the pass is enqueued; a transport
    that fails is recorded with its error and the next one is tried.  `done` collects the records as they finish (the watchdog in
    main() prints the line with whatever is there if a pass hangs), `deadline` (time.monotonic) is the time box of the whole
    pass: every transport gets an equal share of what is left, its number of cycles is cut to fit (at eight ranks on ONE device a
    pass read 11-22 ms per update), and what does not fit at all is recorded as skipped."""
    import torch
    import torch.distributed as dist

    plans = [("rccl in the cycle graph", {"RLARM_COMM": "rccl"}),
             ("peer memory, one-shot inside the weight-gradient launch (tile-wise)", {"RLARM_COMM": "peer", "RLARM_PEER_PHASES": "1"}),
             ("peer memory, one-shot as its own exchange + optimizer launch", {"RLARM_COMM": "peer", "RLARM_PEER_PHASES": "1", "RLARM_PEER_TILES": "0"}),
             ("peer memory, two-phase (reduce-scatter + all-gather)", {"RLARM_COMM": "peer", "RLARM_PEER_PHASES": "2"}),
             ("torch.distributed, host-driven loop", {"RLARM_COMM": "torch"})]
    plain = argparse.Namespace(**{**vars(a), "feeder_episodes": 0, "feeder_envs": 0})   # the passes time the exchange, not a feeder
    keys = sorted({k for _, env in plans for k in env})
    saved = {k: os.environ.get(k) for k in keys}
    dev = "cpu" if shared else "cuda"

    def agree_min(v, dtype=torch.int32):
        t = torch.tensor([v], dtype=dtype, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return t.item()

    def agree_max(v):
        t = torch.tensor([v], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    for n_plan, (name, env) in enumerate(plans):
        left = len(plans) - n_plan
        share = agree_min((deadline - time.monotonic()) / left, torch.float64)     # every rank works with the same budget
        rec = {"exchange": name, "env": env}
        if share < 4.0:
            rec["skipped"] = f"time box: {share:.1f} s left for this pass (RLARM_BENCH_ALT_BUDGET_S)"
            done.append(rec)
            continue
        t_pass = time.monotonic()
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(env)
        ok, r2, err = 1, None, None
        try:
            r2 = Runner(plain, rank, world, False)
            if os.environ.get("RLARM_BENCH_FAIL_ALT") and name.startswith(os.environ["RLARM_BENCH_FAIL_ALT"]) and rank == 0:
                raise RuntimeError("injected failure (RLARM_BENCH_FAIL_ALT)")     # test hook: one rank's pass "fails"
        except Exception as e:      # noqa: BLE001 -- every rank must reach the agreement below
            ok, err = 0, str(e)
        # agreed BEFORE the first collective kernel of this pass: a rank that could not build its state must not leave the
        # others inside an RCCL / torch.distributed collective that never completes
        if int(agree_min(ok)) == 1:
            try:
                t0 = time.perf_counter()
                r2.run_steps(2 * N_BATCHES)
                r2.sync()
                r2.agent.check_exchange()
                warm = time.perf_counter() - t0
            except Exception as e:  # noqa: BLE001
                ok, err, warm = 0, str(e), 0.0
        if int(agree_min(ok)) == 1:
            got, phases = exchange_name(r2.agent)
            rec["ran_as"] = got + (f", phases {phases}" if phases else "") + (", gate kernels (ranks share a device)" if r2.agent._peer is not None and r2.agent.comm.shared_device else "")
            try:
                rec["kernels_per_update"] = r2.agent.engine().get("kernels_per_update")
            except Exception:   # noqa: BLE001
                pass
            # cycles that fit this pass's share of the time box (the two warm cycles above say what a cycle costs here)
            per_cycle = agree_max(warm / 2.0)
            room = share - (time.monotonic() - t_pass) - 2.0
            n_cyc = int(max(1, min(n_cycles, room / max(per_cycle, 1e-6))))
            n_cyc = int(agree_min(n_cyc))
            try:
                barrier(world)
                t0 = time.perf_counter()
                r2.run_steps(n_cyc * N_BATCHES)
                r2.sync()
                barrier(world)
                dt = time.perf_counter() - t0
                r2.agent.check_exchange()
            except Exception as e:  # noqa: BLE001
                ok, err = 0, str(e)
                dt = float("nan")
            if int(agree_min(ok)) == 1:
                dt = agree_max(dt)
                rec.update(us_per_update=round(1e6 * dt / (n_cyc * N_BATCHES), 3),
                           value=round(world * a.batch * n_cyc * N_BATCHES / dt, 1), steps=n_cyc * N_BATCHES,
                           replicas_bit_identical=replicas_identical(r2, world, shared),
                           same_as_headline=(got, phases) == ran and "RLARM_PEER_TILES" not in env)
            else:
                rec["error"] = err or "failed on another rank"
        else:
            rec["error"] = err or "failed on another rank"
        if r2 is not None:
            try:
                r2.agent.close_comm()
            except Exception:       # noqa: BLE001
                pass
            del r2
        done.append(rec)
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    return done


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(a))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    a.gpus = world
    import torch

    # Fewer visible GPUs than ranks (a 1-GPU box rehearsing the N-rank code path): ranks share devices round-robin.
    # RCCL refuses two ranks on one device, so the process group is gloo and the exchange goes through the library's
    # peer-memory all-reduce or, failing that, through torch.distributed on host copies.  Never a bench line to quote.
    n_dev = torch.cuda.device_count()
    shared = world > n_dev
    if "LOCAL_RANK" in os.environ and n_dev > 0:
        os.environ["RLARM_DEVICE"] = str(int(os.environ["LOCAL_RANK"]) % n_dev)

    # RLARM_BENCH_FORCE_DP=1 (diagnostic): run the data-parallel code path -- process group, library-side RCCL
    # communicator, collectives inside the cycle graph -- in a 1-rank group, e.g. to check it on a single-GPU box
    force_dp = world == 1 and os.environ.get("RLARM_BENCH_FORCE_DP") == "1"
    if world > 1 or force_dp:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        dev = int(os.environ.get("RLARM_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(dev)
        if shared:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev))
    r = first_cycle_or_fallback(a, rank, world, force_dp, shared)
    # One-time initialisation, not warm-up.  (1) The first full cycle captures and instantiates the cycle hipGraph (and,
    # at N > 1, sets up the exchange channels).  (2) A rehearsal of the exact warm-up + timed step pattern lets the
    # library capture the partial-cycle graphs that pattern needs (hp_agent_sample_and_update caches one graph per
    # chunk length), then the cycle is completed so that the measured pass starts at the same cycle position and
    # replays the same graphs.  Without it a short --steps would time graph instantiation instead of the hot path.
    # A timed region shorter than a cycle is placed so that it ENDS on a cycle boundary: the soft target update (polyak) of
    # that cycle is then inside the region; `pre` untimed steps in front of the warm-up do the placing.
    pre = (-(a.warmup + a.steps)) % N_BATCHES if a.steps < N_BATCHES else 0
    r.run_steps(pre)
    r.run_steps(a.warmup)
    r.run_steps(a.steps)
    r.run_steps((-r.in_cycle) % N_BATCHES)
    r.sync()
    # The timed loop is a few Python calls per 40 steps; CPython's generational collector, with torch and numpy loaded,
    # takes 30-50 ms for a full (generation 2) pass and triggers one after ~150 cycle calls of a fresh process -- a stall
    # of 700+ steps that is the interpreter's, not the hot path's (tools/ubench/cycle_drift.py).  Long-lived objects are
    # frozen out of the collector and automatic collection is off while the clock runs, as a training loop would do.
    import gc
    gc.collect()
    gc.freeze()
    gc.disable()
    barrier(world)
    if r.env_feeder is not None:
        r.env_thread.start()                 # rollouts run concurrently with everything below
    r.run_steps(pre)
    r.run_steps(a.warmup)
    r.sync()
    barrier(world)
    r.sync()
    opens0, closes0 = r.opens, r.closes
    waves0 = r.env_waves if r.env_feeder is not None else 0
    t0 = time.perf_counter()
    r.run_steps(a.steps)
    r.sync()                      # this rank's K steps are done (ctx.synchronize + torch.cuda.synchronize) ...
    barrier(world)                # ... and every other rank's: the region ends when the last rank leaves its sync
    dt = time.perf_counter() - t0
    gc.enable()
    r.agent.check_exchange()      # a timed region in which an exchange wait timed out (steps skipped) is not a measurement
    feeder_stats = None
    if r.env_feeder is not None:
        waves = r.env_waves - waves0
        r.env_stop = True
        r.env_thread.join(timeout=30)
        feeder_stats = {"envs": a.feeder_envs, "worker_processes": r.env_feeder.n_workers, "waves_in_timed_region": waves,
                        "episodes_per_s": round(waves * a.feeder_envs / dt, 1),
                        "env_steps_per_s": round(waves * a.feeder_envs * 100 / dt, 1),
                        "policy": "hp_agent_act_snapshot on a second stream (snapshot per cycle), one batched call per timestep",
                        "store": "hp_buffer_store_pinned: DMA out of the device-registered shared-memory ring",
                        "env": "synthetic.PointMassGoalEnv (PyBullet is absent from the box)"}
        r.env_feeder.close()
    if a.dump_outputs and rank == 0:      # data-parallel replicas hold the same networks: rank 0 writes for all of them
        dump_outputs(a.dump_outputs, r)
    # cycle-boundary work inside the timed region: [store 2 episodes + normalizer refresh, polyak]; a steady state has
    # one of each per 40 steps
    boundaries = {"store_and_normalizer": r.opens - opens0, "polyak": r.closes - closes0,
                  "steady_state_would_have": round(a.steps / N_BATCHES, 3),
                  **({"placement": f"the {a.steps} timed steps are the LAST {a.steps} updates of a cycle: its soft target update is "
                                   "inside the region, the next cycle's store + normalizer refresh is not (cycle_inclusive_estimate "
                                   "covers whole cycles)"} if a.steps < N_BATCHES else {})}
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if shared else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    # A timed region shorter than one training cycle (the driver's --steps 20) crosses no cycle boundary: measure the
    # boundary-inclusive rate as well, over whole cycles (store 2 episodes, normalizer refresh, 40 updates, polyak each),
    # after the timed region so that the contract's K steps stay exactly K (--full)
    cycle_inclusive = None
    if a.full and (boundaries["polyak"] < max(1, a.steps // N_BATCHES) or a.steps < N_BATCHES):
        n_cyc = 25
        r.run_steps((-r.in_cycle) % N_BATCHES)
        r.run_steps(2 * N_BATCHES)
        r.sync()
        barrier(world)
        tc = time.perf_counter()
        r.run_steps(n_cyc * N_BATCHES)
        r.sync()
        barrier(world)
        dtc = time.perf_counter() - tc
        if world > 1:
            t = torch.tensor([dtc], dtype=torch.float64, device="cpu" if shared else "cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dtc = float(t.item())
        cycle_inclusive = {"steps": n_cyc * N_BATCHES, "cycle_boundaries": n_cyc,
                           "ms_per_step": round(1e3 * dtc / (n_cyc * N_BATCHES), 6),
                           "value": round(world * a.batch * n_cyc * N_BATCHES / dtc, 1),
                           "note": "same process, measured right after the timed region over whole cycles; `value` above is the "
                                   "contract's K-step figure"}
    losses = r.agent.last_losses(1)[0]
    dp = world > 1 or force_dp
    # data-parallel replicas must hold the SAME networks bit for bit (same summed gradients, same Adam): every rank
    # fingerprints its online + target parameters and rank 0 reports whether all fingerprints agree
    replicas_same = None
    devices = None
    if world > 1 and a.full:
        replicas_same = replicas_identical(r, world, shared)
        # "N ranks on N devices" belongs in the record: every rank's PCI bus id, and how many ranks the exchange itself counts
        import ctypes as _C0
        bus = _C0.create_string_buffer(32)
        r.ctx.lib.hp_ctx_pci_bus_id(r.ctx.h, bus, 32)
        mine_id = torch.tensor(list(bus.raw), dtype=torch.uint8, device="cpu" if shared else "cuda")
        ids = [torch.zeros_like(mine_id) for _ in range(world)]
        dist.all_gather(ids, mine_id)
        names = [bytes(t.cpu().tolist()).split(b"\0")[0].decode("ascii", "replace") for t in ids]
        devices = {"pci_bus_ids_by_rank": names, "distinct_devices": len(set(names)), "process_group_backend": dist.get_backend(),
                   "process_group_ranks": dist.get_world_size()}
        if r.agent._native_comm is not None:
            rk, wd = _C0.c_int32(), _C0.c_int32()
            r.agent.lib.hp_comm_info(r.agent._native_comm, _C0.byref(rk), _C0.byref(wd))
            devices["rccl_communicator_ranks"] = wd.value
    # What ran, asked WHILE the transport that carried the timed region is still attached (VERDICT r05 Weak 3: asked after
    # close_comm() the agent is single-rank again and names kernels a data-parallel rank never launches): the engine, the
    # kernels of one update read off the library's own launch logic (hp_agent_update_kernels), the exchange.
    eng = r.agent.engine() if a.full else None
    ran = exchange_name(r.agent) if dp else None
    dp_native = r.agent._native_comm is not None
    dp_peer = r.agent._peer is not None
    peer_phases = ran[1] if (dp and dp_peer) else None
    import ctypes as _C
    mode = _C.c_int32()
    r.agent.lib.hp_agent_cycle_mode(r.agent.h, _C.byref(mode))
    cycle_mode = {0: "none", 1: "hipGraph", 2: "eager launches"}.get(mode.value, str(mode.value))
    # live per-launch durations (HIP event pairs on the launch stream).  At N > 1 every rank runs the pass -- its launches
    # exchange with the peers' -- and rank 0 reports its own figures.
    prof = None
    if a.full and not a.no_profile:
        try:
            prof = profile_kernels(r)
            r.agent.check_exchange()
        except Exception as e:      # noqa: BLE001 -- a diagnostic pass must not cost the run its line
            prof = None
            print(f"[bench rank {rank}] profile pass failed: {e}", file=sys.stderr, flush=True)
    if world > 1:
        barrier(world)
    ms_per_step = 1e3 * dt / a.steps
    value = world * a.batch * a.steps / dt
    out = None
    if rank == 0:
        import ctypes as C
        from rl_arm_under_sparse_reward_amd import _lib as _l
        diagnostics, full_config = {}, {}
        if a.full:
            mhz = C.c_double()
            _l.check(r.ctx.lib.hp_ctx_clock_mhz(r.ctx.h, C.byref(mhz)))      # shader clock right after the timed region
            cal = (C.c_double * 4)()
            try:
                _l.check(r.ctx.lib.hp_ctx_calibrate(r.ctx.h, cal))
                calibration = {"launch_floor_us": round(cal[0], 3), "lds_dma_GBps_per_cu": round(cal[1], 1),
                               "mfma4x4_dependent_cycles": round(cal[2], 2), "shader_clock_mhz": round(cal[3]),
                               "typical": CALIBRATION_TYPICAL}
            except Exception as e:        # noqa: BLE001 -- a diagnostic must not cost the run its line
                calibration = {"error": str(e)}
            full_config = {"engine": eng, "shader_clock_mhz_after_run": round(mhz.value)}
            # ~200 us of probes that characterise THIS box (rlarm_hip_debug.h: hp_ctx_calibrate), taken right after the timed
            # region: about one box in seven of the pool ran every kernel of this path ~1.4 x slower at the same shader clock --
            # with these three rates in the line a slow box can be told from a regression
            diagnostics = {"calibration": calibration}
        out = {
            "metric": baseline_metric_name(a),
            "value": round(value, 1), "unit": "transitions/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(ms_per_step, 6), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "init": "untimed before the warm-up: one training cycle (cycle hipGraph capture / exchange set-up) and one rehearsal "
                    "of the warm-up + timed step pattern (partial-cycle graph captures), ending on a cycle boundary",
            "cycle_boundaries_in_timed_region": boundaries,
            **({"cycle_inclusive_estimate": cycle_inclusive} if cycle_inclusive else {}),
            **({"host_feeder": feeder_stats} if feeder_stats else {}),
            "config": {"workload": f"push task (obs 27, goal 3, action 4, T 100), buffer {a.episodes * 100} transitions "
                                   f"({a.episodes} episodes) per GPU, batch {a.batch} per GPU, replay_k {a.replay_k}, "
                                   "HIP HER sampler + FP32-MFMA DDPG update, 40 updates + store/normalizer/polyak per cycle",
                       "global_batch": world * a.batch, "episodes_per_gpu": a.episodes,
                       **({"feeder_episodes_per_cycle": a.feeder_episodes} if a.feeder_episodes else {}),
                       "parallelism": f"dp{world}" + (
                           " (grad SUM per update [reference semantics, utils.py:47] + normalizer MEAN per cycle: " +
                           ("all-reduce over peer memory fused with Adam, inside the cycle graph)" if dp_peer else
                            "RCCL all-reduce issued by the library inside the cycle graph)" if dp_native
                            else "torch.distributed, host-driven loop)") if dp else ""),
                       "exchange": ("peer-memory" if dp_peer else "rccl" if dp_native else "torch.distributed") if dp else None,
                       "exchange_fallbacks": getattr(r, "fallbacks", None) or None,
                       "peer_exchange_form": {1: "one-shot (every rank reads every peer's whole gradient vector)",
                                              2: "two-phase (reduce-scatter + all-gather over peer memory)"}.get(peer_phases),
                       "cycle_mode": cycle_mode,
                       "peer_gate_kernels": bool(r.agent.comm.shared_device) if dp_peer else None,
                       **({"replicas_bit_identical": replicas_same, "devices": devices} if world > 1 and a.full else {}),
                       "devices_shared_by_ranks": bool(shared) if world > 1 else None,
                       "sampler_rng": "MT19937 numpy-legacy stream on device (bit-exact indices)",
                       "final_losses": [float(losses[0]), float(losses[1])],
                       **full_config},
            **diagnostics,
        }
        if prof:
            out.update(roofline_fields(a, r, eng, prof, ms_per_step, world, dp, ran))
        if a.full and not a.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(a, a.cpu_seconds)
            out["speedup_vs_cpu_baseline"] = round(value / out["cpu_baseline"]["value"], 1)
            # the port timed next to the imported reference where both can run (the build container,
            # tools/cpu_ratio.py) -- the factor that turns "x the port" into "x the reference CPU path"
            ratio_file = os.path.join(REPO, "profiles", "r03_cpu_port_over_reference.json")
            if os.path.exists(ratio_file):
                with open(ratio_file) as fh:
                    rdoc = json.load(fh)
                out["cpu_baseline"]["port_over_reference"] = rdoc["port_over_reference"]
                out["cpu_baseline"]["port_over_reference_source"] = (
                    "profiles/r03_cpu_port_over_reference.json (tools/cpu_ratio.py on the build container: "
                    f"{rdoc.get('host_cpu', '?')}, by threads {({k: v['port_over_reference'] for k, v in rdoc['by_threads'].items()})})")
                out["speedup_vs_reference_cpu_estimate"] = round(out["speedup_vs_cpu_baseline"] * rdoc["port_over_reference_min"], 1)

    def emit(record):
        # RCCL prints its version banner through C stdio, which would otherwise be flushed AFTER Python's output at exit:
        # drain it first so that the JSON record is the last line on stdout
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:       # noqa: BLE001
            pass
        print(json.dumps(record), flush=True)

    if dp:
        r.agent.close_comm()
    if world > 1 and a.full and os.environ.get("RLARM_BENCH_ALTERNATIVES", "1") != "0":
        # The headline record is COMPLETE at this point.  The extra passes run against a time box, under a watchdog: if one of
        # them hangs (a rank died inside a collective) the watchdog prints the line with the passes that finished and
        # ends the process with status 0 -- on every rank, rank 0 first -- instead of losing what may be the only multi-GPU run.
        import threading
        budget = float(os.environ.get("RLARM_BENCH_ALT_BUDGET_S", "150"))
        finished = []
        printed = threading.Lock()

        def watchdog():
            if not printed.acquire(blocking=False):
                return
            if rank == 0:
                out["exchange_alternatives"] = list(finished) + [
                    {"error": f"alternatives pass stopped by the watchdog {budget + 30:.0f} s after it began: a pass did not return "
                              "(the records above are the passes that finished)"}]
                emit(out)
            os._exit(0)

        timer = threading.Timer(budget + 30 + (0 if rank == 0 else 5), watchdog)
        timer.daemon = True
        timer.start()
        try:
            time_exchange_alternatives(a, rank, world, shared, ran, finished, time.monotonic() + budget)
            alternatives = list(finished)
        except Exception as e:      # noqa: BLE001 -- the headline line must survive anything that happens in the extra passes
            alternatives = list(finished) + [{"error": f"alternatives pass aborted: {e}"}]
        if not printed.acquire(blocking=False):     # the watchdog is printing: leave the exit to it
            time.sleep(60)
        timer.cancel()
        if rank == 0:
            out["exchange_alternatives"] = alternatives
    if dp:
        try:
            dist.destroy_process_group()
        except Exception:           # noqa: BLE001
            pass
    if rank == 0:
        emit(out)


def short_kernel(name):
    """'void s8r4::k_fb_split8<0>(unsigned long long, ...)' / 's8r4::k_fb_split8(unsigned' -> 'k_fb_split8<0>' / 'k_fb_split8'
    (tools/trace_summary.py prints this form; summaries committed before round 6 carry the long one)."""
    n = name.strip()
    if n.startswith("void "):
        n = n[5:]
    return n.split("(")[0].split("::")[-1]


def committed_kernel_averages(path):
    """{short kernel name: avg_us}, csrc fingerprint of a committed tools/trace_summary.py file (prologue rows aside)."""
    avg, sha = {}, None
    if not os.path.exists(path):
        return avg, sha
    for line in open(path):
        if line.startswith("# csrc_sha16"):
            sha = line.split()[2]
        cols = line.rstrip().rsplit(None, 5)
        if len(cols) == 6 and not line.startswith("#") and cols[-1].endswith("%") and "[prologue" not in cols[0]:
            try:
                avg.setdefault(short_kernel(cols[0]), float(cols[2]))
            except ValueError:
                pass
    return avg, sha


def roofline_fields(a, r, eng, prof, ms_per_step, world, dp, ran):
    """`roofline` (+ the sampler's two lines at N = 1) of the bench record.  The kernels are the ones the library's launch logic
    names for THIS agent with its transport attached (eng["kernels_per_update"]); durations are this run's HIP event pairs, held
    against the committed rocprofv3 summary of the same configuration where one exists."""
    import ctypes as C

    from rl_arm_under_sparse_reward_amd import _lib as _l
    out = {}
    # Algorithmic MACs per transition (minimal algorithm): 5 forward passes 699,648 + backward dX chains
    # 395,776 run in the chain kernel(s); weight gradients 287,488 (critic 34*256 + 2*256*256 + 256, actor 30*256 + 2*256*256 + 4*256)
    ev_floor_us = prof.pop("_event_pair_empty_us", 0.0)
    kp = eng.get("kernels_per_update") or []
    fallback_chain = {"slab8": "k_fb_slab8", "slab32": "k_fb_slab32"}.get(eng["engine"], "k_gemm_lds")
    chain_kernel = kp[0] if kp else fallback_chain
    dw_kernel = next((k for k in kp[1:] if k.startswith(("k_gemm_lds", "k_dw64"))),
                     "k_dw64_adam" if eng["weight_grad"].startswith("dw64") else "k_gemm_lds_adam")
    split = chain_kernel.startswith("k_fb_split8")
    dw_critic = round(287_488 * 140_032 / 279_808)
    dw_actor = 287_488 - dw_critic
    single = not dp
    if split:   # slab8_split.h: the chain launch also holds the critic's weight gradients (+ exchange + Adam); the launch behind it the actor's
        kinds = {"chain": (None, 699_648 + 395_776 + dw_critic, chain_kernel), "weight_grad": (None, dw_actor, dw_kernel)}
    else:
        kinds = {"chain": (11 if single else None, 699_648 + 395_776, chain_kernel), "weight_grad": (12 if single else None, 287_488, dw_kernel)}
    # HBM traffic needs rocprofv3 --pmc passes around the process (tools/gpu_round6.sh), so it cannot be measured from
    # inside this run: it is read from the newest committed counter summary of this shape, which records a fingerprint of
    # the kernel sources it was taken on -- when the sources have changed since, the figure is reported as stale
    tag = "" if single else "_forced_dp_" + ("peer" if ran and ran[0] == "peer-memory" else "rccl" if ran and ran[0] == "rccl" else "torch")
    pmc, pmc_file, pmc_sha = {}, None, None
    for rnd in ("r06", "r05", "r04", "r03", "r02"):
        cand = f"{rnd}_pmc_traffic_b{a.batch}{tag}.json"
        path = os.path.join(REPO, "profiles", cand)
        if os.path.exists(path) and os.environ.get("RLARM_ENGINE") is None and os.environ.get("RLARM_SLAB_ROWS") is None:
            with open(path) as fh:
                doc = json.load(fh)
            pmc = {short_kernel(k): v["hbm_bytes_per_launch"] for k, v in doc["kernels"].items() if "[prologue" not in k}
            pmc_file, pmc_sha = "profiles/" + cand, doc.get("csrc_sha16")
            break
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        from pmc_summary import csrc_sha16
        sha_now = csrc_sha16()
    except Exception:                      # noqa: BLE001
        sha_now = None
    traffic_stale = (pmc_sha is None or sha_now is None or pmc_sha != sha_now) if pmc_file else None
    # committed rocprofv3 summary of this same configuration (tools/gpu_round6.sh): cross-check for the live numbers.  A real
    # multi-GPU run (world > 1) has no committed trace: its durations are this run's event pairs alone.
    prof_file = None
    if world == 1:
        for rnd in ("r06", "r05", "r04", "r03", "r02"):
            cand = os.path.join(REPO, "profiles", f"{rnd}_kernel_trace_b{a.batch}_k{a.replay_k}{tag}.txt")
            if os.path.exists(cand):
                prof_file = cand
                break
    prof_avg, prof_sha = committed_kernel_averages(prof_file) if prof_file else ({}, None)

    def committed(kernel):     # summaries from before round 6 name the (then untemplated) split kernel without its <form>
        return prof_avg.get(kernel) or prof_avg.get(kernel.split("<")[0]) or 0.0

    def traffic_of(kernel):
        return pmc.get(kernel) or pmc.get(kernel.split("<")[0])

    per = {}
    for name, (kind, macs, kernel) in kinds.items():
        us = C.c_double(float("nan"))
        if kind is not None:
            _l.check(r.agent.lib.hp_agent_debug_chain(r.agent.h, kind, 200, C.byref(us)))
        ev = prof.get({"chain": "forward", "weight_grad": "weight_grad"}[name], {})
        ev2 = prof.get("backward_dx", {}) if name == "chain" else {}
        # live, in situ: one HIP event pair around each eager launch of the training loop on the launch stream, minus what
        # an event pair with nothing in between reads on this stack
        live = ev.get("avg_us", 0.0) - ev_floor_us + (ev2.get("avg_us", 0.0) - ev_floor_us if ev2.get("avg_us") else 0.0)
        rp = committed(kernel)
        if name == "weight_grad" and not rp:   # the ride-along variant runs on all but the last updates of a cycle
            rp = next((committed(k) for k in (kernel + "_ride", kernel.replace("_u", "") + "_ride_u") if committed(k)), 0.0)
        used = max(live, rp)
        tf = 2.0 * macs * a.batch / (used * 1e-6) / 1e12 if used > 0 else 0.0
        per[name] = {"kernel": kernel, "avg_launch_us": round(used, 3), "duration_source": "live" if live >= rp else "committed",
                     "live_event_pair_minus_empty_us": round(live, 3),
                     "rocprofv3_avg_us_committed": round(rp, 3) if rp else None,
                     "graph_replay_warm_us": round(us.value, 3) if us.value == us.value else None, "flop_per_launch": 2.0 * macs * a.batch,
                     "achieved_tflops": round(tf, 3), "frac": round(tf / FP32_MFMA_PEAK_TFLOPS, 5),
                     "traffic_hbm_bytes_per_launch": traffic_of(kernel)}
    dom = max(per, key=lambda k: per[k]["avg_launch_us"])
    pf = os.path.basename(prof_file) if prof_file else None
    out["roofline"] = {
        "bound": "mfma", "kernel": per[dom]["kernel"], "achieved": per[dom]["achieved_tflops"],
        "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": per[dom]["frac"],
        "traffic": per[dom]["traffic_hbm_bytes_per_launch"], "traffic_unit": "HBM bytes per launch (PMC)",
        "traffic_source": pmc_file, "traffic_stale": traffic_stale,
        "traffic_note": "PMC (2 x FETCH_SIZE + WRITE_SIZE) x 1 KiB per launch from separate rocprofv3 --pmc passes of this "
                        "shape; traffic_stale = the kernel sources differ from the ones the counters were taken on "
                        f"(csrc fingerprint then {pmc_sha}, now {sha_now})",
        "flop_per_launch": per[dom]["flop_per_launch"],
        "avg_launch_us": per[dom]["avg_launch_us"],
        # which of the two durations decided `frac` in THIS run, and whether the committed file still describes these kernels
        # (same fingerprint of the kernel sources as the PMC file's; a file without one reads as stale)
        "duration_source": per[dom]["duration_source"],
        "duration_stale": (prof_sha is None or sha_now is None or prof_sha != sha_now) if prof_file else None,
        "duration_note": (f"committed summary: profiles/{pf} (csrc fingerprint then {prof_sha}, now {sha_now}); "
                          "with duration_source == 'committed' and duration_stale the fraction rests on an outdated file -- the live "
                          "figure beside it is this run's") if prof_file else
                         "no committed rocprofv3 summary of this configuration: the durations are this run's event pairs",
        "duration_method": "avg_launch_us = the LARGER of (a) live_event_pair_minus_empty_us: one HIP event pair around each "
                           "eager launch of the training loop on the launch stream, minus event_pair_empty_us (what a pair with "
                           "nothing in between reads), and (b) rocprofv3_avg_us_committed: the kernel's average in the "
                           "committed rocprofv3 --kernel-trace --stats summary of this configuration"
                           + (f" (profiles/{pf})" if pf else " (none)") +
                           ".  graph_replay_warm_us = 200 back-to-back launches of the kernel alone as a hipGraph between one "
                           "event pair (warm caches, no spare workgroups; single-rank two-launch form only): a lower bound",
        "event_pair_empty_us": round(ev_floor_us, 3),
        "whole_update_tflops": round(FLOP_PER_TRANSITION * a.batch / (ms_per_step * 1e-3) / 1e12, 3),
        "whole_update_frac": round(FLOP_PER_TRANSITION * a.batch / (ms_per_step * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS, 5),
        "kernels_per_update": kp,
        "engine": eng,
        "note": "dominant kernel by time: forward AND backward (dX) of a row slab in one workgroup (4-row slabs on "
                "v_mfma_f32_4x4x1 up to batch 512, 8-row up to 1024, 16-row up to 2048; 32-row slabs on v_mfma_f32_32x32x2 "
                "beyond).  At batch 256: 128 chain workgroups on 256 CUs, 16 dependent layers each, 8 of them 256x256 at "
                "~2.4 us against 2.0 us of LDS-DMA weight streaming per CU: a latency chain bound by the per-CU weight "
                "stream, not by the matrix pipes.  At batch 4096 every CU streams the weights at the ~30 GB/s per CU the L2s "
                "deliver to 256 CUs at once (MI355X_MICROARCH.md ldsdma-fill): 16 flop per streamed byte caps the 32-row "
                "engine at ~70 % of the MFMA peak (DESIGN.md 3.1, 3.3)",
        "all_matrix_kernels": per,
    }
    out["kernel_time_us_per_step_event_bracketed"] = {k: round(1e3 * v["ms_per_step"], 3) for k, v in prof.items()}
    if world > 1:
        return out
    # the HBM-bound half of the path.  In the update loop the gather is fused into the chain kernels; the
    # standalone sampler (replay_buffer.sample: k_draw_plan + k_gather_dict in the reference's float64 dict layout)
    # is timed on its own, after the timed region (it advances the sampler stream)
    dus, gus = C.c_double(), C.c_double()
    buf = r.agent.buffer._dev
    _l.check(r.ctx.lib.hp_buffer_sample_device_us(buf.h, r.rng.h, a.batch, float(r.agent.her_module.future_p),
                                                  float(r.agent.her_module.sq_threshold), 200, C.byref(dus), C.byref(gus)))
    row_doubles = 2 * 27 + 3 * 3 + 4
    bytes_per_tr = row_doubles * 8 + 16 + row_doubles * 8 + 4      # rows read + plan record, dict rows + reward written
    s_gbps = bytes_per_tr * a.batch / (gus.value * 1e-6) / 1e9
    out["roofline_sample_kernel"] = {
        "bound": "hbm", "kernel": "k_gather_dict (gather + relabel + reward, float64 dict layout)",
        "achieved": round(s_gbps, 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(s_gbps / HBM_PEAK_GBPS, 6),
        "avg_launch_us": round(gus.value, 3), "bytes_per_transition": bytes_per_tr, "traffic": None,
        "index_draw_kernel_us": round(dus.value, 3),
        "note": "256 random 0.5 KB rows of a 150 MB buffer per launch: two dependent memory latencies, nowhere near a "
                "bandwidth bound; averages over 200 back-to-back launches between one HIP event pair"}
    out["roofline_sample_kernel_fused"] = sample_kernel_fused_fields(a, r)
    return out


def sample_kernel_fused_fields(a, r):
    """The device-output fused sampler (hp_buffer_sample_dev: gather + relabel + reward + clip + normalise -> float32 x, x', a, r
    in device memory), SURVEY 8d's 528 B / transition kernel.  This build stores float64 rows, so what one launch actually moves
    is 67 x 8 B read + a 16 B index record + 65 x 4 B written = 812 B per transition; both figures are given.  At the bench
    batch the launch is two dependent memory latencies; the large-batch figure shows the kernel against the roof."""
    import ctypes as C

    from rl_arm_under_sparse_reward_amd import _lib as _l
    buf = r.agent.buffer._dev
    fd, fg = C.c_double(), C.c_double()
    fused = {}
    for nb, reps in ((a.batch, 200), (1 << 18, 20)):
        _l.check(r.ctx.lib.hp_buffer_sample_dev_us(buf.h, r.rng.h, r.agent.o_norm.h, r.agent.g_norm.h, nb,
                                                   float(r.agent.her_module.future_p), float(r.agent.her_module.sq_threshold), 200.0, reps, 0,
                                                   C.byref(fd), C.byref(fg)))
        fused[nb] = {"batch": nb, "avg_launch_us": round(fg.value, 3), "index_draw_kernel_us": round(fd.value, 3),
                     "achieved_GBps_528B": round(528 * nb / (fg.value * 1e-6) / 1e9, 2),
                     "achieved_GBps_812B_this_build": round(812 * nb / (fg.value * 1e-6) / 1e9, 2),
                     "transitions_per_s_kernel_only": round(nb / (fg.value * 1e-6), 1)}
    big = fused[1 << 18]
    # ... and the opt-in throughput mode (hp_buffer_enable_f32_rows / hp_buffer_sample_dev_f32: float32 mirror of observations +
    # actions, one timestep per 128-byte line; SURVEY 8b storage_dtype = fp32): 572 B per transition (62 f32 + 6 f64 + 16 read, 260 written)
    f32 = None
    try:
        _l.check(r.ctx.lib.hp_buffer_enable_f32_rows(buf.h))
        _l.check(r.ctx.lib.hp_buffer_sample_dev_us(buf.h, r.rng.h, r.agent.o_norm.h, r.agent.g_norm.h, 1 << 18,
                                                   float(r.agent.her_module.future_p), float(r.agent.her_module.sq_threshold), 200.0, 20, 1,
                                                   C.byref(fd), C.byref(fg)))
        f32 = {"kernel": "k_gather_packed (hp_buffer_sample_dev_f32)", "batch": 1 << 18, "avg_launch_us": round(fg.value, 3),
               "achieved_GBps_528B": round(528 * (1 << 18) / (fg.value * 1e-6) / 1e9, 2),
               "frac_528B": round(528 * (1 << 18) / (fg.value * 1e-6) / 1e9 / HBM_PEAK_GBPS, 5),
               "bytes_per_transition_this_mode": 572,
               "note": "indices, relabelled goals, rewards, goal columns and actions bit-identical to the float64 rows; observation columns "
                       "those of float32-rounded observations (tests/test_gpu_her.py::test_sample_device_f32_rows_throughput_mode)"}
    except Exception as e:      # noqa: BLE001 -- a diagnostic must not cost the run its line
        f32 = {"error": str(e)}
    # ... and the opt-in fast draw (hp_buffer_sample_dev_fast: Philox4x32-10 keyed by (seed, call, transition) inside the gather kernel;
    # SURVEY 8b rng_mode): the WHOLE sample -- index draw included -- as one launch, beside the MT19937 path's draw + gather
    fast = None
    try:
        fu = C.c_double()
        _l.check(r.ctx.lib.hp_buffer_sample_dev_fast_us(buf.h, r.agent.o_norm.h, r.agent.g_norm.h, 1 << 18, float(r.agent.her_module.future_p),
                                                        float(r.agent.her_module.sq_threshold), 200.0, 20, 0, C.byref(fu)))
        fast = {"kernel": "k_gather_fused2<.., fast> (hp_buffer_sample_dev_fast)", "batch": 1 << 18, "whole_sample_us": round(fu.value, 3),
                "mt19937_path_whole_sample_us": round(big["avg_launch_us"] + big["index_draw_kernel_us"], 3),
                "transitions_per_s": round((1 << 18) / (fu.value * 1e-6), 1),
                "note": "not the reference's random stream (opt-in); indices bit-equal to the numpy twin, everything behind them unchanged "
                        "(tests/test_gpu_her.py::test_sample_device_fast_draw_matches_its_oracle_twin)"}
    except Exception as e:      # noqa: BLE001
        fast = {"error": str(e)}
    # PMC traffic of the kernel (separate rocprofv3 --pmc passes, tools/gpu_round6.sh): the committed summary of the 2^18 launch
    traffic, tsrc = None, None
    for rnd in ("r06",):
        path = os.path.join(REPO, "profiles", f"{rnd}_pmc_traffic_sample_fused.json")
        if os.path.exists(path):
            with open(path) as fh:
                doc = json.load(fh)
            for k, v in doc.get("kernels", {}).items():
                if short_kernel(k).startswith("k_gather_fused") and v.get("batch") == (1 << 18):
                    traffic, tsrc = v["hbm_bytes_per_launch"], "profiles/" + os.path.basename(path)
    return {
        "bound": "hbm", "kernel": "k_gather_fused2 (hp_buffer_sample_dev: gather + relabel + reward + clip + normalise -> float32 device tensors; 16-byte loads, two transitions per wavefront instruction)",
        "achieved": big["achieved_GBps_528B"], "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(big["achieved_GBps_528B"] / HBM_PEAK_GBPS, 5),
        "bytes_per_transition": 528, "bytes_per_transition_this_build": 812,
        "achieved_this_build_bytes": big["achieved_GBps_812B_this_build"],
        "frac_this_build_bytes": round(big["achieved_GBps_812B_this_build"] / HBM_PEAK_GBPS, 5),
        "avg_launch_us": big["avg_launch_us"], "batch": 1 << 18, "traffic": traffic, "traffic_source": tsrc,
        "at_bench_batch": fused[a.batch],
        "throughput_mode_f32_rows": f32,
        "fast_draw": fast,
        "note": "achieved = SURVEY 8d's algorithmic 528 B / transition (float32 storage) x 2^18 transitions / the kernel's average "
                "launch time; this build keeps float64 rows (bit-identical rewards and inputs), so the bytes it really moves are "
                "812 B / transition (the *_this_build figures).  Random 432-byte row pairs out of this run's shard "
                f"({a.episodes} episodes = {a.episodes * 29840 / 1e6:.0f} MB of float64 rows: Infinity-Cache resident below 256 MB; "
                "profiles/r06_sample_kernel_shard_sweep.txt has the figure on a larger one).  At the bench batch one launch is "
                "two dependent memory latencies"}


if __name__ == "__main__":
    main()
