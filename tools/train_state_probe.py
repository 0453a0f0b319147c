#!/usr/bin/env python
"""What a training-state capture costs the learner, and how fast the state moves (profiles/r07_train_state.txt).

    python tools/train_state_probe.py cycles [--root TREE] [--capture N] us per training cycle (40 updates, batch 256, 5000-episode
                                                                  buffer): plain, or with a capture issued behind every N-th
                                                                  cycle (the previous ticket is retired first: one capture at
                                                                  a time, so N = 1 waits for each drain)
    python tools/train_state_probe.py state                       checksum kernel GB/s on the buffer section, wall time of a full
                                                                  save and a full load at that size

    python tools/train_state_probe.py delta [--root TREE]         full against delta saves at that size (profiles/
                                                                  train_state_delta.json): the learner-stream part of a capture
                                                                  (enqueue until the learner's stream is idle again) and
                                                                  capture-to-file, for a full state and -- where the tree has
                                                                  them -- for a delta with --dirty episodes stored since the base

--root TREE imports the package from another checkout (e.g. the parent commit, built), so that (a) parent, (b) this commit without a
capture and (c) with captures are measured by the same script; each prints one JSON line.  Every figure is the median over
--repeats timed blocks, with the min..max spread next to it.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np


def fingerprint(root):
    """sha256 over the sources that decide the numbers (csrc, the binding, this script)."""
    h = hashlib.sha256()
    pkg = os.path.join(root, "rl_arm_under_sparse_reward_amd")
    files = [os.path.join(pkg, "csrc", f) for f in sorted(os.listdir(os.path.join(pkg, "csrc"))) if f.endswith((".hip", ".h", ".inc"))]
    files += [os.path.join(pkg, "_lib.py"), os.path.join(pkg, "ddpg_agent.py")]
    for f in files:
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def make_agent(n_fill, batch=256):
    import torch
    from rl_arm_under_sparse_reward_amd.arguments import Args
    from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
    from rl_arm_under_sparse_reward_amd.random import DeviceRandomState
    from rl_arm_under_sparse_reward_amd.synthetic import ENV_PARAMS, make_episodes
    args = Args(batch_size=batch)                      # buffer_size 5e5 transitions = 5000 episodes of 100 steps
    torch.manual_seed(0)
    agent = ddpg_agent(args, None, dict(ENV_PARAMS), rng=DeviceRandomState(7))
    left = n_fill
    while left > 0:
        k = min(left, 500)
        agent.buffer.store_episode(make_episodes(k, seed=left, mode="walk"))
        left -= k
    return agent, make_episodes(2, seed=1, mode="walk")


def spread(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2), "n": len(xs)}


def run_cycles(a):
    agent, eps = make_agent(a.episodes)
    lib, ticket, nbytes = agent.lib, C.c_uint64(), C.c_size_t()
    have = False

    count = 0

    def cycle():
        nonlocal have, count
        agent.train_cycle(eps)
        count += 1
        if a.capture and count % a.capture == 0:
            if have:      # retire the previous ticket (its drain overlapped the cycle just enqueued), then capture again
                assert lib.hp_state_fetch(agent.h, ticket.value, 1, None, 0, None, None) == 0
            assert lib.hp_state_capture(*agent._handles(), C.byref(ticket), C.byref(nbytes)) == 0
            have = True

    for _ in range(a.warmup):
        cycle()
    agent.ctx.synchronize()
    per = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.cycles):
            cycle()
        agent.ctx.synchronize()
        per.append((time.perf_counter() - t0) / a.cycles * 1e6)
    out = {"probe": "cycles", "capture_every_n_cycles": int(a.capture), "root": a.root or ".", "source": fingerprint(a.root or REPO),
           "episodes": a.episodes, "batch": 256, "updates_per_cycle": int(agent.args.n_batches), "us_per_cycle": spread(per),
           "captured_bytes": int(nbytes.value)}
    print(json.dumps(out))


def run_state(a):
    from rl_arm_under_sparse_reward_amd import train_state as ts
    agent, _ = make_agent(a.episodes)
    dev = agent.buffer._dev
    import torch
    n = a.episodes * 101 * 27 * 8                       # the buffer_obs section
    t = torch.empty(n, dtype=torch.uint8, device=f"cuda:{agent.ctx.device_id}")
    t.copy_(torch.from_numpy(dev.read("obs", 0, a.episodes).view(np.uint8).reshape(-1)))
    torch.cuda.synchronize()
    out2, gbs = (C.c_uint64 * 2)(), []
    for i in range(a.repeats + 2):
        t0 = time.perf_counter()
        assert agent.lib.hp_state_checksum_dev(agent.ctx.h, C.c_void_p(t.data_ptr()), n, 0, out2) == 0
        if i >= 2:
            gbs.append(n / (time.perf_counter() - t0) / 1e9)     # host wall clock around launch + 16-byte read-back: a lower bound
    saves, loads = [], []
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "state.npz")
        for _ in range(a.repeats):
            t0 = time.perf_counter(); agent.save_training_state(path); saves.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); agent.load_training_state(path); loads.append((time.perf_counter() - t0) * 1e3)
        size = os.path.getsize(path)
        t0 = time.perf_counter(); ts.verify(path); verify_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"probe": "state", "source": fingerprint(REPO), "episodes": a.episodes, "checksum_bytes": n,
                      "checksum_GBps_host_clock": spread(gbs), "hbm_peak_GBps_spec": 8000, "file_bytes": size,
                      "save_ms": spread(saves), "load_ms": spread(loads), "verify_cpu_ms": round(verify_ms, 1)}))


def run_delta(a):
    agent, eps = make_agent(a.episodes)
    lib, ticket, nbytes = agent.lib, C.c_uint64(), C.c_size_t()
    has_delta = hasattr(object.__getattribute__(lib, "_cdll"), "hp_state_capture_delta")

    def learner_part(capture):
        """ms from the capture call until the learner's stream is idle again; the ticket is abandoned outside the clock"""
        out = []
        for _ in range(a.repeats + 1):
            agent.ctx.synchronize()
            t0 = time.perf_counter()
            assert capture() == 0
            agent.ctx.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
            assert lib.hp_state_fetch(agent.h, ticket.value, 1, None, 0, None, None) == 0
        return spread(out[1:])

    def to_file(path, **kw):
        out = []
        for _ in range(a.repeats + 1):
            agent.ctx.synchronize()
            t0 = time.perf_counter(); agent.save_training_state(path, **kw); out.append((time.perf_counter() - t0) * 1e3)
        return spread(out[1:])

    res = {"probe": "delta", "root": a.root or ".", "source": fingerprint(a.root or REPO), "episodes": a.episodes, "T": 100}
    with tempfile.TemporaryDirectory() as d:
        base = os.path.join(d, "state.npz")
        res["full"] = {"learner_stream_ms": learner_part(lambda: lib.hp_state_capture(*agent._handles(), C.byref(ticket), C.byref(nbytes))),
                       "captured_bytes": int(nbytes.value), "capture_to_file_ms": to_file(base), "file_bytes": os.path.getsize(base)}
        if has_delta:
            from rl_arm_under_sparse_reward_amd import train_state as ts
            for _ in range(a.dirty // 2):
                agent.train_cycle(eps)
            since = ts.known_base(agent, base)[1]
            res["delta"] = {"episodes_stored_since_base": a.dirty // 2 * 2,
                            "learner_stream_ms": learner_part(lambda: lib.hp_state_capture_delta(
                                *agent._handles(), since, a.dirty // 2 * 2, C.byref(ticket), C.byref(nbytes))),
                            "captured_bytes": int(nbytes.value)}
            path = os.path.join(d, "state.delta.npz")
            res["delta"]["capture_to_file_ms"] = to_file(path, base=base)
            res["delta"]["file_bytes"] = os.path.getsize(path)
            res["delta"]["n_dirty"] = int(ts.read_manifest(path)["n_dirty"])
            t0 = time.perf_counter(); ts.compose(base, path); res["delta"]["compose_cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(res))


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("probe", choices=["cycles", "state", "delta"])
    p.add_argument("--root", default=None)
    p.add_argument("--capture", type=int, default=0, help="capture behind every N-th cycle (0: never)")
    p.add_argument("--episodes", type=int, default=5000)
    p.add_argument("--cycles", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--dirty", type=int, default=100, help="delta: episodes stored since the base (two per cycle)")
    a = p.parse_args()
    sys.path.insert(0, os.path.abspath(a.root) if a.root else REPO)
    {"cycles": run_cycles, "state": run_state, "delta": run_delta}[a.probe](a)
