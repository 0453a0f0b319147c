"""The direct form of the cycle-opening launch (csrc/cycle_open.hip): hp_agent_train_cycle leaves the cycle's fresh episodes in a
block of a pinned ring and k_cycle_open loads them over the bus itself -- against RLARM_CYCLE_OPEN=copy, the same launch behind an
H2D copy of the episodes into the device staging, as before.  The switch is read by hp_agent_create; each form runs in a fresh child
process (this file, run as a script) with the same seeds, and every comparison is bit for bit: the four buffer arrays, both
normalizers' statistics, the four networks, Adam m / v, the sampler's MT19937 state and the loss log.

Shapes: T = 100, obs 27 / goal 3 / action 4, batch 16, n_batches 2 unless a case says otherwise.
  n1 / n2 / n3   a buffer of 4 episodes is filled, then 8 cycles of n_new = 1 / 2 / 3 fresh episodes each (3: more scatter
                 workgroups).  The oracle replays the random stream on the CPU (slot draw, normalizer plan, minibatch draws): the
                 device's slots equal the oracle's every cycle, the final buffer equals the oracle's, and for n_new >= 2 the seed
                 is ASSERTED to make two staged episodes draw the same slot within the cycles run (store_device.h: later wins).
  six            six cycles of different episodes enqueued back to back with no host synchronisation: the ring (3 blocks) wraps
                 twice (asserted: blocks 1, 2, 0, 1, 2, 0 behind the fill's block 0), so a host write into a block that a queued
                 launch has not read yet shows as other buffer bits.
  grow           the buffer is filled by the eager store_episode + _update_normalizer (which size the device staging for 4
                 episodes but never touch the ring), then n_new = 1, 1, 2, 2, 3, 1: the ring is allocated and then re-allocated
                 twice, and only that moves the buffer's generation, which the cached cycle graphs are keyed on.  ASSERTED from
                 hp_buffer_debug_stage_info after every cycle: block size 1, 1, 2, 2, 3, 3 episodes, generation + 1 at each step up.
  odd            goal 3 / action 3.
  odd_total      T = 7, obs 5 / goal 2 / action 3: 91 doubles per episode, so with n_new = 1 and 3 the block ends in half a
                 16-byte chunk (loaded as 8 bytes: nothing is read past the block).

Shapes at which the launch's loops take further trips (every shape above takes one): a scatter thread of the direct form owns the
16-byte chunks gtid + it * nthreads, it = 0 .. 3, of the block, 2 x 1024 threads per staged episode, so register trip `it` holds
doubles [4096 it, 4096 (it + 1)) of every episode; the normalizer workgroup sums min(256, 49152 / (16 + 8 (obs + goal))) plan rows
per LDS chunk.  TRIPS_AND_CHUNKS states what each case reaches and a test derives it from the shape.  These cases synchronise with
the host after every cycle and are compared with the CPU oracle as well: both normalizers, buffer, slots and random stream.
  wide60         obs 60 / goal 3 / action 7, n_new = 1, 2, 3, 2: 7363 doubles per episode (odd) -- register trips 0 and 1, the half
                 chunk in trip 1 when n_new is odd; two normalizer chunks (94 + 6 rows).
  wide130        130 / 5 / 6, n_new = 1, 3, 2: 14735 doubles -- all four register trips; three normalizer chunks (44 + 44 + 12).
  long300        T = 300 at 27 / 3 / 4 (the slab engine's shape), n_new = 2, 1, 3: 11130 doubles -- trips 0 to 2; chunks 192 + 108,
                 the first of them the launch's largest LDS request (49152 bytes).
  last_fit       152 / 3 / 4, n_new = 1, 2: 16355 doubles, the widest observation that still fits the direct form (16384 doubles
                 per episode is the limit, cycle_open_direct_fits); trip 3 is nearly full.  Normalizer chunks 39 + 39 + 22.
  first_unfit    153 / 3 / 4, n_new = 1, 2: 16456 doubles do not fit, so the "direct" child takes the copy form by itself
                 (ASSERTED: no ring block, no ring bytes) and still computes the oracle's bits.  Chunks 38 + 38 + 24."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, N_BATCHES, SEED, CAP, N_CYCLES = 16, 2, 33, 4, 8
SWITCHES = ("RLARM_CYCLE_OPEN", "RLARM_ENGINE", "RLARM_SPLIT", "RLARM_COMM", "RLARM_UPDATE_GRAPH")
STD = {"obs": 27, "goal": 3, "action": 4, "action_max": 0.5, "max_timesteps": 100}
EAGER_FILL = ("grow",)   # cases whose fill goes through the eager store, not through a cycle
# name: (env_params, [n_new of every cycle after the fill], host synchronisation between cycles)
CASES = {
    "n1": (STD, [1] * N_CYCLES, True),
    "n2": (STD, [2] * N_CYCLES, True),
    "n3": (STD, [3] * N_CYCLES, True),
    "six": (STD, [2] * 6, False),
    "grow": (STD, [1, 1, 2, 2, 3, 1], False),
    "odd": (dict(STD, action=3), [2, 1, 3, 2], False),
    "odd_total": ({"obs": 5, "goal": 2, "action": 3, "action_max": 0.5, "max_timesteps": 7}, [1, 3, 1, 2, 3, 1], False),
    "wide60": (dict(STD, obs=60, action=7), [1, 2, 3, 2], True),
    "wide130": (dict(STD, obs=130, goal=5, action=6), [1, 3, 2], True),
    "long300": (dict(STD, max_timesteps=300), [2, 1, 3], True),
    "last_fit": (dict(STD, obs=152), [1, 2], True),
    "first_unfit": (dict(STD, obs=153), [1, 2], True),
}
# name: (doubles per episode, register trips of the direct form one episode needs, plan rows of every normalizer chunk)
TRIPS_AND_CHUNKS = {
    "wide60": (7363, 2, (94, 6)),
    "wide130": (14735, 4, (44, 44, 12)),
    "long300": (11130, 3, (192, 108)),
    "last_fit": (16355, 4, (39, 39, 22)),
    "first_unfit": (16456, 5, (38, 38, 24)),
}
DIRECT_TRIPS = 4   # STORE_DIRECT_CHUNKS (csrc/stage_block.h): more trips than this do not fit the direct form
ORACLE_CASES = ("n1", "n2", "n3") + tuple(TRIPS_AND_CHUNKS)


def _episodes(case):
    """The fill (CAP episodes) and every cycle's fresh episodes: different values each cycle, the same in both children."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from gpu_common import make_shape_episodes
    p, n_news, _ = CASES[case]
    mk = lambda n, seed: make_shape_episodes(n, p["obs"], p["goal"], p["action"], p["max_timesteps"], seed=seed)   # noqa: E731
    return mk(CAP, 100), [mk(n, 101 + i) for i, n in enumerate(n_news)]


def _oracle(case):
    """The same cycles on the CPU oracle: every cycle's slots, the final store, both normalizers and the random stream."""
    sys.path.insert(0, REPO)
    from oracle.her_replay import EpisodeStore, future_probability
    from oracle.running_norm import RunningNorm, update_normalizers
    p, _, _ = CASES[case]
    T = p["max_timesteps"]
    rs = np.random.RandomState(SEED)
    st = EpisodeStore(T, p["obs"], p["goal"], p["action"], CAP * T)
    on, gn = RunningNorm(p["obs"], default_clip_range=5), RunningNorm(p["goal"], default_clip_range=5)
    fp = future_probability("future", 4)
    fill, cycles = _episodes(case)
    slots = []
    for eps in [fill] + cycles:
        slots.append(np.atleast_1d(np.asarray(st.store_episode(eps, rs), dtype=np.int64)).copy())
        update_normalizers(on, gn, eps, fp, rs)
        for _ in range(N_BATCHES):
            st.sample(BATCH, fp, rs)
    return slots, st, on, gn, rs


def _child(form, out_path):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ctypes as C

    import torch
    from gpu_common import fresh_rng
    from rl_arm_under_sparse_reward_amd import _lib
    from rl_arm_under_sparse_reward_amd.arguments import Args
    from rl_arm_under_sparse_reward_amd.ddpg_agent import (NET_ACTOR, NET_ACTOR_TARGET, NET_CRITIC, NET_CRITIC_TARGET,
                                                            ddpg_agent)
    out = {}
    for name, (params, n_news, sync) in CASES.items():
        for k in SWITCHES:
            os.environ.pop(k, None)
        if form == "copy":
            os.environ["RLARM_CYCLE_OPEN"] = "copy"
        torch.manual_seed(0)
        args = Args(batch_size=BATCH, buffer_size=CAP * params["max_timesteps"])
        assert args.replay_k == 4
        rng = fresh_rng(SEED)
        agent = ddpg_agent(args, None, dict(params), rng=rng)
        fill, cycles = _episodes(name)

        def stage_info():   # host bookkeeping only: no device work, no synchronisation
            gen, nbytes, block = C.c_uint64(), C.c_uint64(), C.c_int32()
            _lib.check(agent.lib.hp_buffer_debug_stage_info(agent.buffer._dev.h, C.byref(gen), C.byref(nbytes), C.byref(block)))
            return [gen.value, nbytes.value, block.value]

        if name in EAGER_FILL:
            agent.buffer.store_episode(fill)
            agent._update_normalizer(fill)
        else:
            agent.train_cycle(fill, N_BATCHES)
        stage = [stage_info()]
        for i, eps in enumerate(cycles):
            agent.train_cycle(eps, N_BATCHES)
            stage.append(stage_info())
            if sync:
                out[f"{name}/slots{i}"] = agent.buffer._dev.last_slots(n_news[i])
        out[f"stage:{name}"] = np.asarray(stage, dtype=np.int64)
        _lib.Context.default().synchronize()
        got = {f"buf_{k}": agent.buffer._dev.read(k) for k in ("obs", "ag", "g", "actions")}
        for tag, nz in (("o", agent.o_norm), ("g", agent.g_norm)):
            for k, v in nz._get().items():
                got[f"{tag}_norm_{k}"] = v
        for tag, slot in (("actor", NET_ACTOR), ("critic", NET_CRITIC), ("actor_target", NET_ACTOR_TARGET),
                          ("critic_target", NET_CRITIC_TARGET)):
            got[tag] = agent._get_flat(slot)
        for tag, slot in (("actor", NET_ACTOR), ("critic", NET_CRITIC)):
            m, v, _ = agent.get_adam_state(slot)
            got[f"m_{tag}"], got[f"v_{tag}"] = m, v
        st = rng.get_state()
        got["rng_key"], got["rng_pos"] = np.asarray(st[1]), np.asarray([st[2]])
        got["losses"] = agent.last_losses((len(cycles) + (name not in EAGER_FILL)) * N_BATCHES)
        for k, v in got.items():
            out[f"{name}/{k}"] = np.asarray(v)
        del agent
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cycle_open_direct")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    res = {}
    for form in ("direct", "copy"):
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", form, str(d / f"{form}.npz")], cwd=REPO,
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert proc.returncode == 0, f"child '{form}' ended with status {proc.returncode}:\n{proc.stdout[-3000:]}"
        res[form] = np.load(d / f"{form}.npz")
    return res


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                                                        np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("case", list(CASES))
def test_direct_form_gives_the_bits_of_the_copy_form(case, runs):
    got, want = runs["direct"], runs["copy"]
    keys = sorted(k for k in want.files if k.startswith(case + "/"))
    assert len(keys) >= 30 and sorted(k for k in got.files if k.startswith(case + "/")) == keys
    for k in keys:
        assert np.all(np.isfinite(want[k])), k
        assert _same_bits(want[k], got[k]), k
    assert np.any(want[f"{case}/losses"] != 0) and np.any(want[f"{case}/buf_obs"] != 0)


@pytest.mark.parametrize("case", ["n1", "n2", "n3"])
def test_slots_and_buffer_match_the_oracle_and_the_seed_collides(case, runs):
    slots, st = _oracle(case)[:2]
    n_news = CASES[case][1]
    if n_news[0] >= 2:   # the later-wins rule is exercised: two staged episodes of one cycle draw the same slot
        assert any(len(set(s.tolist())) < len(s) for s in slots[1:]), [s.tolist() for s in slots]
    for form in ("direct", "copy"):
        for i in range(len(n_news)):
            assert np.array_equal(runs[form][f"{case}/slots{i}"], slots[1 + i]), (form, i)
        for k in ("obs", "ag", "g", "actions"):
            assert _same_bits(runs[form][f"{case}/buf_{k}"], np.asarray(st.buffers[k], dtype=np.float64)), (form, k)


NORM_STATS = ("mean", "std", "total_sum", "total_sumsq", "total_count", "local_sum", "local_sumsq", "local_count")


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_both_forms_give_the_oracles_normalizers_buffer_slots_and_stream(case, runs):
    """The normalizer of the opening launch against the CPU oracle (not only direct against copy, the kernel against itself):
    every statistic of both normalizers after the last cycle, with the buffer, every cycle's slots and the random stream."""
    slots, st, on, gn, rs = _oracle(case)
    n_news = CASES[case][1]
    for form in ("direct", "copy"):
        run = runs[form]
        for tag, ref in (("o", on), ("g", gn)):
            stats = sorted(k.rsplit("_norm_", 1)[1] for k in run.files if k.startswith(f"{case}/{tag}_norm_"))
            assert stats == sorted(NORM_STATS), stats   # everything normalizer._get() returns
            for nm in NORM_STATS:
                assert _same_bits(run[f"{case}/{tag}_norm_{nm}"], np.asarray(getattr(ref, nm))), (form, tag, nm)
        for k in ("obs", "ag", "g", "actions"):
            assert _same_bits(run[f"{case}/buf_{k}"], np.asarray(st.buffers[k], dtype=np.float64)), (form, k)
        for i in range(len(n_news)):
            assert np.array_equal(run[f"{case}/slots{i}"], slots[1 + i]), (form, i)
        key, pos = rs.get_state()[1:3]
        assert np.array_equal(run[f"{case}/rng_key"], np.asarray(key, dtype=np.uint32)) and int(run[f"{case}/rng_pos"][0]) == int(pos), form


def _episode_doubles(case):
    p = CASES[case][0]
    T = p["max_timesteps"]
    return (T + 1) * (p["obs"] + p["goal"]) + T * (p["goal"] + p["action"])


def _episode_bytes(case):
    return 8 * _episode_doubles(case)


@pytest.mark.parametrize("case", list(CASES))
def test_every_case_reaches_the_register_trip_and_chunk_count_it_claims(case):
    """From the shapes' arithmetic alone: the old cases stay within register trip 0 and one normalizer chunk, the new ones reach
    what TRIPS_AND_CHUNKS (and the docstring above) says -- a later change to a shape or to the LDS budget shows here."""
    p = CASES[case][0]
    T, D = p["max_timesteps"], _episode_doubles(case)
    ceil_div = lambda a, b: -(-a // b)   # noqa: E731
    trips = ceil_div(ceil_div(D, 2), 2048)   # 2048 chunks of 16 bytes per episode and trip
    chunk = min(256, 49152 // (16 + 8 * (p["obs"] + p["goal"])))
    n_chunks = ceil_div(T, chunk)
    rows = (chunk,) * (n_chunks - 1) + (T - chunk * (n_chunks - 1),)
    if case not in TRIPS_AND_CHUNKS:
        assert trips == 1 and n_chunks == 1, (D, trips, rows)
        return
    assert (D, trips, rows) == TRIPS_AND_CHUNKS[case]
    assert (trips <= DIRECT_TRIPS) == (case != "first_unfit")
    assert D % 2 == 0 or any(n % 2 for n in CASES[case][1])   # where D is odd, an odd block (half a chunk at its end) occurs
    assert n_chunks >= 2
    # last_fit really is the widest observation that fits at this goal / action / T, first_unfit the next one
    if case == "last_fit":
        assert D + (T + 1) > DIRECT_TRIPS * 4096 >= D


def test_the_ring_really_grows_rotates_and_moves_the_generation(runs):
    """What the grow and six cases rely on, read from the library and not inferred."""
    direct, copy = runs["direct"], runs["copy"]
    for case in CASES:   # the copy form never touches the ring
        st = copy[f"stage:{case}"]
        assert np.all(st[:, 1] == 0) and np.all(st[:, 2] == -1), (case, st.tolist())
    for case in TRIPS_AND_CHUNKS:
        st = direct[f"stage:{case}"]
        if case == "first_unfit":   # too long for the registers: the copy form by itself (its bits: the oracle test above)
            assert np.all(st[:, 1] == 0) and np.all(st[:, 2] == -1), (case, st.tolist())
        else:                       # every cycle, the fill's included, read its episodes from a ring block
            assert np.all(st[:, 2] >= 0) and np.all(st[:, 1] == CAP * _episode_bytes(case)), (case, st.tolist())
    st, ep = direct["stage:grow"], _episode_bytes("grow")
    gen0 = int(st[0, 0])
    assert st[0, 1:].tolist() == [0, -1]                                     # the eager fill: no ring yet
    assert st[1:, 1].tolist() == [ep * n for n in (1, 1, 2, 2, 3, 3)]        # allocated, then re-allocated twice; never shrinks
    assert st[1:, 0].tolist() == [gen0 + k for k in (1, 1, 2, 2, 3, 3)]      # each (re)allocation, and nothing else, moves the generation
    assert st[1:, 2].tolist() == [0, 1, 0, 1, 0, 1]                          # a new ring starts at its first block
    st, ep = direct["stage:six"], _episode_bytes("six")
    assert st[:, 2].tolist() == [0, 1, 2, 0, 1, 2, 0]                        # the fill's cycle, then two wraps
    assert np.all(st[:, 1] == CAP * ep) and np.all(st[:, 0] == st[0, 0])     # sized by the fill; no growth, no new generation
    for case in ("odd", "odd_total"):
        assert np.all(direct[f"stage:{case}"][:, 2] >= 0), case               # these shapes take the direct form


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2], sys.argv[3])
