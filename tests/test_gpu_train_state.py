"""Training state on the device (csrc/state.hip, train_state.py): a run that is stopped, saved and continued by fresh objects is
BIT-identical to the run that never stopped; roll-back on a live agent; captures that do not see later work; refusals that leave
the receiver untouched; the checksum kernel against its numpy twin.  Everything goes through the C ABI via ctypes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from gpu_common import ENV_PARAMS, ctx, fresh_rng, state_equal
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd import train_state as ts
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_CRITIC, ddpg_agent
from rl_arm_under_sparse_reward_amd.synthetic import PointMassGoalEnv
from train_state_common import EPS_PER_CYCLE, N_BATCHES, assert_same, build, cycles, fingerprint

pytestmark = pytest.mark.gpu


CASES = {
    "b256_split": dict(batch=256),
    "b1024_no_split": dict(batch=1024),
    "layers_engine": dict(batch=256, env={"RLARM_ENGINE": "layers"}),
    "overflowing_buffer": dict(batch=256, cap_eps=5),
    "shape_13_3_4_T50": dict(batch=256, ep={"obs": 13, "goal": 3, "action": 4, "action_max": 0.7, "max_timesteps": 50}),
    "shape_20_1_3_T50": dict(batch=256, ep={"obs": 20, "goal": 1, "action": 3, "action_max": 0.7, "max_timesteps": 50}),
    "shape_25_2_5_layers": dict(batch=256, ep={"obs": 25, "goal": 2, "action": 5, "action_max": 1.3, "max_timesteps": 50}),
    "f32_rows": dict(batch=256, f32=True),
    # another hidden width (layer engine), small: 2 + 2 cycles of 3 updates, 16 episodes of room
    "hidden_128": dict(batch=64, cap_eps=16, ep=dict(ENV_PARAMS, hidden=128), n=2, m=2, n_batches=3),
}


@pytest.mark.parametrize("case", list(CASES))
def test_resume_equals_not_stopping(case, tmp_path, monkeypatch):
    c = dict(CASES[case])
    for k, v in c.pop("env", {}).items():
        monkeypatch.setenv(k, v)
    ep, n, m, nb = c.get("ep"), c.get("n", 3), c.get("m", 2), c.get("n_batches", N_BATCHES)
    kw = dict(batch=c["batch"], ep=ep, cap_eps=c.get("cap_eps", 40), f32=c.get("f32", False), n_batches=nb)
    a = build(**kw)
    form = C.c_int32()
    _lib.check(a.lib.hp_agent_update_form(a.h, nb, C.byref(form)))
    if case == "b256_split":
        assert form.value == 1
    if case in ("b1024_no_split", "layers_engine", "shape_25_2_5_layers", "hidden_128"):
        assert form.value == 0
    cycles(a, ep, 0, n + m)
    want, want_losses = fingerprint(a), a.last_losses(m * nb)
    if case == "overflowing_buffer":
        assert want["buffer_counters"][0] == 5 and want["buffer_counters"][1] == (n + m) * EPS_PER_CYCLE * 100
    # run B: n cycles, save, drop everything, fresh objects that start from other weights and another stream, load, m cycles
    b = build(**kw)
    cycles(b, ep, 0, n)
    path = b.save_training_state(tmp_path / "state.npz", epoch=1, cycle=n)
    manifest = ts.verify(path)                        # the numpy twin agrees with the sums the device put into the manifest
    assert manifest["dims"]["hidden"] == (ep or {}).get("hidden", 256)
    if case == "hidden_128":
        assert b.engine()["engine"] == "layers" and b.actor_network.fc2.weight.shape == (128, 128)
        wide = build(torch_seed=5, rng_seed=11, **dict(kw, ep=None))          # a 256-wide agent refuses the 128-wide state, untouched
        fp = fingerprint(wide)
        with pytest.raises(ValueError, match="hidden of the state is 128"):
            wide.load_training_state(path)
        assert_same(fingerprint(wide), fp, "refused width")
        del wide
    del b
    b2 = build(torch_seed=99, rng_seed=4321, **kw)
    before = fingerprint(b2)
    assert before["actor"].tobytes() != want["actor"].tobytes() and before["rng_key"].tobytes() != want["rng_key"].tobytes()
    assert b2.load_training_state(path) == b"" and b2.resumed_at == (1, n)
    with pytest.raises(_lib.HpError, match="only 0 updates logged"):      # the loss log is not part of a state
        b2.last_losses(1)
    cycles(b2, ep, n, m)
    assert_same(fingerprint(b2), want, case)
    assert b2.last_losses(m * nb).tobytes() == want_losses.tobytes()
    if c.get("f32"):
        sa = a.buffer.sample_device(256, a.o_norm, a.g_norm, f32_rows=True)
        sb = b2.buffer.sample_device(256, b2.o_norm, b2.g_norm, f32_rows=True)
        for k in sa:
            assert torch.equal(sa[k].view(torch.int32), sb[k].view(torch.int32)), k
        assert state_equal(b2.rng, *a.rng.get_state()[1:3])


def golden_args(g, tmp_path, sub, n_epochs):
    c = {k: (float(v) if "." in v else int(v)) for k, v in g["cfg"]}
    args = Args(n_epochs=n_epochs, n_cycles=c["n_cycles"], n_batches=c["n_batches"], n_test_rollouts=c["n_test_rollouts"],
                noise_eps=c["noise_eps"], random_eps=c["random_eps"], buffer_size=c["buffer_episodes"] * 100,
                save_dir=str(tmp_path / sub), env_name="stand_in")
    return c, args


def golden_agent(g, args, env, rng_seed, stored):
    agent = ddpg_agent(args, env, env.env_params, rng=fresh_rng(rng_seed))
    orig = agent.train_cycle
    agent.train_cycle = lambda eps, n_batches=None: (stored.append([np.array(a) for a in eps]), orig(eps, n_batches))[1]
    return agent


def test_stitched_learn_follows_the_reference_run_and_equals_the_uninterrupted_one(tmp_path):
    """learn() stopped after epoch 1 (args.state_path) and continued by a NEW agent (args.resume) against
    tests/golden/rollout.npz -- every assertion of test_gpu_rollout.test_learn_follows_the_reference_run_on_the_stand_in_env with its
    tolerances -- and against this build's uninterrupted run, bitwise."""
    from conftest import load_golden
    g = load_golden("rollout.npz")
    # the uninterrupted run
    c, args_u = golden_args(g, tmp_path, "u", None)
    args_u.n_epochs = c["n_epochs"]
    env_u = PointMassGoalEnv(seed=c["env_seed"], max_timesteps=100, distance_threshold=c["distance_threshold"])
    torch.manual_seed(0)
    stored_u = []
    u = golden_agent(g, args_u, env_u, 0, stored_u)
    u._set_flat(NET_ACTOR, g["init_actor"]); u._set_flat(NET_CRITIC, g["init_critic"])
    u.lib.hp_agent_sync_targets(u.h)
    np.random.seed(c["np_seed"])
    u.learn()
    # the stitched run: epoch 1 ...
    assert c["n_epochs"] == 2
    _, args1 = golden_args(g, tmp_path, "s", 1)
    args1.state_path = str(tmp_path / "run.npz")
    env = PointMassGoalEnv(seed=c["env_seed"], max_timesteps=100, distance_threshold=c["distance_threshold"])
    torch.manual_seed(0)
    stored = []
    first = golden_agent(g, args1, env, 0, stored)
    first._set_flat(NET_ACTOR, g["init_actor"]); first._set_flat(NET_CRITIC, g["init_critic"])
    first.lib.hp_agent_sync_targets(first.h)
    np.random.seed(c["np_seed"])
    first.learn()
    assert os.path.exists(tmp_path / "run_rank0.npz") and ts.verify(tmp_path / "run_rank0.npz")["epoch"] == 1
    del first
    # ... the process "dies": numpy's stream is lost, a new agent with other weights and another device stream continues (the test
    # keeps the env object alive: the simulator is the caller's)
    np.random.seed(987654)
    _, args2 = golden_args(g, tmp_path, "s", c["n_epochs"])
    args2.resume = str(tmp_path / "run.npz")
    torch.manual_seed(31)
    agent = golden_agent(g, args2, env, 77, stored)
    agent.learn()
    # the reference's run (the assertions of test_learn_follows_the_reference_run_on_the_stand_in_env)
    assert len(stored) == c["n_epochs"] * c["n_cycles"]
    for i, batch in enumerate(stored):
        tol = 2e-6 if i == 0 else 2e-4
        for nm, a in zip(("obs", "ag", "g", "actions"), batch):
            want = g[f"cycle{i}_{nm}"].astype(np.float64)
            assert a.shape == want.shape and float(np.abs(a - want).max()) <= tol, (i, nm, float(np.abs(a - want).max()))
    key, pos = np.random.get_state()[1:3]
    assert np.array_equal(key, g["key"]) and pos == int(g["pos"])
    assert state_equal(agent.rng, g["key"], g["pos"])
    assert np.allclose(agent.success_rates, g["success_rates"], atol=1.0 / c["n_test_rollouts"] + 1e-9)
    assert np.allclose(agent.o_norm.mean, g["o_mean"], atol=1e-5) and np.allclose(agent.g_norm.std, g["g_std"], atol=1e-5)
    rel = np.linalg.norm(agent._get_flat(NET_ACTOR) - g["actor_final"]) / np.linalg.norm(g["actor_final"] - g["init_actor"])
    assert rel <= 0.1, rel
    assert sorted(p.name for p in (tmp_path / "s" / "stand_in").iterdir()) == list(g["checkpoints"])
    # this build's uninterrupted run, bitwise
    assert_same(fingerprint(agent), fingerprint(u), "stitched vs uninterrupted")
    assert agent.success_rates == u.success_rates and len(agent.success_rates) == c["n_epochs"]
    assert sorted(p.name for p in (tmp_path / "u" / "stand_in").iterdir()) == sorted(p.name for p in (tmp_path / "s" / "stand_in").iterdir())
    for i, (x, y) in enumerate(zip(stored, stored_u)):
        for p, q in zip(x, y):
            assert p.tobytes() == q.tobytes(), i


@pytest.mark.parametrize("batch", [256, 1024])
def test_roll_back_on_a_live_agent_replays_the_same_cycles(batch, tmp_path):
    """Save after cycle n, 3 more cycles, load into the SAME agent, the same 3 cycles again: identical bits (the cached cycle
    graph is replayed across the restore -- nothing it baked in is stale)."""
    a = build(batch=batch, cap_eps=7)                  # the repeated cycles overflow the buffer: random slots, too
    cycles(a, None, 0, 2)
    path = a.save_training_state(tmp_path / "s.npz")
    at_save = fingerprint(a)
    mode = C.c_int32()
    cycles(a, None, 2, 3)
    once, once_losses = fingerprint(a), a.last_losses(3 * N_BATCHES)
    _lib.check(a.lib.hp_agent_cycle_mode(a.h, C.byref(mode)))
    assert mode.value == 1
    a.load_training_state(path)
    assert_same(fingerprint(a), at_save, "restored")
    cycles(a, None, 2, 3)
    _lib.check(a.lib.hp_agent_cycle_mode(a.h, C.byref(mode)))
    assert mode.value == 1
    assert_same(fingerprint(a), once, "second pass")
    assert a.last_losses(3 * N_BATCHES).tobytes() == once_losses.tobytes()


def test_capture_does_not_see_later_work_and_second_capture_is_refused(tmp_path):
    x = build()
    cycles(x, None, 0, 2)
    sync_path = x.save_training_state(tmp_path / "sync.npz")
    y = build()
    cycles(y, None, 0, 2)
    h = y.save_training_state(tmp_path / "async.npz", wait=False)
    assert not os.path.exists(tmp_path / "async.npz")
    with pytest.raises(_lib.HpError, match="has not been fetched yet"):      # documented: one capture at a time, HP_ERR_STATE
        y.save_training_state(tmp_path / "second.npz")
    assert not os.path.exists(tmp_path / "second.npz")
    cycles(y, None, 2, 2)                                                   # training goes on; the snapshot must not move
    y.ctx.synchronize()
    assert h.result() == str(tmp_path / "async.npz") and h.done()
    (wa, wm), (ga, gm) = ts.read_state(sync_path), ts.read_state(tmp_path / "async.npz")
    assert_same(ga, wa, "async vs sync file")
    assert gm == wm
    # the later work did happen, and the next capture is accepted again
    cycles(x, None, 2, 2)
    assert_same(fingerprint(y), fingerprint(x), "after the capture")
    ts.verify(y.save_training_state(tmp_path / "third.npz"))


def test_refusals_leave_the_receiver_untouched(tmp_path):
    src = build()
    cycles(src, None, 0, 2)
    good = src.save_training_state(tmp_path / "good.npz")
    arrays, manifest = ts.read_state(good)
    recv = build(torch_seed=5, rng_seed=11)
    cycles(recv, None, 10, 1)
    before = fingerprint(recv)

    def refused(agent, path, match, fp):
        with pytest.raises(ValueError, match=match):
            agent.load_training_state(path)
        assert_same(fingerprint(agent), fp, match)

    # rank / world size
    for key, val in (("rank", 1), ("world_size", 2)):
        m = dict(manifest); m[key] = val
        refused(recv, ts.write_state(tmp_path / f"{key}.npz", arrays, m), key, before)
    # one corrupted buffer byte under a manifest that describes the ORIGINAL data: only the device-side sums can notice
    bad = dict(arrays)
    raw = arrays["buffer_obs"].copy().view(np.uint8).reshape(-1)
    raw[len(raw) // 2 + 3] ^= 0x04
    bad["buffer_obs"] = raw.view(np.float64).reshape(arrays["buffer_obs"].shape)
    refused(recv, ts.write_state(tmp_path / "corrupt.npz", bad, manifest), "checksum of 'buffer_obs' on the device", before)
    # ... and a flipped bit in the optimizer state
    bad = dict(arrays)
    raw = arrays["adam_critic_v"].copy().view(np.uint8)
    raw[-1] ^= 0x80
    bad["adam_critic_v"] = raw.view(np.float32)
    refused(recv, ts.write_state(tmp_path / "corrupt2.npz", bad, manifest), "checksum of 'adam_critic_v' on the device", before)
    # wrong capacity, wrong dims, wrong T
    other = build(cap_eps=41, torch_seed=5, rng_seed=11)
    refused(other, good, "capacity", fingerprint(other))
    ep = {"obs": 13, "goal": 3, "action": 4, "action_max": 0.5, "max_timesteps": 100}
    other = build(ep=ep, torch_seed=5, rng_seed=11)
    refused(other, good, "obs of the state is 27", fingerprint(other))
    # the library itself names the field when a host skips the Python checks
    secs, total = ts._layout(recv, manifest["dims"]["current_size"])
    blob = np.zeros(total, np.uint8)
    sums = (C.c_uint64 * (2 * _lib.STATE_SECTIONS))()
    d = manifest["dims"]
    for field, msg in (("T", "T of the state is 101"), ("capacity", "capacity of the state is 41"), ("hidden", "hidden of the state is 257")):
        kw = dict(obs_dim=d["obs"], goal_dim=d["goal"], act_dim=d["action"], hidden=d["hidden"], T=d["T"], reserved=0,
                  capacity=d["capacity"], current_size=d["current_size"])
        kw[field] += 1
        with pytest.raises(ValueError, match=msg):
            _lib.check(recv.lib.hp_state_restore(*recv._handles(), C.byref(_lib.StateDims(**kw)), blob.ctypes.data_as(C.c_void_p),
                                                 blob.size, sums))
    assert_same(fingerprint(recv), before, "after the library's refusals")
    # the receiver still works, and takes the good file
    recv.load_training_state(good)
    assert_same(fingerprint(recv), fingerprint(src), "good file")


def test_the_librarys_section_table_is_pythons_for_both_kinds():
    """hp_state_layout / hp_state_layout_delta against expected_shapes / delta_shapes, at a shape where obs, goal, action, T, T + 1
    and the hidden width all differ: names in order, dtype and count of every section, and the offsets -- multiples of 256, each
    the one before plus that section's bytes padded to 256 (so they increase wherever a section holds anything: with room for no
    episode the row sections are empty and share an offset), the total closing the last.  No training."""
    ep = {"obs": 13, "goal": 3, "action": 4, "action_max": 0.7, "max_timesteps": 50, "hidden": 128}
    agent = build(batch=64, ep=ep, cap_eps=16, n_batches=3)

    def padded(dt, count):
        return (count * np.dtype(dt).itemsize + 255) // 256 * 256

    def check(secs, total, want, what):
        assert [s[0] for s in secs] == list(want), what
        for name, dt, count, _ in secs:
            assert (dt, count) == (want[name][0], int(np.prod(want[name][1]))), (what, name)
        offs = [s[3] for s in secs]
        assert offs[0] == 0 and all(o % 256 == 0 for o in offs), what
        for (name, dt, count, off), nxt in zip(secs, offs[1:] + [total]):
            assert nxt == off + padded(dt, count) and (nxt > off or count == 0), (what, name)

    fulls = []
    for cs in (0, 1, 16):
        secs, total = ts._layout(agent, cs)
        assert len(secs) == _lib.STATE_SECTIONS
        check(secs, total, ts.expected_shapes(ts._dims_of(agent, cs)), f"full, current_size {cs}")
        fulls.append(secs)
    for max_dirty in (0, 1, 16):
        dims = ts._dims_of(agent, 16)
        full = ts.expected_shapes(dims)
        want = {k: v for k, v in full.items() if k not in ts.BUFFER_ARRAYS + ("buffer_counters",)}
        want["buffer_delta_header"] = ("<i8", (4,))
        want.update(ts.delta_shapes(dims, max_dirty))
        want["buffer_counters"] = full["buffer_counters"]
        secs, total = ts._layout(agent, max_dirty, delta=True)
        assert len(secs) == _lib.STATE_DELTA_SECTIONS
        check(secs, total, want, f"delta, max_dirty {max_dirty}")
        for f in fulls:                                # the small sections: a full state's, entry for entry
            assert secs[:27] == f[:27] and secs[26][0] == "rng_pos"


@pytest.mark.parametrize("nbytes", [0, 1, 8, 4096 + 3, (64 << 20) + 5])
def test_checksum_kernel_equals_the_numpy_twin(nbytes):
    c = ctx()
    torch.manual_seed(nbytes % 1000)
    t = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=f"cuda:{c.device_id}")
    torch.cuda.synchronize()
    want = ts.checksum(t.cpu().numpy())
    out = (C.c_uint64 * 2)()
    for blocks in (0, 1, 7, 1000):                 # the sums are associative: the launch shape does not matter
        _lib.check(c.lib.hp_state_checksum_dev(c.h, C.c_void_p(t.data_ptr() if nbytes else 0), nbytes, blocks, out))
        assert (int(out[0]), int(out[1])) == want, (nbytes, blocks)
    if nbytes > 64:                                # a section that starts 8 mod 16
        want8 = ts.checksum(t[8:].cpu().numpy())
        _lib.check(c.lib.hp_state_checksum_dev(c.h, C.c_void_p(t.data_ptr() + 8), nbytes - 8, 0, out))
        assert (int(out[0]), int(out[1])) == want8
