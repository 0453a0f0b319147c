"""Delta training states on the device (csrc/state.hip, train_state.py): base + delta restore exactly what a full state taken at
the same instant restores -- through cycle graphs first captured BEFORE the base was saved, which is the pitfall per-slot stamps
read from device memory exist for --, the dirty set is exactly the slots the library reports having written, resume through
base + delta equals not stopping, capture semantics, refusals that leave the receiver untouched, and the dirty scan alone."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from gpu_common import ctx, fresh_rng
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd import train_state as ts
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
from rl_arm_under_sparse_reward_amd.synthetic import make_episodes
from train_state_common import EPS_PER_CYCLE, N_BATCHES, assert_same, build, cycles, episodes, fingerprint

pytestmark = pytest.mark.gpu


def last_slots(agent, n=EPS_PER_CYCLE):
    out = np.empty(n, np.int64)
    _lib.check(agent.lib.hp_buffer_last_slots(agent.buffer._dev.h, _lib.ptr(out, C.c_int64), n))
    return out


def episode_bytes(d):
    return 8 * ((d["T"] + 1) * (d["obs"] + d["goal"]) + d["T"] * (d["goal"] + d["action"]))


def check_delta_file(path):
    """The byte count of a delta's row arrays is exactly n_dirty x episode bytes; the slot list is ascending."""
    arrays, m = ts.read_state(path)
    assert m["kind"] == "delta" and m["format"] == ts.DELTA_FORMAT_VERSION
    assert sum(arrays[n].nbytes for n in ts.DELTA_ROW_ARRAYS) == m["n_dirty"] * episode_bytes(m["dims"])
    assert arrays["buffer_delta_slots"].shape == (m["n_dirty"],) and np.all(np.diff(arrays["buffer_delta_slots"]) > 0)
    return arrays, m


def assert_composes_to(base, delta, full, what=""):
    """compose(base, delta) equals the full state `full` in every device array (buffer_counters among them)."""
    got, gm = ts.compose(base, delta)
    want, wm = ts.read_state(full)
    for name in ts.DEVICE_ARRAYS:
        x, y = got[name], want[name]
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, name)
        assert gm["arrays"][name] == wm["arrays"][name], (what, name)
    assert gm["dims"] == wm["dims"]
    return got, gm


def base_delta_full(agent, tmp_path, step, n, m, between=None):
    """n steps, full save A, [between()], m steps, delta D against A, at once a full save F."""
    for i in range(n):
        step(agent, i)
    a_path = agent.save_training_state(tmp_path / "A.npz")
    if between:
        between(agent)
    for i in range(n, n + m):
        step(agent, i)
    d_path = agent.save_training_state(tmp_path / "D.npz", base=a_path)
    f_path = agent.save_training_state(tmp_path / "F.npz")
    return a_path, d_path, f_path


SHAPE_20_1_3 = {"obs": 20, "goal": 1, "action": 3, "action_max": 0.7, "max_timesteps": 50}
CASES = {
    "growing_cap40": dict(cap_eps=40, n=3, m=3),
    "full_cap12": dict(cap_eps=12, n=7, m=3),                      # filled, then overwritten at random slots
    "tiny_full_cap5": dict(cap_eps=5, n=3, m=3),                   # nearly everything dirty; repeated slots within a store occur
    "f32_rows": dict(cap_eps=12, n=5, m=3, f32=True),
    "shape_20_1_3_T50": dict(cap_eps=12, n=5, m=3, ep=SHAPE_20_1_3),
    "layers_engine": dict(cap_eps=12, n=5, m=3, env={"RLARM_ENGINE": "layers"}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_delta_plus_base_equals_full(case, tmp_path, monkeypatch):
    c = dict(CASES[case])
    for k, v in c.pop("env", {}).items():
        monkeypatch.setenv(k, v)
    ep = c.get("ep")
    agent = build(ep=ep, cap_eps=c["cap_eps"], f32=c.get("f32", False))
    written = []

    def step(a, i):
        a.train_cycle(episodes(ep, i))
        if i == c["n"] - 1 and case == "growing_cap40":
            mode = C.c_int32()
            _lib.check(a.lib.hp_agent_cycle_mode(a.h, C.byref(mode)))
            assert mode.value == 1                                  # the cycle graph is cached before save A
        if i >= c["n"]:
            written.append(last_slots(a))
    a_path, d_path, f_path = base_delta_full(agent, tmp_path, step, c["n"], c["m"])
    arrays, m = check_delta_file(d_path)
    assert_composes_to(a_path, d_path, f_path, case)
    # the dirty set, from the slots the library itself reports (test 2 asserts more on the capacity-12 case)
    assert np.array_equal(arrays["buffer_delta_slots"], np.unique(np.concatenate(written)))
    cs0, cs = ts.read_manifest(a_path)["dims"]["current_size"], m["dims"]["current_size"]
    assert m["base"]["current_size"] == cs0 and cs == min(c["cap_eps"], (c["n"] + c["m"]) * EPS_PER_CYCLE)
    if case == "tiny_full_cap5":
        assert m["n_dirty"] >= 3
    assert ts.verify(d_path)["n_dirty"] == m["n_dirty"] and os.path.getsize(d_path) < os.path.getsize(f_path)


def test_delta_covers_a_store_outside_a_cycle(tmp_path):
    """buffer.store_episode after A (a demo preload): the eager scatter stamps like the cycle's."""
    agent = build(cap_eps=12)
    demo = []

    def preload(a):
        a.buffer.store_episode(make_episodes(3, seed=55, mode="walk"))
        demo.append(last_slots(a, 3))
    a_path, d_path, f_path = base_delta_full(agent, tmp_path, lambda a, i: a.train_cycle(episodes(None, i)), 5, 1, between=preload)
    arrays, m = check_delta_file(d_path)
    assert_composes_to(a_path, d_path, f_path, "store_episode")
    assert set(demo[0]) | set(last_slots(agent)) == set(arrays["buffer_delta_slots"])


def test_delta_covers_device_rollouts(tmp_path):
    """collect_episodes_device + train_cycle with PointMassVecEnv: the device-block path (hp_agent_train_cycle_dev)."""
    from rl_arm_under_sparse_reward_amd.device_env import PointMassVecEnv
    T = 50
    env = PointMassVecEnv(EPS_PER_CYCLE, seed=4, device="cuda:0", max_timesteps=T)
    torch.manual_seed(0)
    agent = ddpg_agent(Args(batch_size=256, buffer_size=12 * T, n_batches=N_BATCHES), env, env.env_params, rng=fresh_rng(12))
    written = []

    def step(a, i):
        a.train_cycle(a.collect_episodes_device())
        if i >= 7:
            written.append(last_slots(a))
    a_path, d_path, f_path = base_delta_full(agent, tmp_path, step, 7, 2)
    arrays, _ = check_delta_file(d_path)
    assert_composes_to(a_path, d_path, f_path, "device rollouts")
    assert np.array_equal(arrays["buffer_delta_slots"], np.unique(np.concatenate(written)))


def test_the_dirty_set_is_exact(tmp_path):
    """Capacity 12, full: the delta's slot list is the sorted unique union of the slots hp_buffer_last_slots reported after every
    store since A -- a reference computed on the host from what the library already reports -- and smaller than the buffer."""
    agent = build(cap_eps=12)
    cycles(agent, None, 0, 7)
    a_path = agent.save_training_state(tmp_path / "A.npz")
    seen = []
    for i in range(7, 10):
        cycles(agent, None, i, 1)
        seen.append(last_slots(agent))
    arrays, m = check_delta_file(agent.save_training_state(tmp_path / "D.npz", base=a_path))
    want = np.unique(np.concatenate(seen))
    assert np.array_equal(arrays["buffer_delta_slots"], want)
    assert m["n_dirty"] == want.size < m["dims"]["current_size"] == 12
    full = fingerprint(agent)
    for k, rows in zip(("obs", "ag", "g", "actions"), ts.DELTA_ROW_ARRAYS):
        assert arrays[rows].tobytes() == np.ascontiguousarray(full[f"buffer_{k}"][want]).tobytes(), k


def test_resume_through_base_and_delta_equals_not_stopping(tmp_path):
    n1, n2, m, kw = 3, 2, 2, dict(cap_eps=7)
    a = build(**kw)
    cycles(a, None, 0, n1 + n2 + m)
    want, want_losses = fingerprint(a), a.last_losses(m * N_BATCHES)
    b = build(**kw)
    cycles(b, None, 0, n1)
    a_path = b.save_training_state(tmp_path / "state.npz", epoch=1, cycle=n1)
    cycles(b, None, n1, n2)
    d_path = b.save_training_state(tmp_path / "state.delta.npz", epoch=1, cycle=n1 + n2, base=a_path)
    del b
    b2 = build(torch_seed=99, rng_seed=4321, **kw)
    before = fingerprint(b2)
    assert before["actor"].tobytes() != want["actor"].tobytes() and before["rng_key"].tobytes() != want["rng_key"].tobytes()
    assert b2.load_training_state(d_path) == b"" and b2.resumed_at == (1, n1 + n2)      # the base: the recorded name, beside it
    cycles(b2, None, n1 + n2, m)
    assert_same(fingerprint(b2), want, "resumed through base + delta")
    assert b2.last_losses(m * N_BATCHES).tobytes() == want_losses.tobytes()
    # another delta against the LOADED state (written out by flatten): lineage and epochs survive the resume
    flat = ts.flatten(a_path, d_path, tmp_path / "flat.npz")
    with pytest.raises(ts.StateError, match="older than the load_training_state|not a state this agent"):
        b2.save_training_state(tmp_path / "no.npz", base=a_path)              # A itself is older than the restore
    d2 = b2.save_training_state(tmp_path / "D2.npz", base=flat)
    f2 = b2.save_training_state(tmp_path / "F2.npz")
    _, m2 = check_delta_file(d2)
    assert_composes_to(flat, d2, f2, "delta against the loaded state")
    lineage = ts.read_manifest(a_path)["lineage"]
    assert m2["lineage"] == m2["base"]["lineage"] == ts.read_manifest(f2)["lineage"] == lineage
    assert 0 < m2["n_dirty"] <= m * EPS_PER_CYCLE


def test_capture_semantics(tmp_path):
    """A wait=False delta does not see later cycles; a second capture of either kind while one is pending raises; a delta capture
    dropped unfetched does not corrupt the next delta against the same base (stamps are absolute)."""
    x, y = build(cap_eps=12), build(cap_eps=12)
    for ag in (x, y):
        cycles(ag, None, 0, 7)
    ax, ay = x.save_training_state(tmp_path / "Ax.npz"), y.save_training_state(tmp_path / "Ay.npz")
    for ag in (x, y):
        cycles(ag, None, 7, 2)
    sync_path = x.save_training_state(tmp_path / "sync.npz", base=ax)
    h = y.save_training_state(tmp_path / "async.npz", wait=False, base=ay)
    assert not os.path.exists(tmp_path / "async.npz")
    for kw in (dict(), dict(base=ay)):
        with pytest.raises(_lib.HpError, match="has not been fetched yet"):
            y.save_training_state(tmp_path / "second.npz", **kw)
    assert not os.path.exists(tmp_path / "second.npz")
    cycles(y, None, 9, 2)                                       # training goes on; the snapshot must not move
    y.ctx.synchronize()
    assert h.result() == str(tmp_path / "async.npz") and h.done()
    (wa, wm), (ga, gm) = ts.read_state(sync_path), ts.read_state(tmp_path / "async.npz")
    assert_same(ga, wa, "async vs sync delta")
    assert gm["n_dirty"] == wm["n_dirty"] and gm["dims"] == wm["dims"] and gm["arrays"] == wm["arrays"]
    # dropped captures, a delta and a full one, at the C level: nobody fetches them, their files are never written
    cycles(x, None, 9, 2)
    ticket, nbytes = C.c_uint64(), C.c_size_t()
    since = ts.known_base(x, ax)[1]
    _lib.check(x.lib.hp_state_capture_delta(*x._handles(), since, 12, C.byref(ticket), C.byref(nbytes)))
    _lib.check(x.lib.hp_state_fetch(x.h, ticket.value, 1, None, 0, None, None))
    cycles(x, None, 11, 1)
    _lib.check(x.lib.hp_state_capture(*x._handles(), C.byref(ticket), C.byref(nbytes)))
    _lib.check(x.lib.hp_state_fetch(x.h, ticket.value, 1, None, 0, None, None))
    cycles(x, None, 12, 1)
    d = x.save_training_state(tmp_path / "D.npz", base=ax)
    f = x.save_training_state(tmp_path / "F.npz")
    check_delta_file(d)
    assert_composes_to(ax, d, f, "after dropped captures")
    # ... and y, which ran the same cycles without them, holds the same buffer
    cycles(y, None, 11, 2)
    assert_same(fingerprint(y), fingerprint(x), "x vs y")


def test_refusals_leave_the_receiver_untouched(tmp_path):
    src, recv = build(cap_eps=12), build(cap_eps=12, torch_seed=5, rng_seed=11)
    cycles(src, None, 0, 3)
    cycles(recv, None, 10, 3)
    foreign = src.save_training_state(tmp_path / "foreign.npz")
    mine = recv.save_training_state(tmp_path / "mine.npz")
    cycles(recv, None, 13, 1)
    before = fingerprint(recv)
    epochs = ts._epochs(recv)

    def refused(exc, match, **kw):
        with pytest.raises(exc, match=match):
            recv.save_training_state(tmp_path / "refused.npz", **kw)
        assert not os.path.exists(tmp_path / "refused.npz")
        assert_same(fingerprint(recv), before, match)

    refused(ts.StateError, "not a state this agent saved or loaded", base=foreign)            # a base from another agent
    assert ts._epochs(recv) == epochs                                                          # nothing was captured
    old = dict(ts.read_manifest(mine))
    arrays, _ = ts.read_state(mine)
    del old["lineage"], old["capture_epoch"]
    refused(ts.StateError, "written before delta states", base=ts.write_state(tmp_path / "old.npz", arrays, old))
    refused(ts.StateError, "'kind' is 'delta'", base=recv.save_training_state(tmp_path / "d.npz", base=mine))
    # a base older than a load_training_state done since
    later = recv.save_training_state(tmp_path / "later.npz")
    recv.load_training_state(mine)
    cycles(recv, None, 13, 1)
    assert_same(fingerprint(recv), before, "rolled back and replayed")
    known = dict(ts._known(recv))
    refused(ts.StateError, "older than the load_training_state done since", base=later)
    refused(ts.StateError, "not a state this agent saved or loaded", base=foreign)
    # ... and at the C level: a since below min_since is HP_ERR_STATE, nothing enqueued, no ticket pending
    _, epoch, min_since = ts._epochs(recv)
    assert min_since > epochs[1] and epoch == min_since + 1
    ticket, nbytes = C.c_uint64(), C.c_size_t()
    for since, match in ((min_since - 1, "older than the last restore"), (epoch, "not a capture of this buffer")):
        with pytest.raises(_lib.HpError, match=match):
            _lib.check(recv.lib.hp_state_capture_delta(*recv._handles(), since, 1, C.byref(ticket), C.byref(nbytes)))
    with pytest.raises(ValueError, match="max_dirty"):
        _lib.check(recv.lib.hp_state_capture_delta(*recv._handles(), min_since, 13, C.byref(ticket), C.byref(nbytes)))
    assert ts._epochs(recv)[1] == epoch and ts._known(recv) == known
    assert_same(fingerprint(recv), before, "after the library's refusals")
    # the loaded state itself is a base: the receiver still works
    d = recv.save_training_state(tmp_path / "ok.npz", base=mine)
    f = recv.save_training_state(tmp_path / "okF.npz")
    assert_composes_to(mine, d, f, "delta against the loaded base")


CHUNK = _lib.STATE_DIRTY_CHUNK


@pytest.mark.parametrize("cap", [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7])
def test_dirty_scan_alone(cap):
    c = ctx()
    h = C.c_void_p()
    _lib.check(c.lib.hp_buffer_create(c.h, cap, 1, 1, 1, 1, C.byref(h)))
    since = 5
    try:
        def scan(stamps, cs, max_dirty):
            stamps = np.ascontiguousarray(stamps, np.uint32)
            out, n, over = np.full(max(max_dirty, 1), -1, np.int64), C.c_int64(), C.c_int32()
            _lib.check(c.lib.hp_state_debug_dirty_scan(h, _lib.ptr(stamps, C.c_uint32), cs, since, max_dirty,
                                                       _lib.ptr(out, C.c_int64), C.byref(n), C.byref(over)))
            return out, n.value, over.value

        clean = np.array([0, 3, 5, 5], np.uint32)[np.arange(cap) % 4]            # never written, older, exactly `since`
        patterns = {"none": clean.copy(), "all": np.full(cap, 6, np.uint32)}
        for name, idx in (("slot0", [0]), ("last", [cap - 1]), ("every_other", np.arange(0, cap, 2))):
            patterns[name] = clean.copy()
            patterns[name][idx] = np.uint32(2 ** 32 - 1) if name == "last" else 9
        for name, stamps in patterns.items():
            want = np.flatnonzero(stamps > since)
            got, n, over = scan(stamps, cap, cap)
            assert n == want.size and not over and np.array_equal(got[:n], want), (cap, name)
            assert np.all(got[n:] == -1), (cap, name)
        # current_size < capacity with dirty stamps beyond it: ignored
        for cs in sorted({0, cap // 2, cap - 1}):
            stamps = patterns["every_other"].copy()
            stamps[cs:] = 9
            want = np.flatnonzero(stamps[:cs] > since)
            got, n, over = scan(stamps, cs, cap)
            assert n == want.size and not over and np.array_equal(got[:n], want), (cap, "beyond", cs)
        # a bound that is too small: the count is the true one, the flag is up, nothing is written past the room
        want = np.flatnonzero(patterns["all"] > since)
        if cap > 1:
            got, n, over = scan(patterns["all"], cap, cap // 2)
            assert n == cap and over == 1 and np.array_equal(got, want[:cap // 2]), cap
    finally:
        c.lib.hp_buffer_destroy(h)
