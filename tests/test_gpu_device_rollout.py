"""Rollouts collected on the device (csrc/rollout.hip, csrc/mt19937_wave.h, device_env.py): policy on device rows, numpy's legacy
normal / uniform / binomial draws on the device stream, teacher-forced exploration against `_select_actions`, the closed loop
against the host lockstep path, and store / train cycle out of the device block."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import bits
from gpu_common import ctx, fresh_rng, host_select_actions, ulp_distance
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_CRITIC, ddpg_agent
from rl_arm_under_sparse_reward_amd.device_env import DeviceEpisodes, PointMassVecEnv, binomial1_qn
from rl_arm_under_sparse_reward_amd.replay_buffer import DeviceEpisodeBuffer
from rl_arm_under_sparse_reward_amd.synthetic import PointMassGoalEnv
from rollout_common import DEV, dev_ptr as p, make, primed

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rows", [1, 2, 5, 64, 1000])
def test_act_device_equals_act(rows):
    torch.manual_seed(0)
    agent = make(None)
    rs = primed(agent)
    obs = rs.normal(0.2, 0.6, size=(rows, 27)); obs[0, :3] = [40.0, -40.0, 0.2]
    g = rs.normal(0.25, 0.2, size=(rows, 3))
    ot, gt = torch.from_numpy(obs).to(DEV), torch.from_numpy(g).to(DEV)
    for target in (False, True):
        for clip_obs in (0.0, 0.5):
            want = agent.act(obs, g, target=target, clip_obs=clip_obs)
            got = agent.act_device(ot, gt, target=target, clip_obs=clip_obs)
            assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (rows, 4)
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (rows, target, clip_obs)


@pytest.mark.parametrize("rows", [1, 5, 33])                     # 33: past the 32-row padding of the GEMMs' Mp
def test_act_device_equals_act_on_the_layer_engine(rows, monkeypatch):
    """The same on the layer-per-launch engine, whose device-to-device tail (mlp_rows, agent_forward.hip) the default engine never
    takes: act_device leaves in device memory the bits act downloads."""
    monkeypatch.setenv("RLARM_ENGINE", "layers")
    probe = make(None)                                           # the switch took: no fused policy kernel to snapshot (HP_ERR_STATE)
    assert probe.lib.hp_agent_policy_snapshot(probe.h, probe.o_norm.h, probe.g_norm.h) == -5
    test_act_device_equals_act(rows)


def test_draw_hooks_follow_numpy():
    """standard_normal / binomial1 consume numpy's words (state, cached normal included); binomials equal, normals within 4 ulp
    (device log: 1 ulp; sqrt, divide, multiply exactly rounded)."""
    dev, rs = fresh_rng(77), np.random.RandomState(77)
    worst = 0
    for size in (1, 3, 4, 1, 1000, 7, 129):
        got, want = dev.standard_normal(size), rs.randn(size)
        d = int(ulp_distance(got, want).max())
        worst = max(worst, d)
        assert d <= 4, (size, d)
        sd, sn = dev.get_state(), rs.get_state()
        assert np.array_equal(sd[1], sn[1]) and sd[2] == sn[2] and sd[3] == sn[3], size
        assert abs(sd[4] - sn[4]) <= 4 * np.spacing(abs(sn[4])), size
        # re-align the cached value so later draws start from identical states
        dev.set_state(sn)
    print("standard_normal: worst distance to numpy", worst, "ulp")
    for p in (0.3, 0.7, 0.0, 1.0, 0.5):
        got, want = dev.binomial1(p, 500), rs.binomial(1, p, 500)
        assert np.array_equal(got, want), p
        sd, sn = dev.get_state(), rs.get_state()
        assert np.array_equal(sd[1], sn[1]) and sd[2:] == sn[2:], p
    # mixed with the older hooks on the same stream
    assert np.array_equal(dev.randint(0, 1000, 50), rs.randint(0, 1000, 50))
    assert np.array_equal(dev.uniform(10), rs.random_sample(10))


def test_set_state_with_a_pending_cached_gaussian_returns_it_first():
    rs = np.random.RandomState(5)
    rs.randn(3)
    st = rs.get_state()
    assert st[3] == 1
    dev = fresh_rng(0)
    dev.set_state(st)
    assert dev.get_state()[3:] == st[3:]
    got, want = dev.standard_normal(2), rs.randn(2)
    assert got[0] == st[4] == want[0]
    assert ulp_distance(got[1:], want[1:]).max() <= 4
    assert dev.get_state()[3] == rs.get_state()[3] == 1
    dev.seed(5)
    assert dev.get_state()[3:] == (0, 0.0)


@pytest.mark.parametrize("epoch", [0, 100])
@pytest.mark.parametrize("n_envs,dims", [(1, (27, 3, 4)), (3, (27, 3, 4)), (64, (27, 3, 4)), (3, (10, 2, 3))])
def test_teacher_forced_exploration_follows_select_actions(n_envs, dims, epoch):
    """Every step is handed the same policy outputs as a host RandomState driven through `_select_actions` in env order: after
    every step key, position and has_gauss are numpy's; every action within one float32 spacing (the device log may differ from
    glibc's in the last place of a float64).  Elements not bit-equal are counted and printed."""
    od, gd, ad = dims
    T, noise_eps, random_eps, amax = 100, 0.2, 0.3, 0.5
    c = ctx()
    buf = DeviceEpisodeBuffer(8, T, od, gd, ad, ctx=c)
    eps = DeviceEpisodes(c, buf, n_envs)
    _lib.check(c.lib.hp_rollout_set_action_max(eps.h, amax))
    dev, rs = fresh_rng(21 + n_envs), np.random.RandomState(21 + n_envs)
    prs = np.random.RandomState(1)
    qn = binomial1_qn(random_eps)[0]
    unequal = total = 0
    want_act = np.empty((n_envs, T, ad))
    rows = [prs.uniform(-1, 1, (T + 1, n_envs, d)) for d in (od, gd, gd)]
    for t in range(T):
        pi = prs.uniform(-0.6, 0.6, (n_envs, ad)).astype(np.float32)
        o, a, g = (torch.from_numpy(r[t]).to(DEV) for r in rows)
        act = torch.from_numpy(pi).to(DEV)
        with c.torch_bridge():
            _lib.check(c.lib.hp_rollout_step(eps.h, None, None, None, dev.h, t, p(o), p(a), p(g), 1, noise_eps, random_eps, qn,
                                             0.15 if epoch >= 100 else 0.0, p(act)))
        dev.mark_normals_drawn()
        want = np.stack([host_select_actions(rs, pi[i], noise_eps, random_eps, amax, epoch >= 100) for i in range(n_envs)])
        got = act.cpu().numpy()
        sd, sn = dev.get_state(), rs.get_state()
        assert np.array_equal(sd[1], sn[1]) and sd[2] == sn[2] and sd[3] == sn[3], t
        assert want.dtype == np.float32 and np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))), t
        unequal += int((bits(got).reshape(-1, 4) != bits(want).reshape(-1, 4)).any(axis=1).sum())
        total += got.size
        want_act[:, t] = got
        dev.set_state(sn)      # carry numpy's cached normal (it may differ in the last place) so states stay comparable
    o, a = torch.from_numpy(rows[0][T]).to(DEV), torch.from_numpy(rows[1][T]).to(DEV)
    with c.torch_bridge():
        _lib.check(c.lib.hp_rollout_finish(eps.h, p(o), p(a)))
    print(f"teacher-forced n_envs={n_envs} dims={dims} epoch={epoch}: {unequal} of {total} float32 actions not bit-equal")
    obs, ag, g, actions = eps.numpy()
    assert np.array_equal(obs, rows[0].transpose(1, 0, 2)) and np.array_equal(ag, rows[1].transpose(1, 0, 2))
    assert np.array_equal(g, rows[2][:T].transpose(1, 0, 2)) and np.array_equal(bits(actions), bits(want_act))


@pytest.mark.parametrize("n_envs,n_rollouts", [(4, 4), (2, 5)])
def test_closed_loop_without_noise_equals_the_host_lockstep_path(n_envs, n_rollouts):
    torch.manual_seed(0)
    host = make([PointMassGoalEnv(seed=10 + i, max_timesteps=50) for i in range(n_envs)])
    primed(host)
    want = host.collect_episodes(n_rollouts, explore=False)
    torch.manual_seed(0)
    agent = make(PointMassVecEnv(n_envs, seed=10, device=DEV, max_timesteps=50))
    primed(agent)
    handle = agent.collect_episodes_device(n_rollouts=n_rollouts, explore=False)
    got = handle.numpy()
    for name, a, b in zip(("obs", "ag", "g", "actions"), got, want):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), name


@pytest.mark.parametrize("f32_rows", [False, True])
def test_store_and_cycle_from_the_device_block_equal_the_host_cycle(f32_rows):
    """train_cycle(handle) against a second agent given handle.numpy() through the existing train_cycle: slots, buffer contents,
    normalizer statistics, parameters and random stream, over three cycles (the cached graph is replayed)."""
    T, n = 50, 4
    agents = []
    for _ in range(2):
        torch.manual_seed(0)
        a = make(PointMassVecEnv(n, seed=10, device=DEV, max_timesteps=T), T=T, seed=8, n_batches=5, buffer_episodes=10)
        if f32_rows:
            a.buffer.enable_f32_rows()
        agents.append(a)
    dev_agent, host_agent = agents
    for cycle in range(3):       # the third cycle overflows the 10-episode buffer: the slot draw consumes the stream
        handle = dev_agent.collect_episodes_device(explore=True)
        episodes = handle.numpy()
        host_agent.rng.set_state(dev_agent.rng.get_state())
        dev_agent.train_cycle(handle)
        host_agent.train_cycle(episodes)
        sa, sb = np.empty(n, np.int64), np.empty(n, np.int64)
        for ag_, out in ((dev_agent, sa), (host_agent, sb)):
            _lib.check(ag_.lib.hp_buffer_last_slots(ag_.buffer._dev.h, _lib.ptr(out, C.c_int64), n))
        assert np.array_equal(sa, sb), cycle
        for which in range(4):
            size = dev_agent.buffer.size
            shape = [(T + 1) * 27, (T + 1) * 3, T * 3, T * 4][which]
            ba, bb = np.empty((size, shape)), np.empty((size, shape))
            for ag_, out in ((dev_agent, ba), (host_agent, bb)):
                _lib.check(ag_.lib.hp_buffer_read(ag_.buffer._dev.h, which, 0, size, _lib.ptr(out, C.c_double)))
            stored = dev_agent.buffer.current_size      # the slots behind it were never written: the allocation is not cleared
            assert stored == host_agent.buffer.current_size == min(size, n * (cycle + 1))
            assert np.array_equal(bits(ba[:stored]), bits(bb[:stored])), (cycle, which)
        for slot in (NET_ACTOR, NET_CRITIC, 2, 3):
            assert np.array_equal(bits(dev_agent._get_flat(slot)), bits(host_agent._get_flat(slot))), (cycle, slot)
        assert np.array_equal(bits(dev_agent.o_norm.mean), bits(host_agent.o_norm.mean))
        assert np.array_equal(bits(dev_agent.g_norm.std), bits(host_agent.g_norm.std))
        sd, sh = dev_agent.rng.get_state(), host_agent.rng.get_state()
        assert np.array_equal(sd[1], sh[1]) and sd[2:] == sh[2:], cycle
    assert dev_agent.buffer.current_size == host_agent.buffer.current_size == 10
    # store_episode(handle) alone: same slots and contents as the host store
    handle = dev_agent.collect_episodes_device(explore=False)
    host_agent.rng.set_state(dev_agent.rng.get_state())
    dev_agent.buffer.store_episode(handle)
    host_agent.buffer.store_episode(handle.numpy())
    sa, sb = np.empty(n, np.int64), np.empty(n, np.int64)
    for ag_, out in ((dev_agent, sa), (host_agent, sb)):
        _lib.check(ag_.lib.hp_buffer_last_slots(ag_.buffer._dev.h, _lib.ptr(out, C.c_int64), n))
    assert np.array_equal(sa, sb)
    assert dev_agent.rng.get_state()[2] == host_agent.rng.get_state()[2]


def test_learn_on_the_device_path_follows_the_reference_run(tmp_path, monkeypatch):
    """learn() with a one-environment PointMassVecEnv against tests/golden/rollout.npz (the reference's own learn() on the stand-in
    environment), tolerances of the host-path test; no numpy state hand-off between cycles."""
    from conftest import load_golden
    from gpu_common import state_equal
    g = load_golden("rollout.npz")
    c = {k: (float(v) if "." in v else int(v)) for k, v in g["cfg"]}
    env = PointMassVecEnv(1, seed=c["env_seed"], device=DEV, max_timesteps=100, distance_threshold=c["distance_threshold"])
    args = Args(n_epochs=c["n_epochs"], n_cycles=c["n_cycles"], n_batches=c["n_batches"], n_test_rollouts=c["n_test_rollouts"],
                noise_eps=c["noise_eps"], random_eps=c["random_eps"], buffer_size=c["buffer_episodes"] * 100,
                save_dir=str(tmp_path), env_name="stand_in")
    agent = ddpg_agent(args, env, env.env_params, rng=fresh_rng(0))
    agent._set_flat(NET_ACTOR, g["init_actor"]); agent._set_flat(NET_CRITIC, g["init_critic"])
    agent.lib.hp_agent_sync_targets(agent.h)
    stored, calls = [], {"get": 0, "set": 0}
    orig = agent.train_cycle
    agent.train_cycle = lambda eps, n_batches=None: (stored.append(eps.numpy()), calls.update(cycle_get=calls["get"], cycle_set=calls["set"]), orig(eps, n_batches))[2]
    np.random.seed(c["np_seed"])
    get0, set0 = np.random.get_state, np.random.set_state
    monkeypatch.setattr(np.random, "get_state", lambda *a, **k: (calls.__setitem__("get", calls["get"] + 1), get0(*a, **k))[1])
    monkeypatch.setattr(np.random, "set_state", lambda *a, **k: (calls.__setitem__("set", calls["set"] + 1), set0(*a, **k))[1])
    agent.learn()
    monkeypatch.undo()
    assert len(stored) == c["n_epochs"] * c["n_cycles"]
    assert calls["cycle_get"] == 1 and calls["cycle_set"] == 0                  # handed over once, before the first cycle ...
    assert calls["get"] == 1 and calls["set"] == 1                              # ... and back once, at the end
    for i, batch in enumerate(stored):
        tol = 2e-6 if i == 0 else 2e-4
        for nm, a in zip(("obs", "ag", "g", "actions"), batch):
            want = g[f"cycle{i}_{nm}"].astype(np.float64)
            assert a.shape == want.shape and float(np.abs(a - want).max()) <= tol, (i, nm, float(np.abs(a - want).max()))
    key, pos = np.random.get_state()[1:3]
    assert np.array_equal(key, g["key"]) and pos == int(g["pos"])
    assert state_equal(agent.rng, g["key"], g["pos"])
    assert np.allclose(agent.success_rates, g["success_rates"], atol=1.0 / c["n_test_rollouts"] + 1e-9)


def test_train_state_carries_the_pending_cached_gaussian(tmp_path):
    """Save in the middle of a device-path run with a cached normal pending (3 action draws per step would leave one; here the
    4-component actions leave none, so one extra normal is drawn first): the resumed run reproduces the next cycle bit for bit."""
    from rl_arm_under_sparse_reward_amd.train_state import read_state
    T, n = 50, 2

    def build():
        torch.manual_seed(0)
        return make(PointMassVecEnv(n, seed=4, device=DEV, max_timesteps=T), T=T, seed=12, n_batches=3, buffer_episodes=20)

    a = build()
    a.train_cycle(a.collect_episodes_device())
    a.rng.standard_normal(1)                                  # leaves the second normal of the pair cached
    assert a.rng.get_state()[3] == 1
    path = a.save_training_state(tmp_path / "mid.npz")
    manifest = read_state(path)[1]
    assert manifest["rng_gauss"][0] == 1 and manifest["rng_gauss"][1] == a.rng.get_state()[4]
    env_rs = [r.get_state() for r in a.vec_env.rs]
    want = a.collect_episodes_device().numpy()
    a.train_cycle(a._rollouts[n])
    want_params = a._get_flat(NET_ACTOR)
    want_state = a.rng.get_state()
    b = build()
    b.load_training_state(path)
    assert b.rng.get_state()[3] == 1
    for r, st in zip(b.vec_env.rs, env_rs):
        r.set_state(st)
    got = b.collect_episodes_device()
    for x, y in zip(got.numpy(), want):
        assert np.array_equal(bits(x), bits(y))
    b.train_cycle(got)
    assert np.array_equal(bits(b._get_flat(NET_ACTOR)), bits(want_params))
    sb = b.rng.get_state()
    assert np.array_equal(sb[1], want_state[1]) and sb[2:] == want_state[2:]
