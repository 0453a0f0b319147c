"""The critic audit on the device (csrc/episode_q.hip: hp_episode_q, hp_episode_q_block; csrc/episode_returns.hip:
hp_episode_returns, hp_episode_returns_block, hp_episode_critic_summary; DeviceEpisodes.returns, ddpg_agent.episode_q,
episode_critic_stats, episode_critic_stats_host, args.eval_critic).

Q is compared with the oracle's critic (oracle.ddpg_update.critic_forward) on inputs prepared in numpy -- float64 clip, subtract,
divide, clip, cast; the action cast to float32 and then divided -- at the project's own bar for the critic forward, rtol 1e-5 /
atol 1e-6 (tests/test_gpu_update.py), no row excluded.  Returns, critic columns and summary are compared bit for bit with the host
twins (synthetic.episode_returns / episode_critic_stats / episode_critic_summary): their orders are fixed."""
import ctypes as C
import shutil

import numpy as np
import pytest
import torch

from conftest import bits
from gpu_common import ctx, fresh_rng, make_shape_episodes
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd import train_state as ts
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_CRITIC, NET_CRITIC_TARGET, ddpg_agent
from rl_arm_under_sparse_reward_amd.device_env import (NativePickPlaceVecEnv, NativePointMassVecEnv, NativePushBlockVecEnv, PushBlockVecEnv,
                                                       generate_demos)
from rl_arm_under_sparse_reward_amd.synthetic import (CRITIC_STATS, EPISODE_SUMMARY, episode_critic_stats, episode_critic_summary,
                                                      episode_returns)
from episode_common import learner, oracle_q, raw_q, refused, shaped_agent
from rollout_common import CONTACT, DEV, agent_on, dev_ptr as p, make, primed

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6


# ------------------------------------------------------------------------------------------ helpers
def assert_q(got, want, what):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{what}: max |Q - oracle| {err.max():.3e} on |Q| up to {np.abs(want).max():.3e}")
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all(), what
    assert np.allclose(got, want, rtol=RTOL, atol=ATOL), (what, float(err.max()))


def assert_audit(agent, batch, stats, q, returns, thr, target=False, tail="persist"):
    """(stats, q, returns) of an audit of the host arrays `batch`: q against the oracle, the rest bit for bit against the twins"""
    stats, q, returns = (v.cpu().numpy() if isinstance(v, torch.Tensor) else v for v in (stats, q, returns))
    assert_q(q, oracle_q(agent, batch[0], batch[2], batch[3], target)[0], "audit")
    gamma, kind = float(agent.args.gamma), agent.args.reward_type
    want_returns = episode_returns(batch[1], batch[2], thr, gamma, kind, tail)
    assert returns.dtype == np.float64 and np.array_equal(bits(returns), bits(want_returns))
    want = episode_critic_stats(q, want_returns, gamma)
    assert stats.dtype == np.float64 and stats.shape == (q.shape[0], 6) and np.array_equal(bits(stats), bits(want)), (stats, want)
    return want


SHAPES = [(1, 1), (5, 3), (3, 63), (2, 64), (3, 65), (7, 100)]     # rows no multiple of 4, slabs that straddle episodes, T / T + 1 strides


# ------------------------------------------------------------------------------------------ 1. Q against the oracle
@pytest.mark.parametrize("obs_dim,goal_dim,act_dim,amax,clips", [(27, 3, 4, 0.5, None), (20, 1, 3, 0.7, None), (29, 3, 1, 2.0, None),
                                                                  (27, 3, 4, 0.5, (0.8, 1.5))])
def test_q_of_random_blocks_equals_the_oracle(obs_dim, goal_dim, act_dim, amax, clips):
    kw = dict(clip_obs=clips[0], clip_range=clips[1]) if clips else {}
    agent = shaped_agent(obs_dim, goal_dim, act_dim, amax, **kw)
    rs = np.random.RandomState(17)
    far = 0.0
    for n, T in SHAPES:
        obs = rs.normal(0.1, 0.6, (n, T + 1, obs_dim))
        obs[:, T] = 1e30                                   # the closing observation of every episode: no step reads it
        g = rs.normal(0.2, 0.5, (n, T, goal_dim))
        actions = rs.uniform(-amax, amax, (n, T, act_dim))
        for target in (False, True):
            want, x, a = oracle_q(agent, obs, g, actions, target)
            got = raw_q(agent, obs, g, actions, target)
            assert_q(got, want, f"{(obs_dim, goal_dim, act_dim, amax)} n {n} T {T} target {target}")
            net = agent.critic_target_network if target else agent.critic_network
            far = max(far, float(np.abs(net(x, a).reshape(n, T) - got).max()))
            if clips:
                assert np.mean(np.abs(obs[:, :T]) > clips[0]) > 0.1 and np.mean(np.abs(x) == clips[1]) > 0.05      # both clips bite
    assert not np.array_equal(raw_q(agent, obs, g, actions, False), raw_q(agent, obs, g, actions, True))
    print(f"largest difference to hp_agent_critic_forward on the same rows: {far:.3e}")


# ------------------------------------------------------------------------------------------ 2. after training
@pytest.mark.parametrize("batch", [64, 256])
def test_q_after_training_cycles_reads_the_stepped_weights(batch):
    """Two train_cycles on a small buffer, one in each launch form of an update sequence, then both nets against the oracle on the
    parameters hp_agent_get_params returns and the statistics of hp_norm_get: a fragment copy that a launch form did not step
    would fail here."""
    T, n_eps = 20, 8
    torch.manual_seed(0)
    env = {"obs": 27, "goal": 3, "action": 4, "action_max": 0.5, "max_timesteps": T}
    agent = ddpg_agent(Args(batch_size=batch, buffer_size=4 * n_eps * T, lr_critic=0.01, lr_actor=0.01), None, env, rng=fresh_rng(3))
    before = agent._get_flat(NET_CRITIC)
    form, forms = C.c_int32(), []
    for cycle, n_batches in enumerate((3, 13)):       # a short sequence: chain launch + tile launch per update; a long one: split launch
        agent.train_cycle(make_shape_episodes(n_eps, 27, 3, 4, T, seed=20 + cycle), n_batches=n_batches)
        _lib.check(agent.lib.hp_agent_update_form(agent.h, n_batches, C.byref(form)))
        forms.append(form.value)
    print(f"batch {batch}: update forms of the two sequences {forms}; engine {agent.engine()['engine']}")
    assert forms == [0, 1], forms
    after, after_t = agent._get_flat(NET_CRITIC), agent._get_flat(NET_CRITIC_TARGET)
    assert np.abs(after - before).max() > 1e-3 and not np.array_equal(after, after_t) and not np.array_equal(after_t, before)
    obs, _, g, actions = make_shape_episodes(5, 27, 3, 4, 33, seed=31)
    for target in (True, False):
        want = oracle_q(agent, obs, g, actions, target)[0]
        assert_q(raw_q(agent, obs, g, actions, target), want, f"batch {batch} target {target}")
    agent._set_flat(NET_CRITIC, before)
    moved = np.abs(raw_q(agent, obs, g, actions) - want).max()          # the bar does tell the weights before from those after
    assert moved > 100 * ATOL, moved


# ------------------------------------------------------------------------------------------ 3. sub-ranges of a block
def test_sub_ranges_of_a_push_block_collection():
    """Nine episodes of T = 20 on eight environments.  first * T is a multiple of 4 for every `first`, so every sub-range starts
    on a slab boundary of the whole-block call; a block of T = 5 has sub-ranges that do not."""
    a = agent_on(NativePushBlockVecEnv, 8, 20, env_seed=21, env_kw=CONTACT, random_eps=0.3)
    eps = a.collect_episodes_device(n_rollouts=9)
    batch = eps.numpy()
    whole = a.episode_q(eps).cpu().numpy()
    assert_q(whole, oracle_q(a, batch[0], batch[2], batch[3])[0], "whole block")
    for first, n in ((3, 4), (0, 1), (8, 1), (1, 8)):
        out = torch.full((9, eps.T), float("nan"), dtype=torch.float32, device=DEV)
        with a.ctx.torch_bridge():
            _lib.check(a.lib.hp_episode_q_block(eps.h, a.h, a.o_norm.h, a.g_norm.h, NET_CRITIC, first, n, float(a.args.clip_obs), p(out[first:])))
        got = out.cpu().numpy()
        assert (first * eps.T) % 4 == 0 and np.array_equal(bits(got[first:first + n]), bits(whole[first:first + n])), (first, n)
        assert np.isnan(got[:first]).all() and np.isnan(got[first + n:]).all()           # nothing outside [first, first + n)
        assert np.array_equal(bits(a.episode_q(eps, first=first, n=n).cpu().numpy()), bits(whole[first:first + n]))
    assert np.array_equal(bits(a.episode_q(eps, first=7).cpu().numpy()), bits(whole[7:]))
    # T = 5: episodes 1, 2, 3 start in the middle of a slab of the whole-block call
    torch.manual_seed(0)
    b = make(NativePointMassVecEnv(3, seed=4, device=DEV, max_timesteps=5), T=5)
    primed(b)
    eps = b.collect_episodes_device(n_rollouts=6, explore=False)
    batch = eps.numpy()
    whole, want = b.episode_q(eps).cpu().numpy(), oracle_q(b, batch[0], batch[2], batch[3])[0]
    assert_q(whole, want, "T = 5, whole block")
    for first, n in ((1, 2), (2, 3), (3, 3), (4, 1), (5, 1)):
        out = torch.full((6, 5), float("nan"), dtype=torch.float32, device=DEV)
        with b.ctx.torch_bridge():
            _lib.check(b.lib.hp_episode_q_block(eps.h, b.h, b.o_norm.h, b.g_norm.h, NET_CRITIC, first, n, float(b.args.clip_obs), p(out[first:])))
        got = out.cpu().numpy()
        assert_q(got[first:first + n], want[first:first + n], f"T = 5, episodes [{first}, {first + n})")
        assert np.isnan(got[:first]).all() and np.isnan(got[first + n:]).all()
        same = np.array_equal(bits(got[first:first + n]), bits(whole[first:first + n]))
        print(f"first {first} (row {first * 5}, {'on' if first * 5 % 4 == 0 else 'off'} a slab boundary): bit-equal to the whole-block call: {same}")
        if first * 5 % 4 == 0:
            assert same


# ------------------------------------------------------------------------------------------ 4. returns and critic columns
def device_returns(ag, g, thr, kind, gamma, tail, q=None):
    c = ctx()
    a, b = torch.from_numpy(np.ascontiguousarray(ag)).to(DEV), torch.from_numpy(np.ascontiguousarray(g)).to(DEV)
    n, T, gd = g.shape
    out = torch.full((n, T), float("nan"), dtype=torch.float64, device=DEV)
    qd = torch.from_numpy(q).to(DEV) if q is not None else None
    stats = torch.full((n, 6), float("nan"), dtype=torch.float64, device=DEV) if q is not None else None
    summary = torch.full((6,), float("nan"), dtype=torch.float64, device=DEV)
    with c.torch_bridge():
        _lib.check(c.lib.hp_episode_returns(c.h, p(a), p(b), n, T, gd, float(thr), kind, float(gamma), tail, p(out),
                                            p(qd) if q is not None else None, p(stats) if q is not None else None))
        if q is not None:
            _lib.check(c.lib.hp_episode_critic_summary(c.h, p(stats), n, p(summary)))
    return out.cpu().numpy(), (stats.cpu().numpy() if q is not None else None), summary.cpu().numpy()


@pytest.mark.parametrize("T", [1, 63, 64, 65, 100, 130])
def test_returns_and_critic_columns_equal_the_twins(T):
    """Less than a chunk of steps, exactly one, one more, and a third chunk; one, two and three goal components; one episode, a
    few, and more workgroups than a wave has lanes; every gamma with both tails (gamma = 1: the zero tail only), sparse and dense;
    a threshold at which about half of the steps succeed, and for one shape none and all of them.  Q is random float32 with a share
    of values exactly at float32(-1 / (1 - gamma))."""
    rs = np.random.RandomState(300 + T)
    cases = 0
    for gd in (1, 2, 3):
        for n in (1, 5, 70):
            ag, g = rs.uniform(0, 0.5, (n, T + 1, gd)), rs.uniform(0, 0.5, (n, T, gd))
            half = float(np.median(np.linalg.norm(ag[:, 1:] - g, axis=-1))) * (1 + 1e-9)
            for thr in ((half, 0.0, 10.0) if (gd, n) == (3, 5) else (half,)):
                for gamma in (0.98, 0.5, 0.0, 1.0):
                    q = rs.uniform(-60, 5, (n, T)).astype(np.float32)
                    if gamma < 1:
                        q[rs.rand(n, T) < 0.25] = np.float32(-1 / (1 - gamma))
                    for tail in ((0,) if gamma == 1.0 else (0, 1)):
                        for kind in (0, 1):
                            want = episode_returns(ag, g, thr, gamma, kind, tail)
                            with_q = (cases % 3) != 2                        # every third case without the critic columns
                            got, stats, summary = device_returns(ag, g, thr, kind, gamma, tail, q if with_q else None)
                            assert np.array_equal(bits(got), bits(want)), (gd, n, thr, gamma, tail, kind)
                            if with_q:
                                want_stats = episode_critic_stats(q, want, gamma)
                                assert np.array_equal(bits(stats), bits(want_stats)), (gd, n, thr, gamma, tail, kind)
                                assert np.array_equal(bits(summary), bits(episode_critic_summary(want_stats)))
                                if gamma < 1 and n * T >= 60:
                                    assert want_stats[:, 5].sum() >= (q == np.float32(-1 / (1 - gamma))).sum() > 0
                                if gamma == 1.0:
                                    assert not want_stats[:, 5].any()
                            cases += 1
                if thr == half and n * T >= 60:
                    r = episode_returns(ag, g, thr, 0.0, 0, 1)               # the rewards themselves
                    assert 0.4 <= (r == 0).mean() <= 0.6
            if (gd, n) == (3, 5):
                assert (episode_returns(ag, g, 0.0, 0.0, 0, 1) == -1).all() and not episode_returns(ag, g, 10.0, 0.0, 0, 1).any()
    print(f"T {T}: {cases} cases")


# ------------------------------------------------------------------------------------------ 5. the forms of episodes
@pytest.mark.parametrize("form", ["stepped", "fused", "waves"])
def test_every_rollout_form_on_the_push_block_environment(form):
    """Seven evaluation episodes on four environments: stepped on the tensor twin, fused per wave on the native environment, all
    waves in one launch with the reset on the device; the online and the target critic."""
    cls = PushBlockVecEnv if form == "stepped" else NativePushBlockVecEnv
    a = agent_on(cls, 4, 20, env_seed=21, env_kw=CONTACT, reset=(form == "waves"))
    eps = a.collect_episodes_device(n_rollouts=7, explore=False)
    assert a.rollout_form == ("stepped" if form == "stepped" else "fused") and (form != "waves" or a.rollout_launches == 1)
    batch, thr = eps.numpy(), a.vec_env.distance_threshold
    for target, tail in ((False, "persist"), (True, "zero")):
        stats, q, returns = a.episode_critic_stats(eps, target=target, tail=tail)
        assert stats.is_cuda and q.dtype == torch.float32 and tuple(q.shape) == (7, eps.T) and tuple(returns.shape) == (7, eps.T)
        assert_audit(a, batch, stats, q, returns, thr, target, tail)
    sub = a.episode_critic_stats(eps, distance_threshold=0.2, first=2, n=3)
    assert_audit(a, [v[2:5] for v in batch], *sub, 0.2)
    alone = eps.returns(thr, 0.98, "dense", "zero", first=1, n=4)
    assert np.array_equal(bits(alone.cpu().numpy()), bits(episode_returns(batch[1][1:5], batch[2][1:5], thr, 0.98, "dense", "zero")))


def test_what_the_critic_thinks_of_pick_and_place_demonstrations():
    env = NativePickPlaceVecEnv(4, seed=0, device=DEV, max_timesteps=100, step_scale=0.2)
    env.enable_device_reset(ctx())
    demos = generate_demos(env, 4)
    assert demos.kept == 4
    torch.manual_seed(0)
    a = make(env, T=100)
    primed(a)
    stats, q, returns = a.episode_critic_stats(demos.episodes)
    obs, ag, g, actions, info = demos.numpy()
    want = assert_audit(a, [obs, ag, g, actions], stats, q, returns, env.distance_threshold)
    assert info[:, -1].all() and (returns.cpu().numpy()[:, -1] == 0).all() and (want[:, 1] < 0).all()       # they end in success, after misses


def test_host_episodes_through_the_same_kernels():
    torch.manual_seed(0)
    a = make(None)
    primed(a)
    for T, n in ((50, 6), (7, 1)):
        batch = make_shape_episodes(n, 27, 3, 4, T)
        thr = float(np.median(np.linalg.norm(batch[1][:, 1:] - batch[2], axis=-1)))
        for target, tail in ((False, "persist"), (True, "zero")):
            out = a.episode_critic_stats_host(batch, thr, target=target, tail=tail)
            assert all(isinstance(v, np.ndarray) for v in out)
            assert_audit(a, batch, *out, thr, target, tail)
    with pytest.raises(ValueError, match="episode_critic_stats_host: obs"):
        a.episode_critic_stats_host([batch[0], batch[1][:, :-1], batch[2], batch[3]], 0.05)
    with pytest.raises(ValueError, match="dimensions differ from the agent's"):
        a.episode_critic_stats_host([batch[0][:, :, :20], batch[1], batch[2], batch[3]], 0.05)


# ------------------------------------------------------------------------------------------ 6. learn()
def evaluation_audit(a):
    """The calls of _eval_agent_device made by hand: the critic summary the twins give on the evaluation's episodes and the Q this
    agent has of them"""
    rows, remaining = [], int(a.args.n_test_rollouts)
    while remaining > 0:
        k = remaining if a.vec_env.reset_streams is not None else min(a.vec_env.n_envs, remaining)
        eps = a.collect_episodes_device(n_rollouts=k, explore=False)
        q, batch = a.episode_q(eps, n=k).cpu().numpy(), eps.numpy()
        assert_q(q, oracle_q(a, batch[0], batch[2], batch[3])[0], "evaluation")
        G = episode_returns(batch[1], batch[2], a.vec_env.distance_threshold, a.args.gamma, a.args.reward_type, "persist")
        rows.append(episode_critic_stats(q, G, a.args.gamma))
        remaining -= k
    return episode_critic_summary(np.concatenate(rows))


@pytest.mark.parametrize("reset", [False, True], ids=["wave_calls", "one_launch"])
def test_eval_critic_is_the_twins_and_changes_nothing_else(tmp_path, reset, capsys):
    """Two epochs of learn() with the option on and off (eval_metrics on in both): the same rates, metrics, parameters and training
    state to the byte, an empty list with it off; with it on, one dict per evaluation whose values are the twins' on the
    evaluation's episodes -- collected again by a twin agent for epoch 0, and for epoch 1 by an agent restored from the state the
    run saved after epoch 0."""
    on = learner(tmp_path, "on", reset, eval_metrics=True, eval_critic=True, state_path=str(tmp_path / "on.npz"))
    save, host_resets = on._save_epoch_state, {}

    def save_and_keep(path, epoch):          # the state after every epoch, and the simulator's own host generators beside it
        out = save(path, epoch)
        shutil.copy(ts.rank_path(path, 0), tmp_path / f"after{epoch}.npz")
        host_resets[epoch] = [r.get_state() for r in on.vec_env.rs]
        return out

    on._save_epoch_state = save_and_keep
    off = learner(tmp_path, "off", reset, eval_metrics=True, state_path=str(tmp_path / "off.npz"))
    printed, rates = [], []
    for a in (on, off):
        np.random.seed(11)
        a.learn()
        printed.append([line for line in capsys.readouterr().out.splitlines() if "eval success rate" in line])
    assert off.eval_critic == [] and len(on.eval_critic) == 2 and len(on.success_rates) == 2
    assert on.success_rates == off.success_rates and on.eval_metrics == off.eval_metrics and len(on.eval_metrics) == 2
    assert all(tuple(m) == EPISODE_SUMMARY for m in on.eval_metrics)
    assert [line.split("] ", 1)[1] for line in printed[0]] == [line.split("] ", 1)[1] for line in printed[1]] and len(printed[0]) == 2
    for slot in (NET_ACTOR, NET_CRITIC):
        assert np.array_equal(bits(on._get_flat(slot)), bits(off._get_flat(slot))), slot
    sa, sb = ts.read_state(ts.rank_path(str(tmp_path / "on.npz"), 0)), ts.read_state(ts.rank_path(str(tmp_path / "off.npz"), 0))
    assert sorted(sa[0]) == sorted(sb[0])
    for name in sa[0]:
        assert np.array_equal(bits(sa[0][name]), bits(sb[0][name])), name
    # the evaluation episodes again
    twin, restored = learner(tmp_path, "twin", reset), learner(tmp_path, "restored", reset)
    for a in (twin, restored):               # what learn() does before its first epoch
        a.enable_explore_streams()
        if reset:
            a.vec_env.enable_device_reset(a.ctx)
    np.random.seed(11)
    twin.rng.set_state(np.random.get_state())
    restored.load_training_state(str(tmp_path / "after1.npz"))
    assert restored.resumed_at[0] == 1
    for r, state in zip(restored.vec_env.rs, host_resets[1]):
        r.set_state(state)
    for i, a in enumerate((twin, restored)):
        for _ in range(a.args.n_cycles):
            a.train_cycle(a.collect_episodes_device(n_rollouts=a.args.num_rollouts_per_mpi, epoch=i))
        a.ctx.synchronize()
        want = evaluation_audit(a)
        m = on.eval_critic[i]
        assert tuple(m) == CRITIC_STATS
        assert np.array_equal(bits(np.array([m[k] for k in CRITIC_STATS])), bits(want)), (i, m, want)
        assert m["abs_error"] >= abs(m["bias"]) and m["max_abs_error"] >= m["abs_error"] and m["return_mean"] <= 0


def test_eval_critic_on_the_host_path():
    """_eval_agent with host environments goes through episode_critic_stats_host"""
    from rl_arm_under_sparse_reward_amd.synthetic import PointMassGoalEnv
    torch.manual_seed(0)
    envs = [PointMassGoalEnv(seed=30 + i, max_timesteps=10, distance_threshold=0.15) for i in range(2)]
    a = make(envs[0], T=10, n_test_rollouts=3, eval_critic=True)
    a.envs = envs
    primed(a)
    states = [e.rs.get_state() for e in envs]
    rate = a._eval_agent()
    assert len(a.eval_critic) == 1 and a.eval_metrics == [] and tuple(a.eval_critic[0]) == CRITIC_STATS
    for e, s in zip(envs, states):
        e.rs.set_state(s)
    b = make(envs[0], T=10, n_test_rollouts=3)
    b.envs = envs
    for slot in (NET_ACTOR, NET_CRITIC):
        b._set_flat(slot, a._get_flat(slot))
    primed(b)
    assert b._eval_agent() == rate and b.eval_critic == []
    m = a.eval_critic[0]
    assert np.isfinite(list(m.values())).all() and m["max_abs_error"] >= m["abs_error"] >= abs(m["bias"])


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_carry_the_librarys_message(monkeypatch):
    torch.manual_seed(0)
    a = make(NativePointMassVecEnv(2, seed=1, device=DEV, max_timesteps=10), T=10)
    primed(a)
    lib, c = a.lib, a.ctx
    eps = a.collect_episodes_device(n_rollouts=3, explore=False)
    obs, g = torch.zeros((3, 11, 27), dtype=torch.float64, device=DEV), torch.zeros((3, 10, 3), dtype=torch.float64, device=DEV)
    ag = torch.zeros((3, 11, 3), dtype=torch.float64, device=DEV)
    act = torch.zeros((3, 10, 4), dtype=torch.float64, device=DEV)
    q, G = torch.zeros((4, 10), dtype=torch.float32, device=DEV), torch.zeros((4, 10), dtype=torch.float64, device=DEV)
    stats, summary = torch.zeros((4, 6), dtype=torch.float64, device=DEV), torch.zeros(6, dtype=torch.float64, device=DEV)
    h, on, gn = a.h, a.o_norm.h, a.g_norm.h
    # hp_episode_q
    good = [h, on, gn, NET_CRITIC, p(obs), p(g), p(act), 3, 10, 200.0, p(q)]
    for k in (0, 1, 2, 4, 5, 6, 10):
        refused(lib.hp_episode_q(*[None if i == k else v for i, v in enumerate(good)]), "hp_episode_q: null argument")
    for net in (NET_ACTOR, 2, 7):
        refused(lib.hp_episode_q(*[net if i == 3 else v for i, v in enumerate(good)]), "hp_episode_q: net must be a critic")
    refused(lib.hp_episode_q(h, gn, gn, NET_CRITIC, p(obs), p(g), p(act), 3, 10, 200.0, p(q)),
            r"hp_episode_q: normalizer sizes 3\+3 do not match the critic input 30")
    refused(lib.hp_episode_q(*[0 if i == 7 else v for i, v in enumerate(good)]), r"hp_episode_q: n_episodes 0 outside \[1, ")
    refused(lib.hp_episode_q(*[0 if i == 8 else v for i, v in enumerate(good)]), r"hp_episode_q: T 0 outside \[1, ")
    refused(lib.hp_episode_q(*[(1 << 23) if i == 7 else (1 << 20) if i == 8 else v for i, v in enumerate(good)]), "hp_episode_q: .* more than one launch holds")
    other = _lib.Context(0)                                     # a second context on the same device
    from rl_arm_under_sparse_reward_amd.normalizer import normalizer
    foreign = normalizer(27, default_clip_range=5, ctx=other)
    refused(lib.hp_episode_q(*[foreign.h if i == 1 else v for i, v in enumerate(good)]), "hp_episode_q: handles belong to different contexts")
    # hp_episode_q_block
    good = [eps.h, h, on, gn, NET_CRITIC, 0, 3, 200.0, p(q)]
    for k in (0, 1, 2, 3, 8):
        refused(lib.hp_episode_q_block(*[None if i == k else v for i, v in enumerate(good)]), "hp_episode_q_block: null argument")
    refused(lib.hp_episode_q_block(*[foreign.h if i == 2 else v for i, v in enumerate(good)]), "hp_episode_q_block: handles belong to different contexts")
    refused(lib.hp_episode_q_block(*[NET_ACTOR if i == 4 else v for i, v in enumerate(good)]), "hp_episode_q_block: net must be a critic")
    for first, n in ((0, 4), (2, 2), (-1, 2), (0, 0)):
        refused(lib.hp_episode_q_block(eps.h, h, on, gn, NET_CRITIC, first, n, 200.0, p(q)),
                rf"hp_episode_q_block: episodes \[{first}, {first + n}\) outside the block of 3")
    with pytest.raises(ValueError, match="outside the block of 3"):
        a.episode_q(eps, first=1, n=3)
    small = shaped_agent(20, 1, 3, 0.7)                         # its normalizers fit itself, not the block
    refused(lib.hp_episode_q_block(eps.h, small.h, small.o_norm.h, small.g_norm.h, NET_CRITIC, 0, 3, 200.0, p(q)),
            "hp_episode_q_block: the block has dimensions 27 / 3 / 4, normalizers and agent have 20 / 1 / 3")
    refused(lib.hp_episode_q_block(eps.h, small.h, on, gn, NET_CRITIC, 0, 3, 200.0, p(q)),
            r"hp_episode_q_block: normalizer sizes 27\+3 do not match the critic input 21")
    # an agent that is not slab-shaped: HP_ERR_STATE
    monkeypatch.setenv("RLARM_ENGINE", "layers")
    layers = make(None, T=10)
    monkeypatch.delenv("RLARM_ENGINE")
    refused(lib.hp_episode_q(layers.h, layers.o_norm.h, layers.g_norm.h, NET_CRITIC, p(obs), p(g), p(act), 3, 10, 200.0, p(q)),
            "hp_episode_q: the agent is not slab-shaped", code=-5)
    refused(lib.hp_episode_q_block(eps.h, layers.h, layers.o_norm.h, layers.g_norm.h, NET_CRITIC, 0, 3, 200.0, p(q)),
            "hp_episode_q_block: the agent is not slab-shaped", code=-5)
    # hp_episode_returns
    good = [c.h, p(ag), p(g), 3, 10, 3, 0.05, 0, 0.98, 1, p(G), p(q), p(stats)]
    swap = lambda k, x: [x if i == k else v for i, v in enumerate(good)]
    for k in (0, 1, 2, 10):
        refused(lib.hp_episode_returns(*swap(k, None)), "hp_episode_returns: null argument")
    refused(lib.hp_episode_returns(*swap(3, 0)), r"hp_episode_returns: n_episodes 0 outside \[1, ")
    refused(lib.hp_episode_returns(*swap(4, 0)), r"hp_episode_returns: T 0 outside \[1, ")
    refused(lib.hp_episode_returns(*swap(5, 257)), r"hp_episode_returns: goal_dim 257 outside \[1, 256\]")
    refused(lib.hp_episode_returns(*swap(7, 2)), "hp_episode_returns: reward_type 2 is neither 0")
    refused(lib.hp_episode_returns(*swap(9, 2)), "hp_episode_returns: tail 2 is neither 0")
    for gamma in (-0.5, 1.25, float("nan")):
        refused(lib.hp_episode_returns(*swap(8, gamma)), r"hp_episode_returns: gamma .* outside \[0, 1\]")
    refused(lib.hp_episode_returns(*swap(8, 1.0)), "hp_episode_returns: gamma 1 with tail 1")
    refused(lib.hp_episode_returns(*swap(11, None)), "hp_episode_returns: q_dev and critic_stats_dev come together")
    refused(lib.hp_episode_returns(*swap(12, None)), "hp_episode_returns: q_dev and critic_stats_dev come together")
    # hp_episode_returns_block
    good = [eps.h, 0, 3, 0.05, 0, 0.98, 1, p(G), p(q), p(stats)]
    for k in (0, 7):
        refused(lib.hp_episode_returns_block(*swap(k, None)), "hp_episode_returns_block: null argument")
    for first, n in ((0, 4), (2, 2), (-1, 2), (0, 0)):
        refused(lib.hp_episode_returns_block(eps.h, first, n, 0.05, 0, 0.98, 1, p(G), p(q), p(stats)),
                rf"hp_episode_returns_block: episodes \[{first}, {first + n}\) outside the block of 3")
    refused(lib.hp_episode_returns_block(*swap(5, 1.0)), "hp_episode_returns_block: gamma 1 with tail 1")
    with pytest.raises(ValueError, match="gamma 1 with tail 1"):
        eps.returns(0.05, 1.0)
    with pytest.raises(ValueError, match="q must be a contiguous float32 device tensor"):
        eps.returns(0.05, 0.98, q=q)
    # hp_episode_critic_summary
    refused(lib.hp_episode_critic_summary(None, p(stats), 3, p(summary)), "hp_episode_critic_summary: null argument")
    refused(lib.hp_episode_critic_summary(c.h, None, 3, p(summary)), "hp_episode_critic_summary: null argument")
    refused(lib.hp_episode_critic_summary(c.h, p(stats), 3, None), "hp_episode_critic_summary: null argument")
    refused(lib.hp_episode_critic_summary(c.h, p(stats), 0, p(summary)), "hp_episode_critic_summary: n_episodes 0 is not positive")
    c.synchronize()
    assert not q.any() and not G.any() and not stats.any() and not summary.any()          # a refused call launches nothing
