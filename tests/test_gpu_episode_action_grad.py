"""The actor-signal audit on the device (csrc/episode_action_grad.hip: hp_episode_action_grad, hp_episode_action_grad_block,
hp_episode_signal_stats, hp_episode_signal_stats_block, hp_episode_signal_summary; ddpg_agent.episode_action_grad,
episode_signal_stats, episode_signal_stats_host, args.audit_actor_signal).

dQ/du is compared with torch autograd through the oracle's critic (action_grad_cases.oracle_action_grad) at the project's bar for
a gradient (tests/test_gpu_teacher_forced.py): against the float32 oracle |device - oracle| <= 1e-4 max|g| over the block, against
the float64 one the device may be at most twice as far as the float32 oracle is, + 1e-6 max|g|.  A row with a critic
pre-activation below RELU_NOISE in float64 (at most one per case: counted by the oracle alone in test_episode_action_grad_cpu.py
for the freshly initialised cases, and asserted here for every case) is held to 2e-3 max|g| instead; no other row is excluded.
The forward values are compared bit for bit with hp_episode_policy / hp_episode_q, the columns and their summary bit for bit with
the host twins."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import action_grad_cases as cases
from conftest import bits
from gpu_common import ctx, fresh_rng, make_shape_episodes
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd import train_state as ts
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_ACTOR_TARGET, NET_CRITIC, NET_CRITIC_TARGET, ddpg_agent
from rl_arm_under_sparse_reward_amd.device_env import NativePickPlaceVecEnv, NativePointMassVecEnv, NativePushBlockVecEnv, generate_demos
from rl_arm_under_sparse_reward_amd.synthetic import SIGNAL_STATS, episode_signal_stats, episode_signal_summary
from episode_common import learner, move_actor, raw_policy, raw_q, refused, tree_bytes
from rollout_common import CONTACT, DEV, agent_on, dev_ptr as p, make, primed

pytestmark = pytest.mark.gpu
host = lambda *ts_: [v.cpu().numpy() if v is not None else None for v in ts_]
GUARD = 4        # rows behind the block in every output: the last slab's dead rows store nothing


# ------------------------------------------------------------------------------------------ helpers
def raw_grad(agent, obs, g, actions, at, target=0):
    """hp_episode_action_grad on uploaded arrays, into poisoned tensors with GUARD rows behind them: (dq_du, pi or None, q)"""
    o, gg, a = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(DEV) for v in (obs, g, actions))
    n, T = g.shape[:2]
    ad = int(agent.env_params['action'])
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    dq, pi, q = nan(n * T + GUARD, ad), nan(n * T + GUARD, ad), nan(n * T + GUARD)
    policy = at == "policy"
    with agent.ctx.torch_bridge():
        _lib.check(agent.lib.hp_episode_action_grad(agent.h, agent.o_norm.h, agent.g_norm.h, target, 0 if policy else 1, p(o), p(gg),
                                                    p(a) if not policy else None, n, T, float(agent.args.clip_obs),
                                                    p(pi) if policy else None, p(q), p(dq)))
    dq, pi, q = host(dq, pi, q)
    assert np.isnan(dq[n * T:]).all() and np.isnan(q[n * T:]).all() and np.isnan(pi[n * T:] if policy else pi).all()
    return dq[:n * T].reshape(n, T, ad), pi[:n * T].reshape(n, T, ad) if policy else None, q[:n * T].reshape(n, T)


def oracle_of(agent, obs, g, actions, at):
    """The oracle gradient from the agent's CURRENT parameters (hp_agent_get_params) and normalizer statistics"""
    pa = {k: v.detach().clone() for k, v in agent.actor_network.state_dict().items()}
    pc = {k: v.detach().clone() for k, v in agent.critic_network.state_dict().items()}
    x = cases.net_rows(obs, g, (agent.o_norm.mean, agent.o_norm.std), (agent.g_norm.mean, agent.g_norm.std), float(agent.args.clip_obs),
                       float(agent.args.clip_range))
    ad = int(agent.env_params['action'])
    return cases.oracle_action_grad(pa, pc, x, np.asarray(actions).reshape(-1, ad), float(agent.env_params['action_max']), at)


def assert_grad(got, o, what):
    """The project's gradient bar on one block; returns (largest error of a kept row / max|g|, tie-flagged rows)"""
    g32, g64, tie = o["g32"].astype(np.float64), o["g64"], o["tie"]
    dev = got.reshape(g32.shape).astype(np.float64)
    assert got.dtype == np.float32 and np.isfinite(dev).all(), what
    gmax = float(np.abs(g32).max())
    assert gmax > 0, what
    keep, ties = ~tie, int(tie.sum())
    err32, dev64, ref64 = np.abs(dev - g32).max(axis=1), np.abs(dev - g64).max(axis=1), np.abs(g32 - g64).max(axis=1)
    worst = float(err32[keep].max()) / gmax if keep.any() else 0.0
    print(f"{what}: max|g| {gmax:.3e}; kept rows: |device - oracle32| {worst * gmax:.3e} ({worst:.2e} max|g|), "
          f"|device - oracle64| {float(dev64[keep].max()) if keep.any() else 0.0:.3e}, |oracle32 - oracle64| "
          f"{float(ref64[keep].max()) if keep.any() else 0.0:.3e}; tie-flagged rows {ties}"
          + (f": |device - oracle32| {float(err32[tie].max()):.3e}" if ties else ""))
    assert ties <= 1, (what, ties)
    if keep.any():
        assert err32[keep].max() <= 1e-4 * gmax, (what, "vs float32 oracle", float(err32[keep].max()), gmax)
        assert dev64[keep].max() <= 2.0 * ref64[keep].max() + 1e-6 * gmax, (what, "vs float64", float(dev64[keep].max()),
                                                                           float(ref64[keep].max()), gmax)
    if ties:
        assert err32[tie].max() <= 2e-3 * gmax, (what, "ReLU tie", float(err32[tie].max()), gmax)
    return worst, ties


def check_cases(agent, shape, what):
    """Every block, clip and `at` of action_grad_cases on one agent: the gradient against the oracle, the forward bit for bit
    against hp_episode_policy / hp_episode_q on the same block"""
    worst, ties, default_clip = 0.0, 0, agent.args.clip_obs
    for block in cases.BLOCKS:
        obs, g, actions = cases.block_inputs(shape, block)
        for clip_obs in cases.CLIPS:
            agent.args.clip_obs = clip_obs
            if clip_obs < 1.0 and block[0] * block[1] > 4:
                assert np.mean(np.abs(obs[:, :block[1]]) > clip_obs) > 0.1          # the clip bites
            for at in cases.ATS:
                dq, pi, q = raw_grad(agent, obs, g, actions, at)
                o = oracle_of(agent, obs, g, actions, at)
                w, t = assert_grad(dq, o, f"{what} {shape} block {block} clip_obs {clip_obs} at {at}")
                worst, ties = max(worst, w), ties + t
                if at == "policy":
                    want_pi, want_q = raw_policy(agent, obs, g)
                    assert np.array_equal(bits(pi), bits(want_pi)) and np.array_equal(bits(q), bits(want_q)), (what, block, at)
                    assert np.allclose(pi.reshape(-1, shape[2]), o["pi"], rtol=1e-5, atol=1e-6)
                else:
                    assert pi is None and np.array_equal(bits(q), bits(raw_q(agent, obs, g, actions))), (what, block, at)
                assert np.allclose(q.reshape(-1), o["q"], rtol=1e-5, atol=1e-6)
    agent.args.clip_obs = default_clip
    print(f"{what} {shape}: largest error of a kept row {worst:.2e} max|g|, {ties} tie-flagged rows in all cases")


def fresh_agent(shape):
    """An agent of a shape holding action_grad_cases.fresh_parameters: the networks and statistics the CPU test counted ties on"""
    params = cases.fresh_parameters(shape)
    torch.manual_seed(0)
    agent = ddpg_agent(Args(batch_size=64, buffer_size=8 * 20), None, cases.env_of(shape), rng=fresh_rng(5))
    assert float(agent.args.clip_range) == cases.CLIP_RANGE
    for slot, name in ((NET_ACTOR, "actor"), (NET_CRITIC, "critic")):
        agent._set_flat(slot, params["flat"][name])
        assert np.array_equal(agent._get_flat(slot), params["flat"][name])
    agent.o_norm.set_stats(*params["o_stats"])
    agent.g_norm.set_stats(*params["g_stats"])
    return agent


def twin_of(agent, stats, dq_du, pi, actions, flat=1e-3):
    """The six columns of an audit against the twin fed the device's dq_du and pi and the recorded actions, by bytes"""
    stats, dq_du, pi = (v.cpu().numpy() if isinstance(v, torch.Tensor) else v for v in (stats, dq_du, pi))
    want = episode_signal_stats(pi, dq_du, actions, agent.env_params['action_max'], action_l2=agent.args.action_l2, flat=flat)
    assert stats.dtype == np.float64 and stats.shape == (pi.shape[0], 6) and np.array_equal(bits(stats), bits(want)), (stats, want)
    return want


def device_summary(c, stats):
    out = torch.full((6,), float("nan"), dtype=torch.float64, device=DEV)
    with c.torch_bridge():
        _lib.check(c.lib.hp_episode_signal_summary(c.h, p(stats), stats.shape[0], p(out)))
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1. / 2. against the oracle, forward bits
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_dq_du_of_a_freshly_initialised_agent_equals_the_oracle(shape):
    check_cases(fresh_agent(shape), shape, "fresh")


def test_dq_du_after_training_cycles_reads_the_stepped_weights():
    """Two train_cycles on a small buffer at batch 64, one in each launch form of an update sequence (3 updates: chain launch +
    tile launch per update; 13: the split launch), as test_pi_and_q_pi_after_training_cycles_read_the_stepped_weights trains
    them: a dX-order fragment copy that a launch form did not step would fail here."""
    T, n_eps, batch, shape = 20, 8, 64, cases.SHAPES[0]
    torch.manual_seed(0)
    agent = ddpg_agent(Args(batch_size=batch, buffer_size=4 * n_eps * T, lr_critic=0.01, lr_actor=0.01), None, cases.env_of(shape, T),
                       rng=fresh_rng(3))
    before = agent._get_flat(NET_CRITIC)
    form, forms = C.c_int32(), []
    for cycle, n_batches in enumerate((3, 13)):
        agent.train_cycle(make_shape_episodes(n_eps, 27, 3, 4, T, seed=20 + cycle), n_batches=n_batches)
        _lib.check(agent.lib.hp_agent_update_form(agent.h, n_batches, C.byref(form)))
        forms.append(form.value)
    assert forms == [0, 1], forms
    assert np.abs(agent._get_flat(NET_CRITIC) - before).max() > 1e-3
    check_cases(agent, shape, "trained")
    obs, g, actions = cases.block_inputs(shape, cases.BLOCKS[1])
    want = oracle_of(agent, obs, g, actions, "policy")["g32"]
    agent._set_flat(NET_CRITIC, before)
    moved = np.abs(raw_grad(agent, obs, g, actions, "policy")[0].reshape(want.shape) - want).max()       # the bar tells the weights apart
    assert moved > 1e-2 * np.abs(want).max(), moved


# ------------------------------------------------------------------------------------------ 3. the columns
@pytest.mark.parametrize("T", [10, 70])
def test_columns_of_exploring_pick_and_place_episodes_equal_the_twin(T):
    a = move_actor(agent_on(NativePickPlaceVecEnv, 3, T, env_seed=21, random_eps=0.3), 7)
    eps = a.collect_episodes_device(n_rollouts=5, epoch=0)
    actions = eps.numpy()[3]
    stats, dq_du, pi, q_pi = a.episode_signal_stats(eps)
    assert stats.is_cuda and dq_du.dtype == pi.dtype == q_pi.dtype == torch.float32 and tuple(dq_du.shape) == (5, T, actions.shape[2])
    want = twin_of(a, stats, dq_du, pi, actions)
    assert (want[:, 0] > 0).all() and ((0 <= want[:, 1:3]) & (want[:, 1:3] <= 1)).all() and (np.abs(want[:, 3]) <= 1).all(), want
    assert np.array_equal(bits(device_summary(a.ctx, stats)), bits(episode_signal_summary(want)))
    for x, y in zip(host(pi, q_pi), host(*a.episode_policy(eps))):
        assert np.array_equal(bits(x), bits(y))
    rec = host(*a.episode_action_grad(eps, at="recorded"))
    assert rec[1] is None and np.array_equal(bits(rec[2]), bits(a.episode_q(eps).cpu().numpy())) and not np.array_equal(rec[0], dq_du.cpu().numpy())
    mid = float(np.median(want[:, 0]))                 # a bound about half of the steps' norms lie below
    biting = twin_of(a, a.episode_signal_stats(eps, flat=mid)[0], dq_du, pi, actions, flat=mid)
    assert 0 < biting[:, 1].mean() < 1, biting[:, 1]


def test_columns_of_pick_and_place_demonstrations_equal_the_twin():
    env = NativePickPlaceVecEnv(4, seed=0, device=DEV, max_timesteps=100, step_scale=0.2)
    env.enable_device_reset(ctx())
    demos = generate_demos(env, 4)
    assert demos.kept == 4
    torch.manual_seed(0)
    a = make(env, T=100)
    primed(a)
    stats, dq_du, pi, q_pi = a.episode_signal_stats(demos.episodes)
    want = twin_of(a, stats, dq_du, pi, demos.numpy()[3])
    assert np.array_equal(bits(device_summary(a.ctx, stats)), bits(episode_signal_summary(want)))
    print("toward_recorded and linear_adv of the demonstrations per episode:", want[:, 3], want[:, 4])


# ------------------------------------------------------------------------------------------ 4. sub-ranges, host episodes
def test_sub_ranges_of_a_push_block_collection_and_host_episodes():
    """Nine episodes of T = 20 on eight environments: first * T is a multiple of 4 for every `first`, so every sub-range starts
    on a slab boundary of the whole-block call and has its bits.  The same episodes read back and handed in as host arrays go
    through the same kernels: the same bits again."""
    a = agent_on(NativePushBlockVecEnv, 8, 20, env_seed=21, env_kw=CONTACT, random_eps=0.3)
    eps = a.collect_episodes_device(n_rollouts=9)
    batch = eps.numpy()
    whole = host(*a.episode_signal_stats(eps))
    twin_of(a, whole[0], whole[1], whole[2], batch[3])
    for first, n in ((3, 4), (0, 1), (8, 1), (1, 8)):
        for x, w in zip(host(*a.episode_signal_stats(eps, first=first, n=n)), whole):
            assert np.array_equal(bits(x), bits(w[first:first + n])), (first, n)
        for at in cases.ATS:
            full, part = host(*a.episode_action_grad(eps, at=at)), host(*a.episode_action_grad(eps, at=at, first=first, n=n))
            for x, w in zip(part, full):
                assert (x is None and w is None) or np.array_equal(bits(x), bits(w[first:first + n])), (first, n, at)
    for x, w in zip(host(*a.episode_action_grad(eps, first=7)), whole[1:]):
        assert np.array_equal(bits(x), bits(w[7:]))
    out = a.episode_signal_stats_host(batch)
    assert all(isinstance(v, np.ndarray) for v in out) and len(out) == 4
    for x, y in zip(out, whole):
        assert x.dtype == y.dtype and np.array_equal(bits(x), bits(y))
    o = oracle_of(a, batch[0], batch[2], batch[3], "policy")
    assert_grad(whole[1], o, "push-block collection")
    with pytest.raises(ValueError, match="episode_signal_stats_host: obs"):
        a.episode_signal_stats_host([batch[0], batch[1][:, :-1], batch[2], batch[3]])
    with pytest.raises(ValueError, match="outside the block of 9"):
        a.episode_signal_stats(eps, first=8, n=2)
    with pytest.raises(ValueError, match="neither 'policy' nor 'recorded'"):
        a.episode_action_grad(eps, at="target")


# ------------------------------------------------------------------------------------------ 5. learn()
def test_audit_actor_signal_is_the_twins_and_changes_nothing_else(tmp_path, capsys):
    """Two epochs of learn() on two native point-mass environments with the option on and off (audit_policy on in both): the same
    rates, policy audit, printed lines, checkpoint files, training state and streams to the byte, an empty list with it off; with
    it on, one dict per epoch.  A third run whose audit call is wrapped keeps what the device computed on each epoch's last
    collection: its entries are the same, and they are the twins' on those arrays."""
    kw = dict(audit_policy=True)
    on = learner(tmp_path, "on", False, audit_actor_signal=True, state_path=str(tmp_path / "on.npz"), **kw)
    off = learner(tmp_path, "off", False, state_path=str(tmp_path / "off.npz"), **kw)
    probe = learner(tmp_path, "probe", False, audit_actor_signal=True, **kw)
    kept, collected = [], []
    audit, collect = probe.episode_signal_stats, probe.collect_episodes_device

    def audit_and_keep(eps, **kwargs):
        out = audit(eps, **kwargs)
        assert eps is collected[-1][0] and collected[-1][1] and kwargs["n"] == probe.args.num_rollouts_per_mpi
        kept.append(host(*out) + [eps.numpy()[3][:kwargs["n"]]])
        return out

    def collect_and_note(*args, **kwargs):
        eps = collect(*args, **kwargs)
        collected.append((eps, kwargs.get("explore", True)))
        return eps

    probe.episode_signal_stats, probe.collect_episodes_device = audit_and_keep, collect_and_note
    printed, finals = [], []
    for a in (on, off, probe):
        np.random.seed(11)
        a.learn()
        printed.append([line for line in capsys.readouterr().out.splitlines() if "eval success rate" in line or "buffer size" in line])
        finals.append((a.rng.get_state(), np.random.get_state()))
    assert off.actor_signal_audit == [] and len(on.actor_signal_audit) == 2 and len(on.success_rates) == 2
    assert on.success_rates == off.success_rates and on.policy_audit == off.policy_audit and len(on.policy_audit) == 2
    assert on.eval_metrics == off.eval_metrics and on.eval_critic == off.eval_critic
    strip = lambda lines: [line.split("] ", 1)[-1] for line in lines]
    assert strip(printed[0]) == strip(printed[1]) and len(printed[0]) == 3
    for x, y in zip(finals[0], finals[1]):                     # the device stream and numpy's, as learn() leaves them
        assert all(np.array_equal(u, v) for u, v in zip(x, y))
    files_on, files_off = tree_bytes(tmp_path / "on"), tree_bytes(tmp_path / "off")
    assert sorted(files_on) == sorted(files_off) and len(files_on) >= 1 and all(files_on[k] == files_off[k] for k in files_on)
    for slot in (NET_ACTOR, NET_CRITIC, NET_ACTOR_TARGET, NET_CRITIC_TARGET):
        assert np.array_equal(bits(on._get_flat(slot)), bits(off._get_flat(slot))), slot
    sa, sb = ts.read_state(ts.rank_path(str(tmp_path / "on.npz"), 0)), ts.read_state(ts.rank_path(str(tmp_path / "off.npz"), 0))
    assert sorted(sa[0]) == sorted(sb[0])
    for name in sa[0]:
        assert np.array_equal(bits(sa[0][name]), bits(sb[0][name])), name
    # the entries
    assert probe.actor_signal_audit == on.actor_signal_audit and probe.success_rates == on.success_rates and len(kept) == 2
    for m, (stats, dq_du, pi, q_pi, actions) in zip(on.actor_signal_audit, kept):
        assert tuple(m) == SIGNAL_STATS
        want = twin_of(on, stats, dq_du, pi, actions)
        assert np.array_equal(bits(np.array([m[k] for k in SIGNAL_STATS])), bits(episode_signal_summary(want))), (m, want)
        assert m["grad_norm"] > 0 and 0 <= m["flat_share"] <= 1 and 0 <= m["reg_share"] <= 1 and m["trunk_signal"] > 0
    assert not np.array_equal(kept[0][1], kept[1][1])          # two collections, two sets of weights


def test_audit_actor_signal_on_the_host_path(tmp_path, capsys):
    """learn() with host environments goes through episode_signal_stats_host on the last collect_episodes result, and leaves the
    run as it is without the option"""
    from rl_arm_under_sparse_reward_amd.synthetic import PointMassGoalEnv
    runs = []
    for audit in (True, False):
        torch.manual_seed(0)
        np.random.seed(11)
        env = PointMassGoalEnv(seed=30, max_timesteps=10, distance_threshold=0.15)
        a = make(env, T=10, seed=5, n_epochs=2, n_cycles=2, n_batches=2, n_test_rollouts=2, buffer_episodes=40, num_rollouts_per_mpi=2,
                 save_dir=str(tmp_path / f"host{int(audit)}"), env_name="pm", audit_actor_signal=audit)
        primed(a)
        if audit:
            stats_host, kept = a.episode_signal_stats_host, []
            a.episode_signal_stats_host = lambda batch, **kwargs: kept.append((batch, stats_host(batch, **kwargs))) or kept[-1][1]
        a.learn()
        capsys.readouterr()
        runs.append((a, [a._get_flat(s) for s in (NET_ACTOR, NET_CRITIC)], np.random.get_state()))
    (a, flat_a, np_a), (b, flat_b, np_b) = runs
    assert b.actor_signal_audit == [] and len(a.actor_signal_audit) == 2 and a.success_rates == b.success_rates
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(flat_a, flat_b))
    assert all(np.array_equal(u, v) for u, v in zip(np_a, np_b))
    assert len(kept) == 2
    for m, (batch, (stats, dq_du, pi, q_pi)) in zip(a.actor_signal_audit, kept):
        assert batch[3].shape[0] == 2 and tuple(m) == SIGNAL_STATS
        want = twin_of(a, stats, dq_du, pi, batch[3])
        assert np.array_equal(bits(np.array([m[k] for k in SIGNAL_STATS])), bits(episode_signal_summary(want)))


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_carry_the_librarys_message():
    torch.manual_seed(0)
    a = make(NativePointMassVecEnv(2, seed=1, device=DEV, max_timesteps=10), T=10)
    primed(a)
    lib, c = a.lib, a.ctx
    eps = a.collect_episodes_device(n_rollouts=3, explore=False)
    obs, g = torch.zeros((3, 11, 27), dtype=torch.float64, device=DEV), torch.zeros((3, 10, 3), dtype=torch.float64, device=DEV)
    act = torch.zeros((3, 10, 4), dtype=torch.float64, device=DEV)
    pi, dq = torch.zeros((4, 10, 4), dtype=torch.float32, device=DEV), torch.zeros((4, 10, 4), dtype=torch.float32, device=DEV)
    q = torch.zeros((4, 10), dtype=torch.float32, device=DEV)
    stats, summary = torch.zeros((4, 6), dtype=torch.float64, device=DEV), torch.zeros(6, dtype=torch.float64, device=DEV)
    h, on, gn = a.h, a.o_norm.h, a.g_norm.h
    # hp_episode_action_grad
    name = "hp_episode_action_grad"
    good = [h, on, gn, 0, 0, p(obs), p(g), p(act), 3, 10, 200.0, p(pi), p(q), p(dq)]
    swap = lambda k, x: [x if i == k else v for i, v in enumerate(good)]
    for k in (0, 1, 2, 5, 6, 12, 13):
        refused(lib.hp_episode_action_grad(*swap(k, None)), f"{name}: null argument")
    for target in (2, -1):
        refused(lib.hp_episode_action_grad(*swap(3, target)), f"{name}: target .* is neither 0")
    for at in (2, -1):
        refused(lib.hp_episode_action_grad(*swap(4, at)), f"{name}: at {at} is neither 0")
    refused(lib.hp_episode_action_grad(*[1 if i == 4 else None if i == 7 else v for i, v in enumerate(good)]),
            rf"{name}: at 1 \(the recorded action\) needs actions_dev")
    refused(lib.hp_episode_action_grad(*swap(11, None)), rf"{name}: at 0 \(the policy's action\) needs pi_dev")
    refused(lib.hp_episode_action_grad(*swap(3, 1)), f"{name}: the target networks keep no dX-order fragments", code=-5)
    refused(lib.hp_episode_action_grad(h, gn, gn, 0, 0, p(obs), p(g), p(act), 3, 10, 200.0, p(pi), p(q), p(dq)),
            rf"{name}: normalizer sizes 3\+3 do not match the network input 30")
    refused(lib.hp_episode_action_grad(*swap(8, 0)), rf"{name}: n_episodes 0 outside \[1, ")
    refused(lib.hp_episode_action_grad(*swap(9, 0)), rf"{name}: T 0 outside \[1, ")
    refused(lib.hp_episode_action_grad(*[(1 << 23) if i == 8 else (1 << 20) if i == 9 else v for i, v in enumerate(good)]),
            f"{name}: .* more than one launch holds")
    other = _lib.Context(0)                                     # a second context on the same device
    from rl_arm_under_sparse_reward_amd.normalizer import normalizer
    foreign = normalizer(27, default_clip_range=5, ctx=other)
    refused(lib.hp_episode_action_grad(*swap(1, foreign.h)), f"{name}: handles belong to different contexts")
    # hp_episode_action_grad_block
    name = "hp_episode_action_grad_block"
    good = [eps.h, h, on, gn, 0, 0, 0, 3, 200.0, p(pi), p(q), p(dq)]
    for k in (0, 1, 2, 3, 10, 11):
        refused(lib.hp_episode_action_grad_block(*swap(k, None)), f"{name}: null argument")
    refused(lib.hp_episode_action_grad_block(*swap(2, foreign.h)), f"{name}: handles belong to different contexts")
    refused(lib.hp_episode_action_grad_block(*swap(4, 3)), f"{name}: target 3 is neither 0")
    refused(lib.hp_episode_action_grad_block(*swap(5, 7)), f"{name}: at 7 is neither 0")
    refused(lib.hp_episode_action_grad_block(*swap(9, None)), rf"{name}: at 0 \(the policy's action\) needs pi_dev")
    refused(lib.hp_episode_action_grad_block(*swap(4, 1)), f"{name}: the target networks keep no dX-order fragments", code=-5)
    assert lib.hp_episode_action_grad_block(*[1 if i == 5 else None if i == 9 else v for i, v in enumerate(good)]) == 0     # at 1 needs no pi
    for first, n in ((0, 4), (2, 2), (-1, 2), (0, 0)):
        refused(lib.hp_episode_action_grad_block(eps.h, h, on, gn, 0, 0, first, n, 200.0, p(pi), p(q), p(dq)),
                rf"{name}: episodes \[{first}, {first + n}\) outside the block of 3")
    with pytest.raises(ValueError, match="outside the block of 3"):
        a.episode_action_grad(eps, first=1, n=3)
    with pytest.raises(_lib.HpError, match="target networks keep no dX-order fragments"):
        a.episode_action_grad(eps, target=True)
    small = ddpg_agent(Args(batch_size=64, buffer_size=160), None, cases.env_of((20, 1, 3, 0.7)), rng=fresh_rng(5))
    refused(lib.hp_episode_action_grad_block(eps.h, small.h, small.o_norm.h, small.g_norm.h, 0, 0, 0, 3, 200.0, p(pi), p(q), p(dq)),
            f"{name}: the block has dimensions 27 / 3 / 4, normalizers and agent have 20 / 1 / 3")
    # an agent that is not slab-shaped: HP_ERR_STATE
    narrow = ddpg_agent(Args(batch_size=64, buffer_size=80), None, cases.env_of((27, 3, 4, 0.5), 10, hidden=128), rng=fresh_rng(5))
    refused(lib.hp_episode_action_grad(narrow.h, narrow.o_norm.h, narrow.g_norm.h, 0, 0, p(obs), p(g), p(act), 3, 10, 200.0, p(pi), p(q), p(dq)),
            r"hp_episode_action_grad: the agent is not slab-shaped \(hidden 128", code=-5)
    refused(lib.hp_episode_action_grad_block(eps.h, narrow.h, narrow.o_norm.h, narrow.g_norm.h, 0, 0, 0, 3, 200.0, p(pi), p(q), p(dq)),
            rf"{name}: the agent is not slab-shaped \(hidden 128", code=-5)
    # hp_episode_signal_stats
    name = "hp_episode_signal_stats"
    good = [c.h, p(pi), p(dq), p(act), 3, 10, 4, 0.5, 1.0, 1e-3, p(stats)]
    for k in (0, 1, 2, 3, 10):
        refused(lib.hp_episode_signal_stats(*swap(k, None)), f"{name}: null argument")
    refused(lib.hp_episode_signal_stats(*swap(4, 0)), rf"{name}: n_episodes 0 outside \[1, ")
    refused(lib.hp_episode_signal_stats(*swap(5, 0)), rf"{name}: T 0 outside \[1, ")
    for ad in (0, 257):
        refused(lib.hp_episode_signal_stats(*swap(6, ad)), rf"{name}: act_dim {ad} outside \[1, 256\]")
    for amax in (0.0, -0.5, float("inf"), float("nan")):
        refused(lib.hp_episode_signal_stats(*swap(7, amax)), f"{name}: max_action .* is not a positive number")
    for l2 in (-0.1, float("inf"), float("nan")):
        refused(lib.hp_episode_signal_stats(*swap(8, l2)), f"{name}: action_l2 .* is not a finite number")
    for flat in (-0.1, float("nan")):
        refused(lib.hp_episode_signal_stats(*swap(9, flat)), f"{name}: flat .* is not a finite number")
    # hp_episode_signal_stats_block
    name = "hp_episode_signal_stats_block"
    good = [eps.h, p(pi), p(dq), 0, 3, 0.5, 1.0, 1e-3, p(stats)]
    for k in (0, 1, 2, 8):
        refused(lib.hp_episode_signal_stats_block(*swap(k, None)), f"{name}: null argument")
    for first, n in ((0, 4), (2, 2), (-1, 2), (0, 0)):
        refused(lib.hp_episode_signal_stats_block(eps.h, p(pi), p(dq), first, n, 0.5, 1.0, 1e-3, p(stats)),
                rf"{name}: episodes \[{first}, {first + n}\) outside the block of 3")
    refused(lib.hp_episode_signal_stats_block(*swap(6, -2.0)), rf"{name}: action_l2 -2 is not a finite number")
    # hp_episode_signal_summary
    name = "hp_episode_signal_summary"
    refused(lib.hp_episode_signal_summary(None, p(stats), 3, p(summary)), f"{name}: null argument")
    refused(lib.hp_episode_signal_summary(c.h, None, 3, p(summary)), f"{name}: null argument")
    refused(lib.hp_episode_signal_summary(c.h, p(stats), 3, None), f"{name}: null argument")
    refused(lib.hp_episode_signal_summary(c.h, p(stats), 0, p(summary)), f"{name}: n_episodes 0 is not positive")
    c.synchronize()
    assert not pi.any() and not stats.any() and not summary.any()          # a refused call launches nothing
