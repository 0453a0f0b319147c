"""Rollout side next to the hot path: batched policy call, lockstep feeder, learn() end to end on
the stand-in GoalEnv (rl_arm_under_sparse_reward_amd/synthetic.py).  The real PyBullet envs are out of scope."""
import numpy as np
import pytest
import torch

from conftest import bits
from gpu_common import fresh_rng
from oracle import ddpg_update as oupd
from oracle.running_norm import RunningNorm
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
from rl_arm_under_sparse_reward_amd.synthetic import PointMassGoalEnv
from rollout_common import make, primed

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("engine", ["", "RLARM_ENGINE=layers"])       # fused policy kernel | layer-per-launch fallback
@pytest.mark.parametrize("rows", [1, 5, 64, 100])
def test_act_equals_preproc_plus_actor_and_tracks_oracle(rows, engine, monkeypatch):
    """hp_agent_act = _preproc_inputs (:163-171) + actor forward: bit-identical to the two-step device path, and within
    float32 rounding of the oracle's normalise + forward."""
    if engine:
        monkeypatch.setenv(*engine.split("="))
    torch.manual_seed(0)
    agent = make(None)
    rs = primed(agent)
    obs = rs.normal(0.2, 0.6, size=(rows, 27)); obs[0, :3] = [40.0, -40.0, 0.2]     # exercises the +-5 clip
    g = rs.normal(0.25, 0.2, size=(rows, 3))
    got = agent.act(obs, g)
    assert got.shape == (rows, 4) and got.dtype == np.float32
    x = np.concatenate([agent.o_norm.normalize(obs), agent.g_norm.normalize(g)], axis=1).astype(np.float32)
    two_step = agent.actor_network(x)
    assert np.array_equal(bits(got), bits(np.asarray(two_step)))
    one = agent.act(obs[0], g[0])                               # single rows, as the reference's loop passes them
    assert one.shape == (4,) and np.array_equal(bits(one), bits(got[0]))
    on, gn = RunningNorm(27, default_clip_range=5), RunningNorm(3, default_clip_range=5)
    rs2 = np.random.RandomState(0)
    on.update(rs2.normal(0.2, 0.3, size=(400, 27))); on.recompute_stats()
    gn.update(rs2.normal(0.25, 0.1, size=(400, 3))); gn.recompute_stats()
    xo = torch.tensor(np.concatenate([on.normalize(obs), gn.normalize(g)], axis=1), dtype=torch.float32)
    assert np.array_equal(bits(xo.numpy()), bits(x))            # inputs: same float64 arithmetic, same bits
    want = oupd.actor_forward({k: v for k, v in agent.actor_network.state_dict().items()}, xo, 0.5).numpy()
    assert np.allclose(got, want, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        agent.act(obs, g[:-1] if rows > 1 else np.zeros((2, 3)))


def test_lockstep_feeder_equals_one_env_at_a_time():
    """K environments stepped in lockstep with one batched policy call give the episodes K sequential rollouts give
    (noise off; every row of the batched forward is independent of its neighbours)."""
    torch.manual_seed(0)
    agent = make([PointMassGoalEnv(seed=10 + i, max_timesteps=50) for i in range(3)])
    primed(agent)
    together = agent.collect_episodes(3, explore=False)
    apart = []
    for i in range(3):
        agent.envs = [PointMassGoalEnv(seed=10 + i, max_timesteps=50)]
        apart.append(agent.collect_episodes(1, explore=False))
    for k in range(4):
        assert np.array_equal(together[k], np.concatenate([a[k] for a in apart]))
    assert together[0].shape == (3, 51, 27) and together[3].shape == (3, 50, 4) and together[0].dtype == np.float64
    # more episodes than environments: waves of len(envs)
    agent.envs = [PointMassGoalEnv(seed=10 + i, max_timesteps=50) for i in range(2)]
    five = agent.collect_episodes(5, explore=False)
    assert five[0].shape == (5, 51, 27)
    assert np.array_equal(five[0][:2], together[0][:2])


def test_exploration_draws_follow_the_reference_order():
    """_select_actions (:174-184) consumes numpy's global stream as randn(action), uniform(action), binomial(1)."""
    torch.manual_seed(0)
    agent = make([PointMassGoalEnv(seed=1, max_timesteps=50)])
    pi = np.array([0.1, -0.2, 0.3, 0.05], np.float32)
    np.random.seed(4)
    got = agent._select_actions(torch.from_numpy(pi).unsqueeze(0))
    np.random.seed(4)
    a = pi.copy()                      # float32, updated in place like the reference's `action += ...`
    a += agent.args.noise_eps * 0.5 * np.random.randn(4)
    a = np.clip(a, -0.5, 0.5)
    ra = np.random.uniform(-0.5, 0.5, 4)
    a += np.random.binomial(1, agent.args.random_eps, 1)[0] * (ra - a)
    assert got.dtype == np.float32 and np.array_equal(got, a)


def test_learn_reaches_goals_on_the_point_mass(tmp_path):
    """learn() (:92-161) end to end: rollouts -> store -> normalizer -> 40 updates -> polyak, evaluation, checkpoint per
    epoch.  HER + DDPG solves the reach task within a few hundred episodes (the CPU oracle learner does in 8 epochs of
    10 cycles; tools/experiments notes), so success must rise from chance to >= 0.8."""
    np.random.seed(0)
    torch.manual_seed(0)
    envs = [PointMassGoalEnv(seed=1 + i, max_timesteps=50) for i in range(2)]
    args = Args(batch_size=256, buffer_size=400 * 50, n_epochs=14, n_cycles=10, n_test_rollouts=20, noise_eps=0.2,
                save_dir=str(tmp_path), env_name="point_mass")
    agent = ddpg_agent(args, envs, envs[0].env_params, rng=fresh_rng(5))
    before = agent._eval_agent()
    agent.learn()
    assert len(agent.success_rates) == 14
    # three seeds of this recipe (tools/ubench/learn_probe.py) are at >= 0.9 from epoch 8 on; the bar leaves room for
    # the run-to-run differences any change of float32 summation order brings
    assert max(agent.success_rates[-3:]) >= 0.8 and before <= 0.4, (before, agent.success_rates)
    assert agent.buffer.current_size == 14 * 10 * 2
    saved = sorted(p.name for p in (tmp_path / "point_mass").iterdir())
    assert len(saved) == 14 and all(name.endswith("_model.pt") for name in saved)


def test_learn_follows_the_reference_run_on_the_stand_in_env(tmp_path):
    """learn() end to end against tests/golden/rollout.npz = the reference's own learn() on this env (N1 + N3): with the
    single shared random stream the device run consumes exactly the reference's random words (final MT19937 state
    bit-identical: every exploration draw, overflow slot and HER index in the reference's order), stores the same
    episodes and reports the same evaluation success rates.  Episode values carry the float32 rounding differences of
    the actor forward through the closed loop (point mass: contractive), hence the small absolute tolerances."""
    from conftest import load_golden
    from gpu_common import state_equal
    from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_CRITIC
    g = load_golden("rollout.npz")
    c = {k: (float(v) if "." in v else int(v)) for k, v in g["cfg"]}
    env = PointMassGoalEnv(seed=c["env_seed"], max_timesteps=100, distance_threshold=c["distance_threshold"])
    args = Args(n_epochs=c["n_epochs"], n_cycles=c["n_cycles"], n_batches=c["n_batches"], n_test_rollouts=c["n_test_rollouts"],
                noise_eps=c["noise_eps"], random_eps=c["random_eps"], buffer_size=c["buffer_episodes"] * 100,
                save_dir=str(tmp_path), env_name="stand_in")
    agent = ddpg_agent(args, env, env.env_params, rng=fresh_rng(0))
    agent._set_flat(NET_ACTOR, g["init_actor"]); agent._set_flat(NET_CRITIC, g["init_critic"])
    agent.lib.hp_agent_sync_targets(agent.h)
    stored = []
    orig = agent.train_cycle
    agent.train_cycle = lambda eps, n_batches=None: (stored.append([np.array(a) for a in eps]), orig(eps, n_batches))[1]
    np.random.seed(c["np_seed"])
    agent.learn()
    assert len(stored) == c["n_epochs"] * c["n_cycles"]
    for i, batch in enumerate(stored):
        tol = 2e-6 if i == 0 else 2e-4          # cycle 0: untouched initial weights; later cycles: fp32 updates in between
        for nm, a in zip(("obs", "ag", "g", "actions"), batch):
            want = g[f"cycle{i}_{nm}"].astype(np.float64)
            assert a.shape == want.shape and float(np.abs(a - want).max()) <= tol, (i, nm, float(np.abs(a - want).max()))
    key, pos = np.random.get_state()[1:3]
    assert np.array_equal(key, g["key"]) and pos == int(g["pos"])            # same words, same order, to the last draw
    assert state_equal(agent.rng, g["key"], g["pos"])
    assert np.allclose(agent.success_rates, g["success_rates"], atol=1.0 / c["n_test_rollouts"] + 1e-9)
    assert np.allclose(agent.o_norm.mean, g["o_mean"], atol=1e-5) and np.allclose(agent.g_norm.std, g["g_std"], atol=1e-5)
    rel = np.linalg.norm(agent._get_flat(NET_ACTOR) - g["actor_final"]) / np.linalg.norm(g["actor_final"] - g["init_actor"])
    assert rel <= 0.1, rel
    assert sorted(p.name for p in (tmp_path / "stand_in").iterdir()) == list(g["checkpoints"])
