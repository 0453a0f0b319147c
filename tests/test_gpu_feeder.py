"""Multi-process experience feeder (BASELINE config 5): worker processes step the environments, one
batched policy call per timestep, episodes land in a device-registered shared-memory ring and are stored by DMA."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import bits
from gpu_common import fresh_rng
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import NET_ACTOR, NET_CRITIC, ddpg_agent
from rl_arm_under_sparse_reward_amd.feeder import EpisodeFeeder
from rl_arm_under_sparse_reward_amd.synthetic import PointMassGoalEnv

pytestmark = pytest.mark.gpu
T = 50


def make(n_envs, seed=3, **kw):
    specs = [(PointMassGoalEnv, dict(seed=10 + i, max_timesteps=T)) for i in range(n_envs)]
    envs = [cls(**k) for cls, k in specs]
    args = Args(batch_size=128, buffer_size=64 * T, **kw)
    agent = ddpg_agent(args, envs, envs[0].env_params, rng=fresh_rng(seed))
    rs = np.random.RandomState(0)
    agent.o_norm.update(rs.normal(0.2, 0.3, size=(400, 27))); agent.o_norm.recompute_stats()
    agent.g_norm.update(rs.normal(0.25, 0.1, size=(400, 3))); agent.g_norm.recompute_stats()
    return agent, specs


def test_worker_processes_reproduce_the_in_process_lockstep_rollouts():
    torch.manual_seed(0)
    agent, specs = make(6)
    want = agent.collect_episodes(6, explore=False)              # same environments (same seeds), stepped in this process
    feeder = EpisodeFeeder(agent, specs, n_workers=3, n_slots=2)
    try:
        slot = feeder.collect_wave(explore=False)
        got = feeder.episodes(slot)
        for a, b in zip(want, got):
            assert a.shape == b.shape and np.array_equal(bits(a), bits(np.ascontiguousarray(b)))
        # store_episode straight out of the shared ring (no CPU copy), then the next wave into the other slot
        feeder.store_wave(slot)
        assert agent.buffer.current_size == 6
        for key, src in zip(("obs", "ag", "g", "actions"), got):
            assert np.array_equal(agent.buffer.buffers[key][:6], src), key
        slot2 = feeder.collect_wave(explore=True)
        assert slot2 != slot
        acts = feeder.episodes(slot2)[3]
        assert np.all(np.abs(acts) <= 0.5) and not np.array_equal(acts, got[3])      # exploration noise applied by the workers
        assert np.array_equal(acts, acts.astype(np.float32).astype(np.float64))       # float32 actions, like the reference
        late = feeder.collect_wave(epoch=100, explore=True)                            # waits for slot 0's DMA ticket
        assert late == slot and np.all(np.abs(feeder.episodes(late)[3]) <= np.float32(0.15))   # ddpg_agent.py:118-119 (float32 clip)
        del got, acts
    finally:
        feeder.close()


def test_train_cycle_from_feeder_equals_train_cycle_on_the_same_episodes():
    outs = []
    for via_feeder in (False, True):
        torch.manual_seed(0)
        agent, specs = make(4, seed=9)
        feeder = EpisodeFeeder(agent, specs, n_workers=2, n_slots=2)
        try:
            for cycle in range(3):
                slot = feeder.collect_wave(explore=False)
                if via_feeder:
                    agent.train_cycle_from_feeder(feeder, slot, n_batches=4)
                else:
                    agent.train_cycle([np.array(a) for a in feeder.episodes(slot)], n_batches=4)
            outs.append((agent._get_flat(NET_ACTOR), agent._get_flat(NET_CRITIC), agent.last_losses(12),
                         agent.o_norm.mean, agent.buffer.buffers["ag"][:12], agent.rng.get_state()[2]))
        finally:
            feeder.close()
    for a, b in zip(*outs):
        assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b)))


def test_policy_snapshot_needs_the_slab_engine(monkeypatch):
    """A layer-engine agent has no fused policy kernel to run a snapshot on: hp_agent_policy_snapshot refuses with HP_ERR_STATE."""
    monkeypatch.setenv("RLARM_ENGINE", "layers")
    torch.manual_seed(0)
    agent, _ = make(2)
    monkeypatch.delenv("RLARM_ENGINE")
    status = agent.lib.hp_agent_policy_snapshot(agent.h, agent.o_norm.h, agent.g_norm.h)
    assert status == -5, status                                  # HP_ERR_STATE
    with pytest.raises(_lib.HpError, match=r"hp_agent_policy_snapshot: needs the fused policy kernel \(slab8 engine\)"):
        _lib.check(status)


def test_policy_snapshot_serves_the_feeder_while_the_learner_moves_on():
    torch.manual_seed(0)
    agent, specs = make(4)
    rs = np.random.RandomState(1)
    obs, g = rs.normal(0.2, 0.5, size=(9, 27)), rs.normal(0.25, 0.2, size=(9, 3))

    def snap_act(rows=9):
        out = np.empty((rows, 4), np.float32)
        d = C.c_double
        _lib.check(agent.lib.hp_agent_act_snapshot(agent.h, _lib.ptr(obs, d), _lib.ptr(g, d), rows, 0.0, _lib.ptr(out, C.c_float)))
        return out

    with pytest.raises(_lib.HpError):
        snap_act()                                               # no snapshot yet
    agent.policy_snapshot()
    before = agent.act(obs, g)
    assert np.array_equal(bits(snap_act()), bits(before))        # same arithmetic as hp_agent_act
    for rows in (1, 5):                                          # other row counts that leave the last 4-row slab partly empty
        assert np.array_equal(bits(snap_act(rows)), bits(agent.act(obs[:rows], g[:rows]))), rows
    from rl_arm_under_sparse_reward_amd.synthetic import make_episodes
    agent.buffer.store_episode(make_episodes(8, seed=2, T=T, mode="walk"))
    agent._update_network(5)                                     # the learner's actor moves ...
    assert not np.array_equal(agent.act(obs, g), before)
    assert np.array_equal(bits(snap_act()), bits(before))        # ... the feeder still sees its snapshot
    agent.policy_snapshot()
    agent.ctx.synchronize()
    assert np.array_equal(bits(snap_act()), bits(agent.act(obs, g)))
    # a feeder on the snapshot policy collects waves while training cycles are queued
    feeder = EpisodeFeeder(agent, specs, n_workers=2, n_slots=2, snapshot_policy=True)
    try:
        agent._update_network(40)                                # enqueued, asynchronous
        slot = feeder.collect_wave(explore=False)
        assert np.all(np.isfinite(feeder.episodes(slot)[0]))
    finally:
        feeder.close()
