"""One exploration stream per environment (csrc/rng_streams.hip, k_rollout_step_streams in csrc/rollout.hip,
random.DeviceRandomStreams, ddpg_agent.enable_explore_streams): every stream against its own numpy RandomState to the last word,
independence of the width, the same bits as the single-stream kernel for the same stream, the closed loop against n host workers,
the training state, and the refusals.  Everything goes through the C ABI."""
import numpy as np
import pytest
import torch

from conftest import bits
from gpu_common import ctx, fresh_rng, host_select_actions, ulp_distance
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.device_env import DeviceEpisodes, PointMassVecEnv, binomial1_qn
from rl_arm_under_sparse_reward_amd.random import DeviceRandomStreams
from rl_arm_under_sparse_reward_amd.replay_buffer import DeviceEpisodeBuffer
from rl_arm_under_sparse_reward_amd.synthetic import PointMassGoalEnv
from rollout_common import DEV, assert_states_bit_equal, dev_ptr as p, make, primed

pytestmark = pytest.mark.gpu
NET_ACTOR = 0


# --------------------------------------------------------------------------------------------------------------- 1. seeding
@pytest.mark.parametrize("n", [5, 1000])
def test_seeding_equals_numpy_for_every_stream(n):
    c = ctx()
    base = 4000
    s = DeviceRandomStreams(n, base_seed=base, ctx=c)
    assert len(s) == n
    states = s.get_states()
    for i in (range(n) if n <= 64 else list(range(0, n, 37)) + [n - 1]):
        assert_states_bit_equal(s.get_state(i), np.random.RandomState(base + i).get_state(), i)
    for i in range(n):
        assert_states_bit_equal(states[i], np.random.RandomState(base + i).get_state(), i)
    seeds = np.random.RandomState(n).randint(0, 2**32 - 1, n, dtype=np.int64)
    seeds[0], seeds[-1] = 0, 2**32 - 1
    s.seed(seeds=seeds)
    keys, pos, has, val = s.get_arrays()
    for i in range(n):
        want = np.random.RandomState(int(seeds[i])).get_state()
        assert np.array_equal(keys[i], want[1]) and pos[i] == want[2] == 624 and has[i] == 0 and val[i] == 0.0, i
    s2 = DeviceRandomStreams(n, seeds=list(seeds), ctx=c)          # the constructor form
    assert all(np.array_equal(a, b) for a, b in zip(s2.get_arrays(), (keys, pos, has, val)))


def test_set_state_round_trips_a_pending_cached_normal():
    s = DeviceRandomStreams(4, base_seed=7, ctx=ctx())
    rs = np.random.RandomState(5)
    rs.randn(3)
    st = rs.get_state()
    assert st[3] == 1
    s.set_state(2, st)
    assert_states_bit_equal(s.get_state(2), st, "one")
    for i in (0, 1, 3):                                               # the neighbours did not move
        assert_states_bit_equal(s.get_state(i), np.random.RandomState(7 + i).get_state(), i)
    all_states = s.get_states()
    assert_states_bit_equal(all_states[2], st, "bulk get")
    s.seed(base_seed=7)
    assert s.get_state(2)[3:] == (0, 0.0)                             # numpy's seed() drops the cached normal
    s.set_states(all_states)
    assert_states_bit_equal(s.get_state(2), st, "bulk set")


# -------------------------------------------------------------------------------------------- 2. teacher-forced exploration
def step_streams(c, eps, streams, t, o, a, g, act, noise_eps, random_eps, clip_abs, explore=1):
    qn = binomial1_qn(random_eps)[0]
    with c.torch_bridge():
        _lib.check(c.lib.hp_rollout_step_streams(eps.h, None, None, None, streams.h if streams is not None else None, t, p(o), p(a),
                                                 p(g), explore, noise_eps, random_eps, qn, clip_abs, p(act)))


@pytest.mark.parametrize("epoch", [0, 100])
@pytest.mark.parametrize("n_envs,dims", [(1, (27, 3, 4)), (3, (27, 3, 4)), (64, (27, 3, 4)), (257, (27, 3, 4)), (1000, (27, 3, 4)),
                                         (3, (10, 2, 3))])
def test_teacher_forced_exploration_follows_one_randomstate_per_env(n_envs, dims, epoch):
    """Env i is handed its own policy row and must consume what `_select_actions` driven by RandomState(seed_i) alone consumes:
    after every step, for every env, key, pos and has_gauss are numpy's, every action lies within one float32 spacing, the
    cached normal within 4 ulp (then realigned from numpy with the bulk setter, as the single-stream test does).  Elements not
    bit-equal are counted and printed.  A single stream seeded beside the run is never touched."""
    od, gd, ad = dims
    T, noise_eps, random_eps, amax = 100, 0.2, 0.3, 0.5
    c = ctx()
    buf = DeviceEpisodeBuffer(8, T, od, gd, ad, ctx=c)
    eps = DeviceEpisodes(c, buf, n_envs)
    _lib.check(c.lib.hp_rollout_set_action_max(eps.h, amax))
    base = 300 + n_envs
    streams = DeviceRandomStreams(n_envs, base_seed=base, ctx=c)
    host = [np.random.RandomState(base + i) for i in range(n_envs)]
    bystander = fresh_rng(99)
    bystander_state = bystander.get_state()
    prs = np.random.RandomState(1)
    unequal = total = 0
    want_act = np.empty((n_envs, T, ad))
    rows = [prs.uniform(-1, 1, (T + 1, n_envs, d)) for d in (od, gd, gd)]
    for t in range(T):
        pi = prs.uniform(-0.6, 0.6, (n_envs, ad)).astype(np.float32)
        o, a, g = (torch.from_numpy(r[t]).to(DEV) for r in rows)
        act = torch.from_numpy(pi).to(DEV)
        step_streams(c, eps, streams, t, o, a, g, act, noise_eps, random_eps, 0.15 if epoch >= 100 else 0.0)
        want = np.stack([host_select_actions(host[i], pi[i], noise_eps, random_eps, amax, epoch >= 100) for i in range(n_envs)])
        got = act.cpu().numpy()
        keys, pos, has, val = streams.get_arrays()
        sn = [h.get_state() for h in host]
        nk, npos, nhas = np.stack([s[1] for s in sn]), np.array([s[2] for s in sn]), np.array([s[3] for s in sn])
        nval = np.array([s[4] for s in sn])
        assert np.array_equal(keys, nk) and np.array_equal(pos, npos) and np.array_equal(has, nhas), t
        assert int(ulp_distance(val, nval).max()) <= 4, t
        assert want.dtype == np.float32 and np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))), t
        unequal += int((bits(got).reshape(-1, 4) != bits(want).reshape(-1, 4)).any(axis=1).sum())
        total += got.size
        want_act[:, t] = got
        streams.set_arrays(nk, npos, nhas, nval)     # carry numpy's cached normals so later steps start from identical states
    o, a = torch.from_numpy(rows[0][T]).to(DEV), torch.from_numpy(rows[1][T]).to(DEV)
    with c.torch_bridge():
        _lib.check(c.lib.hp_rollout_finish(eps.h, p(o), p(a)))
    print(f"per-env streams n_envs={n_envs} dims={dims} epoch={epoch}: {unequal} of {total} float32 action elements not bit-equal")
    obs, ag, g, actions = eps.numpy()
    assert np.array_equal(obs, rows[0].transpose(1, 0, 2)) and np.array_equal(ag, rows[1].transpose(1, 0, 2))
    assert np.array_equal(g, rows[2][:T].transpose(1, 0, 2)) and np.array_equal(bits(actions), bits(want_act))
    assert_states_bit_equal(bystander.get_state(), bystander_state, "bystander")


def test_a_step_without_exploration_touches_no_stream():
    n, T = 5, 10
    c = ctx()
    buf = DeviceEpisodeBuffer(8, T, 27, 3, 4, ctx=c)
    eps = DeviceEpisodes(c, buf, n)
    streams = DeviceRandomStreams(n, base_seed=11, ctx=c)
    before = streams.get_arrays()
    prs = np.random.RandomState(2)
    o, a, g = (torch.from_numpy(prs.uniform(-1, 1, (n, d))).to(DEV) for d in (27, 3, 3))
    pi = prs.uniform(-0.6, 0.6, (n, 4)).astype(np.float32)
    for s in (streams, None):
        act = torch.from_numpy(pi).to(DEV)
        step_streams(c, eps, s, 0, o, a, g, act, 0.2, 0.3, 0.15, explore=0)
        assert np.array_equal(bits(act.cpu().numpy()), bits(np.clip(pi.astype(np.float64), -0.15, 0.15).astype(np.float32)))
    assert all(np.array_equal(x, y) for x, y in zip(streams.get_arrays(), before))


# ------------------------------------------------------------------------------------------------- 3. width independence
def run_wide(n_envs, seeds, pis, T, rows_active=None):
    """T teacher-forced exploring steps of a wave of `rows_active` (default all) environments; -> (actions [T, rows, ad], streams)"""
    c = ctx()
    ad = pis.shape[-1]
    buf = DeviceEpisodeBuffer(8, T, 27, 3, ad, ctx=c)
    eps = DeviceEpisodes(c, buf, n_envs)
    _lib.check(c.lib.hp_rollout_set_action_max(eps.h, 0.5))
    k = n_envs if rows_active is None else rows_active
    if k != n_envs:
        _lib.check(c.lib.hp_rollout_begin(eps.h, 0, k))
    streams = DeviceRandomStreams(n_envs, seeds=seeds[:n_envs], ctx=c)
    prs = np.random.RandomState(3)
    o, a, g = (torch.from_numpy(prs.uniform(-1, 1, (k, d))).to(DEV) for d in (27, 3, 3))
    out = []
    for t in range(T):
        act = torch.from_numpy(np.ascontiguousarray(pis[t, :k])).to(DEV)
        step_streams(c, eps, streams, t, o, a, g, act, 0.2, 0.3, 0.0)
        out.append(act.cpu().numpy())
    return np.stack(out), streams


def test_an_envs_draws_do_not_depend_on_the_width():
    T = 40
    seeds = list(np.random.RandomState(8).randint(0, 2**31, 64))
    pis = np.random.RandomState(9).uniform(-0.6, 0.6, (T, 64, 4)).astype(np.float32)
    wide, s_wide = run_wide(64, seeds, pis, T)
    narrow, s_narrow = run_wide(3, seeds, pis, T)
    assert np.array_equal(bits(wide[:, :3]), bits(narrow))
    for i in range(3):
        assert_states_bit_equal(s_wide.get_state(i), s_narrow.get_state(i), i)
    assert not np.array_equal(s_wide.get_state(0)[1], np.random.RandomState(seeds[0]).get_state()[1])     # 40 steps outlast a key


def test_a_partial_wave_advances_only_its_own_streams():
    T = 40
    seeds = [50, 51, 52, 53]
    pis = np.random.RandomState(9).uniform(-0.6, 0.6, (T, 4, 4)).astype(np.float32)
    part, s_part = run_wide(4, seeds, pis, T, rows_active=2)
    full, s_full = run_wide(4, seeds, pis, T)
    assert np.array_equal(bits(part), bits(full[:, :2]))
    for i in (0, 1):
        assert_states_bit_equal(s_part.get_state(i), s_full.get_state(i), i)
    for i in (2, 3):
        assert_states_bit_equal(s_part.get_state(i), np.random.RandomState(seeds[i]).get_state(), i)
        assert not np.array_equal(s_full.get_state(i)[1], np.random.RandomState(seeds[i]).get_state()[1])


# ------------------------------------------------------------------------------------------------- 4. same code, same bits
@pytest.mark.parametrize("ad", [4, 3])
def test_one_stream_gives_the_single_stream_kernels_bits(ad):
    """One env whose stream starts at the state of a single hp_rng: hp_rollout_step_streams and hp_rollout_step give bit-identical
    actions, recorded blocks and final states (ad = 3 leaves a cached normal pending on every other step)."""
    T, noise_eps, random_eps = 100, 0.2, 0.3
    c = ctx()
    buf = DeviceEpisodeBuffer(8, T, 27, 3, ad, ctx=c)
    eps_a, eps_b = DeviceEpisodes(c, buf, 1), DeviceEpisodes(c, buf, 1)
    for e in (eps_a, eps_b):
        _lib.check(c.lib.hp_rollout_set_action_max(e.h, 0.5))
    single = fresh_rng(1234)
    single.standard_normal(1)                  # start with a cached normal pending
    streams = DeviceRandomStreams(1, base_seed=0, ctx=c)
    streams.set_state(0, single.get_state())
    qn = binomial1_qn(random_eps)[0]
    prs = np.random.RandomState(4)
    o, a, g = (torch.from_numpy(prs.uniform(-1, 1, (1, d))).to(DEV) for d in (27, 3, 3))
    for t in range(T):
        pi = prs.uniform(-0.6, 0.6, (1, ad)).astype(np.float32)
        act_a, act_b = torch.from_numpy(pi).to(DEV), torch.from_numpy(pi).to(DEV)
        clip = 0.15 if t >= T // 2 else 0.0
        step_streams(c, eps_a, streams, t, o, a, g, act_a, noise_eps, random_eps, clip)
        with c.torch_bridge():
            _lib.check(c.lib.hp_rollout_step(eps_b.h, None, None, None, single.h, t, p(o), p(a), p(g), 1, noise_eps, random_eps, qn,
                                             clip, p(act_b)))
        assert np.array_equal(bits(act_a.cpu().numpy()), bits(act_b.cpu().numpy())), t
    single.mark_normals_drawn()
    assert_states_bit_equal(streams.get_state(0), single.get_state(), "final")
    for x, y in zip(eps_a.numpy(), eps_b.numpy()):
        assert np.array_equal(bits(x), bits(y))


# ------------------------------------------------------------------------------------------------------- 5. closed loop
def test_closed_loop_equals_one_host_worker_per_env():
    """collect_episodes_device with streams against n reference-style workers on the host: env i = PointMassGoalEnv(seed + i),
    its own RandomState(base + i), `agent.act` on its row and the host `_select_actions`.  Tolerance of a first cycle (2e-6: the
    policy's float32 outputs feed back through the environment); stream keys and positions exact.  Seven episodes on four
    environments: the second wave is partial and advances the first three streams only."""
    n, n_rollouts, T, env_seed, base = 4, 7, 50, 10, 900
    torch.manual_seed(0)
    agent = make(PointMassVecEnv(n, seed=env_seed, device=DEV, max_timesteps=T), T=T, noise_eps=0.05)
    primed(agent)
    streams = agent.enable_explore_streams(base_seed=base)
    learner_before = agent.rng.get_state()
    got = agent.collect_episodes_device(n_rollouts=n_rollouts, explore=True).numpy()
    assert_states_bit_equal(agent.rng.get_state(), learner_before, "learner stream")     # untouched by exploring steps
    amax = agent.env_params["action_max"]
    envs = [PointMassGoalEnv(seed=env_seed + i, max_timesteps=T) for i in range(n)]
    host = [np.random.RandomState(base + i) for i in range(n)]
    want = [[], [], [], []]
    for first in (0, n):
        for i in range(min(n, n_rollouts - first)):
            o = envs[i].reset()
            ep = ([], [], [], [])
            for _ in range(T):
                pi = agent.act(o["observation"], o["desired_goal"])
                action = host_select_actions(host[i], pi, agent.args.noise_eps, agent.args.random_eps, amax, False)
                for dst, v in zip(ep, (o["observation"], o["achieved_goal"], o["desired_goal"], action)):
                    dst.append(np.array(v, dtype=np.float64))
                o = envs[i].step(action)[0]
            ep[0].append(np.array(o["observation"])); ep[1].append(np.array(o["achieved_goal"]))
            for dst, src in zip(want, ep):
                dst.append(np.array(src))
    for nm, a, b in zip(("obs", "ag", "g", "actions"), got, want):
        b = np.array(b)
        worst = float(np.abs(a - b).max())
        print(f"closed loop {nm}: worst absolute difference {worst:.3e}")
        assert a.shape == b.shape and worst <= 2e-6, (nm, worst)
    for i in range(n):
        sd, sn = streams.get_state(i), host[i].get_state()
        assert np.array_equal(sd[1], sn[1]) and sd[2] == sn[2] and sd[3] == sn[3], i


# ---------------------------------------------------------------------------------------------------- 6. training state
def test_train_state_carries_the_streams(tmp_path):
    """Save mid-run with streams enabled and a cached normal pending in stream 0; a fresh agent resumed from the file reproduces
    the next collect_episodes_device and train_cycle bit for bit.  A state with streams is refused by an agent without them and
    the other way round, and both messages name the arrays."""
    from rl_arm_under_sparse_reward_amd.train_state import STREAM_ARRAYS, StateError, read_state, verify
    T, n = 50, 3

    def build(streams=True):
        torch.manual_seed(0)
        a = make(PointMassVecEnv(n, seed=4, device=DEV, max_timesteps=T), T=T, seed=12, n_batches=3, buffer_episodes=20)
        if streams:
            a.enable_explore_streams(base_seed=70)
        return a

    a = build()
    a.train_cycle(a.collect_episodes_device())
    rs = np.random.RandomState(0)
    rs.set_state(a.explore_streams.get_state(0))
    rs.randn(1)                                                # leaves the second normal of the pair cached
    a.explore_streams.set_state(0, rs.get_state())
    assert a.explore_streams.get_state(0)[3] == 1
    saved = a.explore_streams.get_arrays()
    path = a.save_training_state(tmp_path / "mid.npz")
    arrays, manifest = read_state(path)
    assert manifest["explore_streams"]["n"] == n
    for name, x in zip(STREAM_ARRAYS, saved):
        assert arrays[name].dtype == x.dtype and np.array_equal(bits(arrays[name]), bits(x)), name
    assert arrays["explore_stream_has_gauss"][0] == 1 and arrays["explore_stream_gauss"][0] == rs.get_state()[4]
    verify(path)
    env_rs = [r.get_state() for r in a.vec_env.rs]
    want = a.collect_episodes_device().numpy()
    a.train_cycle(a._rollouts[n])
    want_params, want_state, want_streams = a._get_flat(NET_ACTOR), a.rng.get_state(), a.explore_streams.get_arrays()

    b = build()
    b.explore_streams.seed(base_seed=1)                        # whatever they held is replaced by the file's
    b.load_training_state(path)
    assert all(np.array_equal(x, y) for x, y in zip(b.explore_streams.get_arrays(), saved))
    for r, st in zip(b.vec_env.rs, env_rs):
        r.set_state(st)
    got = b.collect_episodes_device()
    for x, y in zip(got.numpy(), want):
        assert np.array_equal(bits(x), bits(y))
    b.train_cycle(got)
    assert np.array_equal(bits(b._get_flat(NET_ACTOR)), bits(want_params))
    sb = b.rng.get_state()
    assert np.array_equal(sb[1], want_state[1]) and sb[2:] == want_state[2:]
    for x, y in zip(b.explore_streams.get_arrays(), want_streams):
        assert np.array_equal(bits(x), bits(y))

    plain = build(streams=False)
    before = plain._get_flat(NET_ACTOR)
    with pytest.raises(StateError, match="explore_stream_keys.*explore_stream_gauss"):
        plain.load_training_state(path)
    assert np.array_equal(bits(plain._get_flat(NET_ACTOR)), bits(before))            # refused before anything changed
    plain.train_cycle(plain.collect_episodes_device())
    plain_path = plain.save_training_state(tmp_path / "plain.npz")
    arrays_plain, manifest_plain = read_state(plain_path)
    assert "explore_streams" not in manifest_plain and not [k for k in arrays_plain if k.startswith("explore_stream")]
    with pytest.raises(StateError, match="explore_stream_keys.*explore_stream_gauss.*missing"):
        b.load_training_state(plain_path)


# ------------------------------------------------------------------------------------------------------------ 7. errors
def test_refusals_carry_the_librarys_message():
    c = ctx()
    with pytest.raises(ValueError, match=r"hp_streams_create: 0 streams"):
        DeviceRandomStreams(0, ctx=c)
    with pytest.raises(ValueError, match=r"hp_streams_seed: 2 seeds for 3 streams"):
        DeviceRandomStreams(3, seeds=[1, 2], ctx=c)
    with pytest.raises(ValueError, match="Seed must be between 0 and"):
        DeviceRandomStreams(3, base_seed=2**32 - 2, ctx=c)
    s = DeviceRandomStreams(2, base_seed=1, ctx=c)
    with pytest.raises(ValueError, match=r"stream 2 outside \[0, 2\)"):
        s.get_state(2)
    T = 10
    buf = DeviceEpisodeBuffer(8, T, 27, 3, 4, ctx=c)
    eps = DeviceEpisodes(c, buf, 4)
    prs = np.random.RandomState(2)
    o, a, g = (torch.from_numpy(prs.uniform(-1, 1, (4, d))).to(DEV) for d in (27, 3, 3))
    act = torch.from_numpy(prs.uniform(-0.6, 0.6, (4, 4)).astype(np.float32)).to(DEV)
    before = s.get_arrays()
    with pytest.raises(ValueError, match="a wave of 4 environments is wider than the array of 2 streams"):
        step_streams(c, eps, s, 0, o, a, g, act, 0.2, 0.3, 0.0)
    with pytest.raises(ValueError, match="hp_rollout_step_streams: exploration needs the stream array"):
        step_streams(c, eps, None, 0, o, a, g, act, 0.2, 0.3, 0.0)
    assert all(np.array_equal(x, y) for x, y in zip(s.get_arrays(), before))
    _lib.check(c.lib.hp_rollout_begin(eps.h, 0, 2))             # a wave the array covers is accepted
    step_streams(c, eps, s, 0, o, a, g, act, 0.2, 0.3, 0.0)
    assert s.get_state(0)[2] != 624
    # the agent: streams for another number of environments, and no vectorised environment at all
    torch.manual_seed(0)
    agent = make(PointMassVecEnv(3, seed=1, device=DEV, max_timesteps=T), T=T)
    agent.explore_streams = s
    with pytest.raises(ValueError, match="2 exploration streams for 3 environments"):
        agent.collect_episodes_device()
    with pytest.raises(ValueError, match="no vectorised device environment"):
        make(None).enable_explore_streams()


# ------------------------------------------------------------------------------------- the public switch: args.explore_streams
def test_learn_turns_the_streams_on_from_args_and_resumes_with_them(tmp_path):
    """learn() with args.explore_streams: the streams appear before the first wave as RandomState(args.seed + rank * n_envs + i),
    exploring waves move them and leave `agent.rng` alone, evaluation waves move neither; a second learn() that resumes from the
    state the first one saved (args.resume) enables the mode before it loads and starts from the saved streams."""
    from rl_arm_under_sparse_reward_amd.arguments import Args
    from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
    n, T, seed = 3, 50, 77

    def build(n_epochs, **extra):
        torch.manual_seed(0)
        env = PointMassVecEnv(n, seed=2, device=DEV, max_timesteps=T)
        args = Args(n_epochs=n_epochs, n_cycles=2, n_batches=2, n_test_rollouts=2, num_rollouts_per_mpi=n, buffer_size=20 * T,
                    save_dir=str(tmp_path), env_name="streams", explore_streams=True, seed=seed)
        args.state_path = str(tmp_path / "run.npz")
        for k, v in extra.items():
            setattr(args, k, v)
        agent = ddpg_agent(args, env, env.env_params, rng=fresh_rng(0))
        seen, orig = [], agent.collect_episodes_device

        def watched(*a, **k):
            s0, r0 = agent.explore_streams.get_states(), agent.rng.get_state()
            out = orig(*a, **k)
            seen.append((k.get("explore", True), s0, agent.explore_streams.get_states(), r0, agent.rng.get_state()))
            return out

        agent.collect_episodes_device = watched
        return agent, seen

    agent, seen = build(1)
    assert agent.explore_streams is None
    agent.learn()
    assert len(agent.explore_streams) == n and [s[0] for s in seen[:2]] == [True, True] and not seen[-1][0]
    for i in range(n):
        assert_states_bit_equal(seen[0][1][i], np.random.RandomState(seed + 0 * n + i).get_state(), i)
    for explore, s0, s1, r0, r1 in seen:
        assert_states_bit_equal(r0, r1, "agent.rng across a collection")
        moved = [not (np.array_equal(a[1], b[1]) and a[2:] == b[2:]) for a, b in zip(s0, s1)]
        assert all(moved) if explore else not any(moved), (explore, moved)
    final = agent.explore_streams.get_states()

    resumed, seen2 = build(2, resume=str(tmp_path / "run.npz"))
    resumed.learn()
    assert resumed.resumed_at == (1, 0) and seen2[0][0]
    for i in range(n):
        assert_states_bit_equal(seen2[0][1][i], final[i], i)
