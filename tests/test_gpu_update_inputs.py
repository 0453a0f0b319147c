"""The minibatch an update launch gathers FOR ITSELF, bit for bit against the CPU oracle.

An update does not train on what hp_buffer_sample_dev returns: every launch form gathers its own minibatch inside the launch
(s8_gather in the chain kernels, s8_gather_ahead in spare workgroups / behind the weight-gradient tiles, k_gather_fused in front
of the slab32 and layers engines, the split launch's own calls).  hp_agent_debug_inputs (rlarm_hip_debug.h) copies the two
input sets of the agent's arena out -- set 0 = XA, XP, XT, R, set 1 = XA2, XP2, XT2, R2 -- and everything here is compared by
bits with EpisodeStore.sample + oracle.ddpg_update.minibatch_tensors driven from the same stream state as the device:

    XA   norm(obs) | norm(g') | 0 ... | float32(action) / float32(max_action) at act_off | 0 ...      every column, every row
    XP   norm(obs) | norm(g') | 0 ...                                                                  columns below act_off
    XT   norm(obs_next) | norm(g') | 0 ...                                                             columns below act_off
    R    the float32 bits of compute_reward

and rows B .. Mp - 1 of all of these are +0 (the weight-gradient GEMMs sum over Mp rows).  The action columns of XP and XT
are NOT gather output: the chains write pi(x) and pi'(x_next) there (padded rows included: tanh of the bias chain), no
weight-gradient GEMM reads them (the actor's K1 is act_off, the target nets have no gradients), and they are not compared.

What a set holds after hp_agent_sample_and_update(n) (agent.hip: enqueue_updates; asserted below, per sequence):

  * slab8 (4-, 8-, 16-row slabs, with or without dw64) and the split launch -- the plan always gathers ahead.  Update 0 gathers
    in-chain into set 0; update u gathers update u + 1 into set (u + 1) & 1.  So set (n - 1) & 1 holds update n - 1, set
    (n - 2) & 1 holds update n - 2, and after n = 1 set 1 is untouched.  The in-chain gather (s8_gather; the split launch's
    critic / actor chains) writes XA, XP[:, :act_off] and R; x_next goes to the LDS only (Xout = nullptr), so XT[:, :act_off]
    of a set that holds update 0 is left as it was -- asserted as "unchanged", and x_next of that form is covered through the
    next update's s8_gather_ahead copy (n = 3: both sets come from s8_gather_ahead).  The split launch's target chains gather
    x_next of the NEXT update a second time into their LDS (Q.tgs): that copy is never observable either.
  * slab32 -- gathers ahead too; update 0 comes from k_gather_fused (XA, XP, XT, R all in global memory), later ones from
    s8_gather_ahead behind the weight-gradient tiles (k_gemm_lds_adam_ride*, k_dw64_adam).
  * layers -- never ahead: every update's k_gather_fused writes set 0; set 1 is never written.

Every sequence draws fresh minibatches (the stream runs on), consecutive minibatches are asserted to differ, and a set the
form does not write is asserted unchanged, so neither stale contents nor swapped sets can pass.  No tolerance anywhere."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import bits, load_golden
from gpu_common import fresh_rng, make_shape_episodes, state_equal
from oracle.ddpg_update import minibatch_tensors
from oracle.her_replay import EpisodeStore
from oracle.running_norm import RunningNorm, update_normalizers
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent
from rl_arm_under_sparse_reward_amd.synthetic import make_episodes
from update_common import HP, HP_ENV, expect_engine, pairs_as_one_step_episodes, set_launch, threshold_pairs

pytestmark = pytest.mark.gpu
SPLIT_MIN_UPDATES = 12      # agent.h: the shortest sequence that takes the split form by itself


def _u32(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.uint32)


def _env(od, gd, ad, T, amax=0.7):
    return {"obs": od, "goal": gd, "action": ad, "action_max": amax, "max_timesteps": T}


def _make(batch, env, n_eps, eps, seed=7, replay_k=4, prime=(0.1, 0.35, 0.2, 0.15)):
    """Agent + oracle twin: the same episodes stored, the same stream state, normalizers with the same non-trivial statistics
    (narrow enough that clip_range 1.5 acts on clipped observations: (0.8 - 0.1) / 0.35 = 2)."""
    od, gd, ad, T = env["obs"], env["goal"], env["action"], env["max_timesteps"]
    args = Args(batch_size=batch, buffer_size=n_eps * T, replay_k=replay_k, **HP)
    rng = fresh_rng(seed)
    torch.manual_seed(0)
    agent = ddpg_agent(args, None, dict(env), rng=rng)
    rs = np.random.RandomState(seed)
    st = EpisodeStore(T, od, gd, ad, n_eps * T)
    st.store_episode(eps, rs)
    agent.buffer.store_episode(eps)
    on, gn = RunningNorm(od, default_clip_range=args.clip_range), RunningNorm(gd, default_clip_range=args.clip_range)
    prs = np.random.RandomState(seed + 1000)
    for ref, dev, v in ((on, agent.o_norm, prs.normal(prime[0], prime[1], (64, od))),
                        (gn, agent.g_norm, prs.normal(prime[2], prime[3], (64, gd)))):
        ref.update(v); dev.update(v)
        ref.recompute_stats(); dev.recompute_stats()
    side = SimpleNamespace(st=st, rs=rs, on=on, gn=gn, rng=rng, args=args, env=env, fp=float(agent.her_module.future_p),
                           batch=batch, clipped_obs=False, clipped_range=False)
    _norms_equal(agent, side)
    return agent, side


def _norms_equal(agent, side):
    for dev, ref in ((agent.o_norm, side.on), (agent.g_norm, side.gn)):
        assert np.array_equal(bits(dev.mean), bits(ref.mean)) and np.array_equal(bits(dev.std), bits(ref.std))


def _oracle_minibatch(side, dims):
    """The oracle's next minibatch as the arena rows it must become (padded rows and columns +0), and its index draw."""
    tr, idx = side.st.sample(side.batch, side.fp, side.rs)
    x, xn, a, r = (t.numpy() for t in minibatch_tensors(tr, side.on, side.gn, clip_obs=side.args.clip_obs))
    B, Mp, ldx, off, ad, xdim = (dims[k] for k in ("B", "Mp", "ldx", "act_off", "act_dim", "xdim"))
    assert (B, ad, xdim) == (side.batch, a.shape[1], x.shape[1]) and Mp % 32 == 0 and Mp >= B and off >= xdim and ldx >= off + ad
    want = {k: np.zeros((Mp, ldx), np.float32) for k in ("XA", "XP", "XT")}
    want["R"] = np.zeros(Mp, np.float32)
    want["XA"][:B, :xdim] = x
    want["XA"][:B, off:off + ad] = a.astype(np.float32) / np.float32(side.env["action_max"])      # float32 division (models.py:38)
    want["XP"][:B, :xdim] = x
    want["XT"][:B, :xdim] = xn
    want["R"][:B] = r[:, 0]
    side.clipped_obs |= bool(np.any(np.abs(tr["obs"]) > side.args.clip_obs))
    side.clipped_range |= bool(np.any(np.abs(x) == np.float32(side.args.clip_range)))
    return want, idx, tr


def _same(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    diff = _u32(got) != _u32(want)
    if diff.any():
        where = np.argwhere(diff)
        i = tuple(where[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} words differ; first at {i}: got {got[i]!r} "
                             f"(0x{int(_u32(got)[i]):08x}), want {want[i]!r} (0x{int(_u32(want)[i]):08x}); rows "
                             f"{sorted(set(int(w[0]) for w in where))[:8]}")


def _check_set(got, want, before, what, x_next):
    """One input set against the minibatch it must hold.  x_next False: the form left x_next in the LDS, XT's gathered columns
    must be what they were before the sequence."""
    off = got["act_off"]
    _same(got["XA"], want["XA"], f"{what} XA")
    _same(got["XP"][:, :off], want["XP"][:, :off], f"{what} XP[:, :act_off]")
    _same(got["R"], want["R"], f"{what} R")
    if x_next:
        _same(got["XT"][:, :off], want["XT"][:, :off], f"{what} XT[:, :act_off]")
    else:
        _same(got["XT"][:, :off], before["XT"][:, :off], f"{what} XT[:, :act_off] (in-chain gather: must be untouched)")


def _untouched(got, before, what):
    off = got["act_off"]
    _same(got["XA"], before["XA"], f"{what} XA (set not written by this sequence)")
    _same(got["XP"][:, :off], before["XP"][:, :off], f"{what} XP (set not written by this sequence)")
    _same(got["XT"][:, :off], before["XT"][:, :off], f"{what} XT (set not written by this sequence)")
    _same(got["R"], before["R"], f"{what} R (set not written by this sequence)")


def _run_sequence(agent, side, n, run=None, distinct=True):
    """One sequence of n updates, then every set the form defines against the oracle.  Returns [(update, set, index draw)] of the
    minibatches that were observed."""
    engine = agent.engine()["engine"]
    ahead, first_in_global = engine != "layers", engine != "slab8"     # k_gather_fused writes x_next out, s8_gather does not
    before = [agent.debug_inputs(0), agent.debug_inputs(1)]
    (run or agent._update_network)(n)
    mbs = [_oracle_minibatch(side, before[0]) for _ in range(n)]
    if distinct:
        for a, b in zip(mbs, mbs[1:]):
            assert not np.array_equal(a[0]["XA"], b[0]["XA"])
    sets = [agent.debug_inputs(0), agent.debug_inputs(1)]
    assert all(sets[s][k] == before[s][k] for s in (0, 1) for k in ("B", "Mp", "ldx", "act_off", "act_dim", "xdim"))
    seen = []
    holds = {(n - 1) & 1: n - 1} if ahead else {0: n - 1}
    if ahead and n >= 2:
        holds[(n - 2) & 1] = n - 2
    for s in (0, 1):
        what = f"{engine} n={n} set {s}"
        if s in holds:
            u = holds[s]
            _check_set(sets[s], mbs[u][0], before[s], f"{what} (update {u})", x_next=u > 0 or first_in_global)
            seen.append((u, s, mbs[u][1]))
        else:
            _untouched(sets[s], before[s], what)
    return seen


def _finish(agent, side, clips=True):
    assert state_equal(side.rng, *side.rs.get_state()[1:3])       # the launches consumed exactly the oracle's words
    if clips:
        assert side.clipped_obs and side.clipped_range              # both clips acted on what was compared


# ----------------------------------------------------------------------------------------------------------- launch forms
@pytest.mark.parametrize("launch", ["default", "split", "slab8_rows8", "slab8_rows16", "slab32", "dw64", "layers"])
def test_every_launch_form_gathers_the_oracles_minibatch(launch, monkeypatch):
    """27/3/4, batch 256, max_action 0.7, clip_obs 0.8, clip_range 1.5: sequences of 1 (in-chain gather into set 0), 2 (gather
    ahead into set 1) and 3 updates (gather ahead back into set 0, over the first update's rows) on one agent; the default table
    also runs the shortest sequence that takes the split form by itself."""
    set_launch(launch, monkeypatch)
    agent, side = _make(256, HP_ENV, 64, make_episodes(64, seed=3, mode="walk"))
    expect_engine(agent, launch, {"slab32": "slab32", "layers": "layers"}.get(launch, "slab8"))
    fresh = agent.debug_inputs(1)
    assert not fresh["XA"].any() and not fresh["R"].any() and (fresh["Mp"], fresh["ldx"], fresh["act_off"]) == (256, 48, 32)
    for n in (1, 2, 3):
        _run_sequence(agent, side, n)
    if launch == "default":
        k = agent.update_kernels(SPLIT_MIN_UPDATES)
        assert k["prologue"] and all(u[0].startswith("k_fb_split8") for u in k["updates"]), k
        assert agent.update_kernels(SPLIT_MIN_UPDATES - 1)["updates"][0][0] == "k_fb_slab8"
        _run_sequence(agent, side, SPLIT_MIN_UPDATES)
    _finish(agent, side)


# --------------------------------------------------------------------------------------------------------- ragged batches
@pytest.mark.parametrize("batch,want", [(7, ("slab8", 4, "gemm_lds 32x32")), (449, ("slab8", 4, "gemm_lds 32x32")),
                                        (513, ("slab8", 8, "gemm_lds 32x32")), (1281, ("slab8", 16, "gemm_lds 32x32")),
                                        (2080, ("slab32", 32, "dw64 split 3"))])
def test_ragged_batches_gather_every_live_row_and_leave_the_padding_zero(batch, want, monkeypatch):
    """The default table at batches that are no multiple of the slab: a last slab with fewer live rows than it has, a last group
    of s8_gather_ahead's per = ceil(B / ng) rows that is short and no multiple of its 4 rows in flight (ng = 4 beside the
    chains: per 2, 113, 129, 321; ng = 64 in k_dw64_adam at 2080: per 33).  Rows B .. Mp - 1 of XA, of the gathered columns of XP and
    XT and of R are +0 after every sequence (the expected arrays hold +0 there)."""
    set_launch("default", monkeypatch)
    agent, side = _make(batch, HP_ENV, 64, make_episodes(64, seed=3, mode="walk"))
    e = agent.engine()
    assert (e["engine"], e["slab_rows"], e["weight_grad"]) == want, e
    for n in (1, 2, 3):
        for u, s, _ in _run_sequence(agent, side, n):
            got = agent.debug_inputs(s)
            off = got["act_off"]
            assert got["Mp"] == -(-batch // 32) * 32        # (2080 has no padded row: it is ragged for dw64's 64-row slices)
            for key, cols in (("XA", got["ldx"]), ("XP", off), ("XT", off)):
                assert not _u32(got[key][batch:, :cols]).any(), (batch, n, s, key)
            assert not _u32(got["R"][batch:]).any(), (batch, n, s)
    _finish(agent, side)


# ----------------------------------------------------------------------------------------------------------------- shapes
# (obs, goal, action, engine of the default table)
SHAPES = [(20, 1, 3, "slab8"),       # one goal component: the c == 0 branch is the whole squared distance
          (29, 3, 1, "slab8"),       # xdim 32 = act_off: no zero gap, one action
          (13, 3, 4, "slab8"),       # xdim 16: act_off 16, ldx 32
          (14, 3, 4, "slab8"),       # xdim 17: act_off moves to 32, ldx 48
          (29, 3, 4, "slab8"),       # xdim 32, ldx 48: the slab engines' column limit
          (60, 3, 7, "layers")]      # falls to the layers engine
SHAPE_CASES = [(s, "default") for s in SHAPES] + [(s, launch) for s in SHAPES if s[3] == "slab8" for launch in ("split", "slab32")]


@pytest.mark.parametrize("shape,launch", SHAPE_CASES, ids=[f"{o}_{g}_{a}_{launch}" for (o, g, a, _), launch in SHAPE_CASES])
def test_other_env_shapes_gather_the_oracles_minibatch(shape, launch, monkeypatch):
    """GoalEnv shapes at which a lane's role in the gathers changes (statistics hoisted per lane, the action block's offset,
    the reward's operand lanes), batch 136 (no multiple of 32: 24 padded rows; per = 34), 24 episodes of 50 steps."""
    od, gd, ad, engine = shape
    set_launch(launch, monkeypatch)
    env = _env(od, gd, ad, 50)
    agent, side = _make(136, env, 24, make_shape_episodes(24, od, gd, ad, 50, seed=3))
    expect_engine(agent, launch, "slab32" if launch == "slab32" else engine)
    d = agent.debug_inputs(0)
    assert (d["xdim"], d["act_off"], d["Mp"]) == (od + gd, -(-(od + gd) // 16) * 16, 160)
    seen_r = set()
    for n in (1, 2, 3):
        for u, s, _ in _run_sequence(agent, side, n):
            seen_r |= set(_u32(agent.debug_inputs(s)["R"][:136]).tolist())
    assert seen_r == {0x80000000, 0xBF800000}, seen_r            # both reward values occurred
    _finish(agent, side)


def test_one_step_episodes_and_a_single_stored_episode():
    """T = 1 and one episode in the buffer, as the sampler's fuzz has it: every row is transition (0, 0), relabelled or not."""
    env = _env(27, 3, 4, 1)
    eps = make_shape_episodes(1, 27, 3, 4, 1, seed=5)
    agent, side = _make(40, env, 1, eps)
    assert agent.engine()["engine"] == "slab8"
    for n in (1, 2, 3):
        for u, s, idx in _run_sequence(agent, side, n, distinct=False):
            assert not idx["e"].any() and not idx["t"].any() and idx["her"].any() and not idx["her"].all()
    _finish(agent, side, clips=False)


# ------------------------------------------------------------------------------------------- rewards on the success radius
@pytest.mark.parametrize("launch", ["default", "split", "slab32", "layers"])
@pytest.mark.parametrize("pairs", ["golden_gd3", "radius_gd1", "radius_gd5"])
def test_reward_bits_on_the_success_radius_through_the_in_launch_gathers(pairs, launch, monkeypatch):
    """The pairs within a few ulps of the 0.05 radius (tests/golden/reward_adversarial.npz, gd 3; threshold_pairs for gd 1 and
    5) as one-step episodes, future_p = 0: every R[m] an update launch leaves must be r_bits[e_m], e_m from the oracle's draw,
    for the gather of a sequence's first update AND for the gather ahead (sequences of 2 updates: set 0 = s8_gather /
    k_gather_fused, set 1 = s8_gather_ahead; layers: sequences of 1, k_gather_fused only).  Each of the two must meet at least
    99 % of the stored pairs: ceil(5.5 M / B) sequences give an expected 99.6 % (checked on the CPU for these seeds)."""
    set_launch(launch, monkeypatch)
    if pairs == "golden_gd3":
        gold = load_golden("reward_adversarial.npz")
        ag, g, r_bits, od, ad = gold["ag"], gold["g"], gold["r_bits"], 27, 4
        assert ag.shape == (4096, 3)
    else:
        gd = int(pairs[-1])
        (ag, g, r_bits), od, ad = threshold_pairs(gd), 12, 3
    M, gd = ag.shape
    batch = 256 if launch == "split" else 1024
    agent, side = _make(batch, _env(od, gd, ad, 1), M, pairs_as_one_step_episodes(ag, g, od, ad), replay_k=0,
                        prime=(0.1, 0.35, 0.15, 0.1))
    assert side.fp == 0.0
    expect_engine(agent, launch, {"slab32": "slab32", "layers": "layers"}.get(launch, "slab8"))
    n = 1 if launch == "layers" else 2
    met = np.zeros((n, M), bool)
    for _ in range(-(-11 * M // (2 * batch))):
        seen = _run_sequence(agent, side, n, distinct=gd > 1)      # (gd 1: every goal is 0, the input rows are all alike; R is not)
        assert sorted(u for u, _, _ in seen) == list(range(n))
        for u, s, idx in seen:
            assert not idx["her"].any()
            got = agent.debug_inputs(s)["R"]
            assert np.array_equal(_u32(got[:batch]), r_bits[idx["e"]]), (pairs, launch, u, s)
            met[u, idx["e"]] = True
    cover = met.mean(axis=1)
    print(f"radius pairs {pairs} through {launch}: M {M}, batch {batch}, coverage per gather {cover.tolist()}")
    assert (cover >= 0.99).all(), cover
    _finish(agent, side, clips=False)


# ------------------------------------------------------------------------------------------------------------- the cycle
@pytest.mark.parametrize("mode", ["eager_calls", "cycle_graph"])
def test_a_cycles_updates_gather_the_oracles_minibatches(mode, monkeypatch):
    """A small FULL buffer, 2 fresh episodes and 3 batches per cycle, 5 cycles: the fresh episodes overwrite random slots first,
    then the normalizers move, then the updates gather.  cycle_graph: hp_agent_train_cycle, whose opening launch (k_cycle_open)
    scatters, updates the normalizers and draws the first plans, as a cached hipGraph that later cycles replay -- the sets are
    what a replayed graph leaves.  eager_calls: the same cycle call by call on plain launches (RLARM_UPDATE_GRAPH=0), plans from
    k_draw_plan.  The oracle side is that of test_updates_track_oracle_over_a_cycle."""
    set_launch("default", monkeypatch)
    graph = mode == "cycle_graph"
    monkeypatch.setenv("RLARM_UPDATE_GRAPH", "1" if graph else "0")
    agent, side = _make(256, HP_ENV, 16, make_episodes(16, seed=9, mode="walk"), seed=11)
    assert agent.buffer.current_size == 16 == side.st.size
    for c in range(5):
        new = make_episodes(2, seed=100 + c, mode="walk")

        def cycle(n):
            side.st.store_episode(new, side.rs)
            if graph:
                agent.train_cycle(new, n_batches=n)
            else:
                agent.buffer.store_episode(new)
                agent._update_normalizer(new)
                agent._update_network(n)
                agent._soft_update_target_network()
            update_normalizers(side.on, side.gn, new, side.fp, side.rs, clip_obs=side.args.clip_obs)
            _norms_equal(agent, side)

        seen = _run_sequence(agent, side, 3, run=cycle)
        assert sorted((u, s) for u, s, _ in seen) == [(1, 1), (2, 0)]
        assert np.array_equal(bits(agent.buffer.buffers["obs"][:16]), bits(side.st.buffers["obs"]))
    mode_now = C.c_int32()
    _lib.check(agent.lib.hp_agent_cycle_mode(agent.h, C.byref(mode_now)))
    assert mode_now.value == (1 if graph else 0)
    _finish(agent, side)
