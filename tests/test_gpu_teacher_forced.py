"""Teacher-forced parity: EVERY update is held to the north-star bar, not just the first of a chain.

A chained comparison lets two correct float32 trajectories separate (Adam divides by sqrt(v) ~ |g|), so beyond the first
update it can only be an envelope.  Here the device is restarted from the oracle's exact state before every update --
online parameters, target networks, Adam exp_avg / exp_avg_sq and step count (hp_agent_set_adam) -- then runs ONE sampled
update (her.py:13-41 draw + gather on the device, ddpg_agent.py:250-277, torch.optim.Adam step t) and is compared with the
oracle's update from the same state on the bit-identical minibatch, for 40 consecutive steps (Adam bias corrections of
steps 1..40, polyak in between):

    both losses     1e-5 relative                                   (BASELINE.json north_star)
    gradients       1e-4 * max|g| absolute per network against the oracle, AND against the float64 gradient of the same
                    state: device error <= 2 x the error of torch's own float32 gradient (+ 1e-6 max|g|) -- two float32
                    gradients are each ~1e-5 max|g| from the exact one after a few steps, so their mutual distance says
                    little; the distance to float64 says who is right
    optimizer step  torch.optim.Adam ITSELF, loaded with the oracle's pre-step state and fed the DEVICE's gradient, must
                    land within 1 float32 ulp of the parameter + 5e-10 (= 5e-7 of lr: torch's CPU kernels fuse some
                    multiply-adds the device keeps apart) of the device's post-step parameters: pins m / v / bias-correction arithmetic of every step t, in every
                    optimizer kernel (GEMM epilogue, k_adam_frag4, dw64 epilogue, k_peer_adam, k_peer_adam2)
    parameters      5e-6 absolute against the ORACLE's post-step parameters on the well-conditioned elements
                    (|g| >= 1% of max|g|), median 1e-7 over all elements

A step that FAILS the gradient bar while a hidden unit's pre-activation on the differentiated path is below float32
summation noise (|z| < 2e-7 in float64: ReLU' may take either value in a correct float32 implementation -- observed at step
2 of batch 256: z = 5e-9, the device's gradient then differs by 5e-5 max|g| from torch's while both losses agree to 1e-7)
is held to the loss and optimizer checks and a 2e-3 max|g| gradient bound; at most 3 of the 80 (step, network) pairs (12 at batch
4096: 16x the pre-activations) may use that excuse.

Why not 5e-6 on every element against the oracle: from step 2 on Adam's step is lr * m_hat / (sqrt(v_hat) + eps) with m, v
mixing this gradient into the history; for an element whose gradient is at rounding level (|g| ~ 1e-9: sums that cancel)
two correct float32 gradients differ by a large FRACTION of themselves, and the step moves by percents of lr = 1e-3
(observed 4e-5 at step 2, batch 256).  Gradient-within-tolerance + optimizer-exact-given-the-gradient is the statement
that holds for every element; it is what the three checks above assert together.

Batch sizes of BASELINE configs 2 / 5 / 3-4 / 4096 with their default engines, and the data-parallel optimizer kernels
in a 1-rank group."""
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gpu_common import ENV_PARAMS, DeviceEpisodeBuffer, fresh_rng, make_shape_episodes, state_equal
from oracle import ddpg_update as oupd
from oracle.her_replay import EpisodeStore, future_probability
from oracle.running_norm import RunningNorm, preproc_og, update_normalizers
from rl_arm_under_sparse_reward_amd import _lib
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import (NET_ACTOR, NET_ACTOR_TARGET, NET_CRITIC, NET_CRITIC_TARGET,
                                                        ddpg_agent)
from rl_arm_under_sparse_reward_amd.synthetic import make_episodes
from update_common import HP, HP_ENV, expect_engine, set_launch

pytestmark = pytest.mark.gpu
LOSS_RTOL = 1e-5
PARAM_ATOL = 5e-6
RELU_NOISE = 2e-7       # |pre-activation| below which two float32 sums of ~300 O(0.1) terms can disagree on the sign
ADAM_ULPS = 1.0         # in units of (1 ulp of the parameter + 5e-10), see below
N_STEPS = 40


def _adam_flat(optim, params):
    """torch.optim.Adam state of the oracle in the flat order of utils.py:18-27 (zeros and step 0 before the first step)."""
    m, v, step = [], [], 0
    for p in params.values():
        st = optim.state.get(p, {})
        m.append(st["exp_avg"] if st else torch.zeros_like(p))
        v.append(st["exp_avg_sq"] if st else torch.zeros_like(p))
        step = int(st["step"]) if st else 0
    return oupd.flatten(m), oupd.flatten(v), step


class _AdamTwin:
    """torch.optim.Adam carrying a copy of the oracle optimizer's state: step_with(flat_grad) applies ONE step of the real
    third-party optimizer to that gradient and returns the flat parameters."""

    def __init__(self, params, optim, lr):
        self.params = [p.detach().clone().requires_grad_(True) for p in params.values()]
        self.opt = torch.optim.Adam(self.params, lr=lr)
        for mine, theirs in zip(self.params, params.values()):
            st = optim.state.get(theirs, {})
            if st:
                self.opt.state[mine] = {"step": st["step"].clone(), "exp_avg": st["exp_avg"].clone(),
                                        "exp_avg_sq": st["exp_avg_sq"].clone()}

    def step_with(self, flat_grad):
        off = 0
        for p in self.params:
            n = p.numel()
            p.grad = torch.from_numpy(np.ascontiguousarray(flat_grad[off:off + n])).reshape(p.shape).clone()
            off += n
        self.opt.step()
        return oupd.flatten(self.params)


def _f64_gradients(actor, critic, actor_t, critic_t, x, x_next, actions, r, max_action=0.5, gamma=0.98, action_l2=1.0):
    """ddpg_agent.py:250-277 in float64 from the same float32 state and minibatch: the yardstick that says how far a CORRECT
    float32 gradient (torch's) is from the exact one, element by element."""
    A = {k: v.detach().double().requires_grad_(True) for k, v in actor.items()}
    Cn = {k: v.detach().double().requires_grad_(True) for k, v in critic.items()}
    AT = {k: v.detach().double() for k, v in actor_t.items()}
    CT = {k: v.detach().double() for k, v in critic_t.items()}
    x, x_next, actions, r = x.double(), x_next.double(), actions.double(), r.double()
    with torch.no_grad():
        q_next = oupd.critic_forward(CT, x_next, oupd.actor_forward(AT, x_next, max_action), max_action)
        target_q = torch.clamp(r + gamma * q_next, -1 / (1 - gamma), 0)
    critic_loss = (target_q - oupd.critic_forward(Cn, x, actions, max_action)).pow(2).mean()
    a_real = oupd.actor_forward(A, x, max_action)
    actor_loss = -oupd.critic_forward(Cn, x, a_real, max_action).mean() + action_l2 * (a_real / max_action).pow(2).mean()
    ga = torch.autograd.grad(actor_loss, list(A.values()))
    gc = torch.autograd.grad(critic_loss, list(Cn.values()))
    flat = lambda ts: np.concatenate([t.detach().numpy().ravel() for t in ts])     # noqa: E731

    # smallest |pre-activation| on each loss's differentiated path: ReLU' jumps at 0, so a hidden unit whose pre-activation
    # is below float32 summation noise takes EITHER mask in a correct float32 implementation (and its whole row's
    # gradient contribution moves by percents): such a step cannot be held to a rounding-level gradient bound
    def min_preact(p, keys, h):
        lo = float("inf")
        for k in keys:
            z = torch.nn.functional.linear(h, p[k + ".weight"], p[k + ".bias"])
            lo = min(lo, float(z.abs().min()))
            h = torch.relu(z)
        return lo

    with torch.no_grad():
        xa = torch.cat([x, a_real / max_action], dim=1)
        lo_actor = min(min_preact(A, ("fc1", "fc2", "fc3"), x), min_preact(Cn, ("fc1", "fc2", "fc3"), xa))
        lo_critic = min_preact(Cn, ("fc1", "fc2", "fc3"), torch.cat([x, actions / max_action], dim=1))
    return {"actor": flat(ga), "critic": flat(gc), "min_preact": {"actor": lo_actor, "critic": lo_critic}}


def _teach(agent, learner):
    """device state := oracle state (parameters, targets, optimizer moments, step count)."""
    agent._set_flat(NET_ACTOR, learner.flat("actor"))
    agent._set_flat(NET_CRITIC, learner.flat("critic"))
    agent._set_flat(NET_ACTOR_TARGET, learner.flat("actor_target"))
    agent._set_flat(NET_CRITIC_TARGET, learner.flat("critic_target"))
    ma, va, sa = _adam_flat(learner.actor_optim, learner.actor)
    mc, vc, sc = _adam_flat(learner.critic_optim, learner.critic)
    assert sa == sc
    agent.set_adam_state(NET_ACTOR, ma, va, sa)
    agent.set_adam_state(NET_CRITIC, mc, vc, sc)
    return sa


def _run(batch, k, comm=None, n_steps=N_STEPS, n_eps=64, env_params=None, hp=None, before_step=None, on_minibatch=None,
         polyak_every=10, spare_eps=0, torch_seed=0):
    """`n_steps` teacher-forced updates.  env_params: the GoalEnv shape and action_max (bmirobot's 27/3/4 and 0.5 when None;
    other shapes get gpu_common.make_shape_episodes); hp: Args overrides of the learner's hyperparameters, given to the
    device agent, the oracle learner, the normalizers, the Adam twins and the float64 yardstick alike.  before_step(i, side)
    may change the oracle's state before it is taught to the device; on_minibatch(i, side, mb) sees each step's minibatch
    before the oracle's update; spare_eps: room in the replay buffer for that many more episodes; torch_seed: of the initial
    weights.  Returns the worst
    numbers, the agent and `side`: the oracle's learner, store, normalizers and RNG, the episodes and the settings."""
    torch.set_num_threads(4)
    ep = dict(env_params or ENV_PARAMS)
    hp = dict(hp or {})
    args = Args(batch_size=batch, buffer_size=(n_eps + spare_eps) * ep["max_timesteps"], replay_k=k, **hp)
    od, gd, ad, T = ep["obs"], ep["goal"], ep["action"], ep["max_timesteps"]
    if env_params is None:
        eps = make_episodes(n_eps, seed=3, mode="walk")
    else:
        eps = make_shape_episodes(n_eps, od, gd, ad, T, seed=3)
    torch.manual_seed(torch_seed)
    rng = fresh_rng(7)
    agent = ddpg_agent(args, None, ep, comm=comm, rng=rng)
    a0 = {kk: v.detach().clone() for kk, v in agent.actor_network.state_dict().items()}
    c0 = {kk: v.detach().clone() for kk, v in agent.critic_network.state_dict().items()}
    amax = float(ep["action_max"])
    learner = oupd.DDPGLearner(a0, c0, max_action=amax, gamma=args.gamma, action_l2=args.action_l2,
                               lr_actor=args.lr_actor, lr_critic=args.lr_critic, polyak=args.polyak)
    lrs = {"actor": args.lr_actor, "critic": args.lr_critic}
    rs = np.random.RandomState(7)
    st = EpisodeStore(T, od, gd, ad, (n_eps + spare_eps) * T)
    fp = future_probability("future", k)
    on, gn = RunningNorm(od, default_clip_range=args.clip_range), RunningNorm(gd, default_clip_range=args.clip_range)
    st.store_episode(eps, rs)
    agent.buffer.store_episode(eps)
    two = [a[-2:] for a in eps]
    scratch = DeviceEpisodeBuffer(2, T, od, gd, ad)
    scratch.store(rng, two)
    _lib.check(agent.lib.hp_norm_update_from_staged(scratch.h, rng.h, agent.o_norm.h, agent.g_norm.h, fp, float(args.clip_obs)))
    agent.o_norm.recompute_stats(); agent.g_norm.recompute_stats()
    update_normalizers(on, gn, two, fp, rs, clip_obs=args.clip_obs)
    side = SimpleNamespace(learner=learner, st=st, rs=rs, on=on, gn=gn, fp=fp, rng=rng, args=args, env_params=ep, lrs=lrs,
                           eps=eps, batch=batch)
    worst_loss, worst_param, worst_grad, worst_adam, worst_vs64, n_ambiguous = 0.0, 0.0, 0.0, 0.0, 0.0, 0
    for i in range(n_steps):
        if before_step is not None:
            before_step(i, side)
        step = _teach(agent, learner)
        assert step == i
        m_dev, v_dev, s_dev = agent.get_adam_state(NET_CRITIC)       # the hook round-trips (pack/unpack is lossless)
        assert s_dev == i and np.array_equal(m_dev, _adam_flat(learner.critic_optim, learner.critic)[0])
        twins = {"actor": _AdamTwin(learner.actor, learner.actor_optim, lrs["actor"]),
                 "critic": _AdamTwin(learner.critic, learner.critic_optim, lrs["critic"])}     # oracle state BEFORE the step
        agent._update_network(1)
        got = agent.last_losses(1)[0]
        tr, _ = st.sample(batch, fp, rs)
        mb = oupd.minibatch_tensors(tr, on, gn, clip_obs=args.clip_obs)
        if on_minibatch is not None:
            on_minibatch(i, side, mb)
        g64 = _f64_gradients(learner.actor, learner.critic, learner.actor_target, learner.critic_target, *mb,
                             max_action=amax, gamma=args.gamma, action_l2=args.action_l2)
        res = learner.update(*mb)
        for j, name in enumerate(("actor_loss", "critic_loss")):
            rel = abs(float(got[j]) - res[name]) / max(abs(res[name]), 1e-3)
            worst_loss = max(worst_loss, rel)
            assert rel <= LOSS_RTOL, (i, name, got[j], res[name], rel)
        for slot, name in ((NET_ACTOR, "actor"), (NET_CRITIC, "critic")):
            g_ref = res[f"{name}_grads"].astype(np.float64)
            g_dev = agent.get_flat_grads(slot)
            gmax = float(np.abs(g_ref).max())
            gerr = float(np.max(np.abs(g_dev - g_ref)))
            # ... and both against the float64 gradient of the same state: the device may not be further from the exact
            # gradient than 2x what torch's own float32 arithmetic is (+ 1e-6 max|g| of slack for the luck of one draw)
            dev64, ref64 = float(np.max(np.abs(g_dev - g64[name]))), float(np.max(np.abs(g_ref - g64[name])))
            strict = gerr <= 1e-4 * gmax and dev64 <= 2.0 * ref64 + 1e-6 * gmax
            # a ReLU mask may legitimately differ (see _f64_gradients) -- but only a step that HAS a pre-activation inside
            # float32 summation noise may use that excuse, and only when the strict bar actually failed
            ambiguous = (not strict) and g64["min_preact"][name] < RELU_NOISE
            n_ambiguous += int(ambiguous)
            if not ambiguous:
                worst_grad = max(worst_grad, gerr / gmax)
                worst_vs64 = max(worst_vs64, dev64 / max(ref64, 1e-30))
                assert gerr <= 1e-4 * gmax, (i, name, "grad vs oracle", gerr, gmax)
                assert dev64 <= 2.0 * ref64 + 1e-6 * gmax, (i, name, "grad vs float64", dev64, ref64, gmax)
            else:       # one row's contribution through one unit: a few percent of 1/B of the gradient
                assert gerr <= 2e-3 * gmax, (i, name, "grad vs oracle (ReLU tie)", gerr, gmax, g64["min_preact"][name])
            p_dev32 = agent._get_flat(slot)
            p_twin32 = twins[name].step_with(g_dev)                          # torch.optim.Adam on the device's gradient
            p_dev = p_dev32.astype(np.float64)
            # allowed: one ulp of the parameter (final rounding of p + step) + 5e-7 of the step size lr (the step itself is
            # ~6 float32 operations, and torch's CPU kernels fuse some multiply-adds the device keeps apart): 5e-10
            allowed = np.spacing(np.abs(p_twin32)).astype(np.float64) + 5e-7 * lrs[name]
            ulps = np.abs(p_dev - p_twin32.astype(np.float64)) / allowed
            aerr = float(ulps.max())
            worst_adam = max(worst_adam, aerr)
            assert aerr <= ADAM_ULPS, (i, name, "adam", aerr)
            p_ref = learner.flat(name).astype(np.float64)
            well = np.abs(g_ref) >= 1e-2 * gmax
            err = float(np.max(np.abs(p_dev - p_ref)[well]))
            if not ambiguous:
                worst_param = max(worst_param, err)
                assert err <= PARAM_ATOL, (i, name, "param", err, int(well.sum()))
            assert float(np.median(np.abs(p_dev - p_ref))) <= 1e-7, (i, name)
        assert agent.get_adam_state(NET_ACTOR)[2] == i + 1
        if i % polyak_every == polyak_every - 1:   # ddpg_agent.py:149-150 every so often: targets != online nets later on
            agent._soft_update_target_network(); learner.soft_update()
            tgt = agent._get_flat(NET_CRITIC_TARGET).astype(np.float64)
            assert float(np.max(np.abs(tgt - learner.flat("critic_target")))) <= PARAM_ATOL
    assert state_equal(rng, *rs.get_state()[1:3])              # the sampler consumed exactly the oracle's words
    # of 2 x 40 (step, network) pairs: ties that flip a mask are rare events, not an excuse -- their number grows with the
    # number of pre-activations per update, i.e. with the batch (observed: 1 at batch 256, 9 at 4096)
    assert n_ambiguous <= 3 * max(1, batch // 1024), n_ambiguous
    return (worst_loss, worst_grad, worst_adam, worst_param, worst_vs64, n_ambiguous), agent, side


@pytest.mark.parametrize("batch,k", [(256, 4), (512, 8), (1024, 4), (4096, 4)],
                         ids=["config2_b256", "config5_b512_k8", "config3_4_b1024", "b4096"])
def test_every_update_meets_the_north_star_bar_single_rank(batch, k, monkeypatch):
    monkeypatch.setenv("RLARM_KEEP_GRADS", "1")      # the optimizer epilogues also write the gradient out (read by hp_agent_create)
    worst, agent, _ = _run(batch, k)
    print(f"teacher-forced batch {batch} k {k} engine {agent.engine()}: worst over 40 steps: loss rel {worst[0]:.2e}, "
          f"grad / max|g| {worst[1]:.2e} (error vs float64 = {worst[4]:.2f} x torch float32's), optimizer vs torch.optim.Adam {worst[2]:.2f} x (1 ulp + 5e-10), well-conditioned param {worst[3]:.2e}, ReLU ties {worst[5]}")


@pytest.mark.parametrize("batch,k,n_eps", [(256, 4, 64), (256, 4, 5000), (64, 4, 64), (320, 8, 64)],
                         ids=["b256", "b256_full_shard", "b64", "b320_k8"])
def test_every_update_meets_the_bar_through_the_split_launch(batch, k, n_eps, monkeypatch):
    """Round 4: the same bars through slab8_split.h (RLARM_SPLIT=1 forces it for single updates too): target chains in a
    prologue launch, critic chains + the critic's weight-gradient tiles and optimizer step inside the chain launch behind the
    two in-launch counters, the actor's tiles behind it -- on the 64-episode buffer and on the full 5000-episode shard."""
    monkeypatch.setenv("RLARM_KEEP_GRADS", "1")
    monkeypatch.setenv("RLARM_SPLIT", "1")
    worst, agent, _ = _run(batch, k, n_eps=n_eps, n_steps=N_STEPS if n_eps <= 64 else 20)
    print(f"teacher-forced (split launch) batch {batch} k {k} episodes {n_eps}: worst: loss rel {worst[0]:.2e}, grad / max|g| {worst[1]:.2e} "
          f"(vs float64 = {worst[4]:.2f} x torch float32's), optimizer {worst[2]:.2f} x (1 ulp + 5e-10), param {worst[3]:.2e}, ReLU ties {worst[5]}")


@pytest.mark.parametrize("batch,k", [(256, 4), (512, 8)], ids=["config2_b256", "config5_b512_k8"])
def test_every_update_meets_the_bar_on_the_full_shard(batch, k, monkeypatch):
    """the teacher-forced bars on the BASELINE shard (5000 episodes, 149 MB of float64 rows), default engines."""
    monkeypatch.setenv("RLARM_KEEP_GRADS", "1")
    worst, agent, _ = _run(batch, k, n_eps=5000, n_steps=20)
    print(f"teacher-forced full shard batch {batch} k {k} engine {agent.engine()}: worst over 20 steps: loss rel {worst[0]:.2e}, "
          f"grad / max|g| {worst[1]:.2e}, optimizer {worst[2]:.2f} x (1 ulp + 5e-10), param {worst[3]:.2e}, ReLU ties {worst[5]}")


@pytest.mark.parametrize("transport", ["peer", "peer+notiles", "peer+2phase", "native", "torch",
                                       "peer+split", "peer+notiles+split", "peer+2phase+split", "native+split"])
def test_every_update_meets_the_bar_through_the_data_parallel_optimizer(transport, monkeypatch):
    """1-rank group, forced exchange: backward -> exchange -> separate optimizer kernel (k_peer_adam; k_peer_reduce_slice +
    k_peer_adam2; RCCL + k_adam_frag4; torch.distributed + hp_agent_apply), the kernels every rank of a multi-GPU job runs --
    and, round 4, "peer" = weight gradients + tile-wise exchange + optimizer step in ONE launch (k_gemm_lds_adam_peer).
    Round 6, +split: the same transports through the split launch, which data-parallel ranks now take as well -- "peer": the
    critic's in-launch tiles exchange tile-wise and step inside k_fb_split8<1>, the actor's in k_gemm_lds_adam_peer behind it;
    every other transport: k_fb_split8<2> (gradients only) + k_gemm_lds, then the exchange and the optimizer kernel."""
    import torch.distributed as dist
    from rl_arm_under_sparse_reward_amd.utils import Communicator
    split = transport.endswith("+split")
    if split:
        transport = transport[:-6]
        monkeypatch.setenv("RLARM_SPLIT", "1")         # single updates too (the teacher-forced loop issues them one at a time)
    if transport.endswith("+2phase"):
        transport = transport[:-7]
        monkeypatch.setenv("RLARM_PEER_PHASES", "2")
    if transport.endswith("+notiles"):               # "peer" alone: the tile-wise exchange inside the weight-gradient launch (round 4)
        transport = transport[:-8]
        monkeypatch.setenv("RLARM_PEER_TILES", "0")
    monkeypatch.setenv("RLARM_COMM", transport)
    monkeypatch.setenv("RLARM_KEEP_GRADS", "1")      # the peer optimizer kernels write the exchanged sum out for get_grads
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    comm = None
    try:
        comm = Communicator(0, force=True)
        worst, agent, _ = _run(256, 4, comm=comm)
        assert (agent._peer is not None) == (transport == "peer")
        assert (agent._native_comm is not None) == (transport == "native")
        kernels = agent.update_kernels(1)["updates"][0]
        print(f"data-parallel optimizer path {transport}{' +split' if split else ''}: kernels of one update {kernels}")
        if split:
            tiles_in_launch = os.environ.get("RLARM_PEER_TILES") != "0" and os.environ.get("RLARM_PEER_PHASES") != "2"
            assert kernels[0] == ("k_fb_split8<1>" if transport == "peer" and tiles_in_launch else "k_fb_split8<2>"), kernels
        else:
            assert kernels[0] == "k_fb_slab8", kernels
        _lib.Context.default().synchronize()
        torch.cuda.synchronize()
        agent.close_comm()
        del agent
    finally:
        if comm is not None:
            comm.close()
        _lib.Context.default().set_stream(None)
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------------------------
# The same bars away from the reference's defaults (update_common.HP, HP_ENV), through the launch structures of
# update_common.LAUNCH.
CASE_STEPS = 12              # polyak every 4 steps: later steps see targets that differ from the online nets


def _report(tag, worst, agent, n_steps, extra=""):
    e = agent.engine()
    print(f"teacher-forced {tag} engine {e['engine']} rows {e['slab_rows']} {e['weight_grad']}: worst over {n_steps} steps: "
          f"loss rel {worst[0]:.2e}, grad / max|g| {worst[1]:.2e} (error vs float64 = {worst[4]:.2f} x torch float32's), "
          f"optimizer vs torch.optim.Adam {worst[2]:.2f} x (1 ulp + 5e-7 lr), well-conditioned param {worst[3]:.2e}, "
          f"ReLU ties {worst[5]}{extra}")


@pytest.mark.parametrize("launch", ["default", "split", "slab8_rows8", "slab8_rows16", "slab32", "dw64", "adam_unfused",
                                    "layers"])
def test_every_update_meets_the_bar_at_other_hyperparameters(launch, monkeypatch):
    """Case A: HP at 27/3/4, batch 256, through every launch structure of the update."""
    set_launch(launch, monkeypatch)
    worst, agent, _ = _run(256, 4, n_steps=CASE_STEPS, hp=HP, env_params=HP_ENV, polyak_every=4)
    expect_engine(agent, launch, {"slab32": "slab32", "layers": "layers"}.get(launch, "slab8"))
    _report(f"hparams {launch} batch 256", worst, agent, CASE_STEPS)


@pytest.mark.parametrize("batch,k,want", [(7, 4, ("slab8", 4, "gemm_lds 32x32")), (449, 4, ("slab8", 4, "gemm_lds 32x32")),
                                          (513, 8, ("slab8", 8, "gemm_lds 32x32")), (1281, 4, ("slab8", 16, "gemm_lds 32x32")),
                                          (2080, 4, ("slab32", 32, "dw64 split 3"))])
def test_every_update_meets_the_bar_at_other_hyperparameters_ragged(batch, k, want, monkeypatch):
    """Case A, ragged batches on the default table: padding rows, 1/B, the dw64 slices of a batch that is no multiple of 64."""
    set_launch("default", monkeypatch)
    worst, agent, _ = _run(batch, k, n_steps=CASE_STEPS, hp=HP, env_params=HP_ENV, polyak_every=4)
    e = agent.engine()
    assert (e["engine"], e["slab_rows"], e["weight_grad"]) == want, e
    _report(f"hparams default batch {batch} k {k}", worst, agent, CASE_STEPS)


def _target_q_probe(side):
    """The next states of every stored transition, clipped and normalised like a minibatch (float32)."""
    if not hasattr(side, "x_next_probe"):
        obs, _, g, _ = side.eps
        o, gg = preproc_og(obs[:, 1:, :].reshape(-1, obs.shape[-1]), g.reshape(-1, g.shape[-1]), side.args.clip_obs)
        side.x_next_probe = torch.tensor(np.concatenate([side.on.normalize(o), side.gn.normalize(gg)], axis=1), dtype=torch.float32)
    return side.x_next_probe


def _spread_target_q(i, side, lo=-4.5, hi=4.5):
    """Before every step: rescale and shift the oracle critic target's head (q_out) so that Q' of the stored next states
    runs from `lo` at its 10th to `hi` at its 90th percentile.  With gamma = 0.5 (clip_return 2) and r in {-1, 0},
    r + gamma Q' then falls below -2 on some rows and above 0 on others: both sides of the clamp of ddpg_agent.py:259-260."""
    L, amax = side.learner, side.env_params["action_max"]
    x = _target_q_probe(side)
    with torch.no_grad():
        q = oupd.critic_forward(L.critic_target, x, oupd.actor_forward(L.actor_target, x, amax), amax).double().numpy()
        q10, q90 = np.percentile(q, [10, 90])
        scale = (hi - lo) / (q90 - q10)
        L.critic_target["q_out.weight"].mul_(float(scale))
        L.critic_target["q_out.bias"].mul_(float(scale)).add_(float(lo - scale * q10))


def _clamp_branches(i, side, mb):
    """float64 target of the taught state on this minibatch: the fraction of rows clamped at -clip_return and at 0."""
    L, amax, gamma = side.learner, side.env_params["action_max"], side.args.gamma
    AT = {kk: v.detach().double() for kk, v in L.actor_target.items()}
    CT = {kk: v.detach().double() for kk, v in L.critic_target.items()}
    _, xn, _, r = (t.double() for t in mb)
    with torch.no_grad():
        y = (r + gamma * oupd.critic_forward(CT, xn, oupd.actor_forward(AT, xn, amax), amax)).numpy()
    lo, hi = float(np.mean(y < -1 / (1 - gamma))), float(np.mean(y > 0))
    assert lo >= 0.05 and hi >= 0.05, (i, lo, hi)
    side.branch_min = min(getattr(side, "branch_min", (1.0, 1.0))[0], lo), min(getattr(side, "branch_min", (1.0, 1.0))[1], hi)


@pytest.mark.parametrize("launch", ["default", "split", "slab32", "layers"])
def test_every_update_meets_the_bar_on_both_clamp_branches(launch, monkeypatch):
    """Case B: gamma 0.5 puts clip_return at 2; the target critic's head is spread so that every minibatch has rows clamped
    at -2 AND rows clamped at 0 (>= 5% each, asserted in float64 on the taught state, so the case cannot pass vacuously)."""
    set_launch(launch, monkeypatch)
    hp = dict(HP, gamma=0.5)
    worst, agent, side = _run(256, 4, n_steps=CASE_STEPS, hp=hp, env_params=HP_ENV, polyak_every=4,
                              before_step=_spread_target_q, on_minibatch=_clamp_branches)
    expect_engine(agent, launch, {"slab32": "slab32", "layers": "layers"}.get(launch, "slab8"))
    _report(f"clamp branches {launch}", worst, agent, CASE_STEPS,
            f", rows clamped at -clip_return >= {side.branch_min[0]:.2f}, at 0 >= {side.branch_min[1]:.2f}")


# (obs, goal, action, action_max, default engine): the slab engines' eligibility edges and the first shapes beyond them
SHAPES = [(13, 3, 4, 0.7, "slab8"),      # xdim 16: the action at column 16, ldx 32
          (29, 3, 4, 0.5, "slab8"),      # xdim 32: K1 of the actor full, the action right after x, no zero gap
          (29, 3, 1, 2.0, "slab8"),      # one action
          (20, 1, 3, 0.7, "slab8"),      # one-wide goal, three actions
          (30, 3, 4, 0.7, "layers"),     # xdim 33: the first shape of the layer engine
          (25, 2, 5, 1.3, "layers"),     # five actions
          (60, 3, 7, 0.5, "layers")]
SHAPE_CASES = [(s, "default") for s in SHAPES] + [(s, launch) for s in SHAPES if s[4] == "slab8" for launch in ("split", "slab32")]


@pytest.mark.parametrize("shape,launch", SHAPE_CASES, ids=[f"{o}_{g}_{a}_{launch}" for (o, g, a, _, _), launch in SHAPE_CASES])
def test_every_update_meets_the_bar_at_other_env_shapes(shape, launch, monkeypatch):
    """Case C: GoalEnv shapes other than 27/3/4, default hyperparameters, 24 episodes of 50 steps."""
    o, g, a, amax, engine = shape
    set_launch(launch, monkeypatch)
    env = {"obs": o, "goal": g, "action": a, "action_max": amax, "max_timesteps": 50}
    worst, agent, _ = _run(256, 4, n_steps=CASE_STEPS, n_eps=24, env_params=env, polyak_every=4)
    expect_engine(agent, launch, "slab32" if launch == "slab32" else engine)
    _report(f"shape {o}/{g}/{a} action_max {amax} {launch}", worst, agent, CASE_STEPS)


# Case E: hidden widths other than 256 and network inputs wider than 256 columns -- what hp_agent_create accepts (any multiple of
# 32) and only the layer-per-launch engine runs.  WIDE: the widest input the rest of the learner accepts -- 256 observation columns
# is the normalizers' limit (NORM_MAX), 7 goal columns the HER sampler's (her.py refuses goal_dim >= 8: the device sums the squared
# goal distance in index order, numpy pairwise from 8 elements on; a 250 / 10 / 4 shape is therefore refused).  xdim 263: the actor's
# first layer reduces over 272 columns and the critic's over 288, a full 256-column chunk of the staged reduction (gemm_lds.h,
# gemm_tile) and a remainder chunk of 16 / 32; the critic's first-layer dX and dW have 9 column tiles.
WIDE_ENV = {"obs": 256, "goal": 7, "action": 4, "action_max": 0.7, "max_timesteps": 20}
# (hidden, batch, env, episodes, torch seed of the initial weights): what each case reaches -- and, last, its number of (step,
# network) pairs, of 2 x 12, whose smallest float64 pre-activation lies below RELU_NOISE, counted on the CPU with the oracle alone
# (relu_tie_upper_bound below): an upper bound on what the cap of 3 ReLU ties can ever be asked to excuse.  The wider the layers,
# the more pre-activations per update and the more often one of them is that small: with _run's seed 0 the count is 4 at
# hidden 128, 6 at 512, 6 and 4 for the wide input at 256 and 288: these four take the first seed with the smallest count among
# 0 .. 23 (128: 0 at seed 1; 512: 1 at seed 4; 256 wide: 0 at seed 12; 288 wide: 2 at seed 3).
WIDTH_CASES = {
    # one 32-wide column tile per problem; reductions of 32 (kc 32: 2 of 8 waves have products); the heads' dX reduces over 16
    "h32": (32, 256, HP_ENV, 64, 0),                # ties <= 0
    # no multiple of 64; 6 super-steps for 8 waves; three column tiles
    "h96": (96, 256, HP_ENV, 64, 0),                # ties <= 0
    # the width the refusal tests of the fused entry points name
    "h128": (128, 256, HP_ENV, 64, 1),              # ties <= 0
    # the first width whose staged reduction takes a second chunk: 256 + 32, the barrier in between and a remainder chunk
    "h288": (288, 256, HP_ENV, 64, 0),              # ties <= 3
    # two full chunks, 16 column tiles, arena and launch order twice as large
    "h512": (512, 256, HP_ENV, 64, 4),              # ties <= 1
    # Mp 32: weight gradients on the staged k-major x k-major path with K 32 and padded rows
    "h96_b7": (96, 7, HP_ENV, 64, 0),               # ties <= 0
    # weight gradients on the ring path, 1/B no power of two, a partial last block of batch rows
    "h96_b449": (96, 449, HP_ENV, 64, 0),           # ties <= 1
    # the first layer's forward reduction takes a remainder chunk; 9 column tiles in the critic's first-layer dX and dW
    "h256_wide": (256, 256, WIDE_ENV, 24, 12),      # ties <= 0
    # both reductions loop
    "h288_wide": (288, 256, WIDE_ENV, 24, 3),       # ties <= 2
}


def relu_tie_upper_bound(case, n_steps=CASE_STEPS, polyak_every=4, torch_seed=None):
    """The oracle's half of _run for a WIDTH_CASES entry, on the CPU (no device is touched: the networks are the host containers
    ddpg_agent would build from the same torch seed): how many (step, network) pairs have a float64 pre-activation below
    RELU_NOISE.  Not a test; `python -c "import test_gpu_teacher_forced as t; print(t.relu_tie_upper_bound('h512'))"` from tests/."""
    from rl_arm_under_sparse_reward_amd.models import actor, critic
    hidden, batch, env, n_eps, seed = WIDTH_CASES[case]
    ep, args = dict(env, hidden=hidden), Args(batch_size=batch, replay_k=4, **HP)
    od, gd, ad, T = ep["obs"], ep["goal"], ep["action"], ep["max_timesteps"]
    eps = make_shape_episodes(n_eps, od, gd, ad, T, seed=3)
    torch.manual_seed(seed if torch_seed is None else torch_seed)
    a0, c0 = actor(ep).state_dict(), critic(ep).state_dict()
    amax = float(ep["action_max"])
    learner = oupd.DDPGLearner(a0, c0, max_action=amax, gamma=args.gamma, action_l2=args.action_l2, lr_actor=args.lr_actor,
                               lr_critic=args.lr_critic, polyak=args.polyak)
    rs, st, fp = np.random.RandomState(7), EpisodeStore(T, od, gd, ad, n_eps * T), future_probability("future", 4)
    on, gn = RunningNorm(od, default_clip_range=args.clip_range), RunningNorm(gd, default_clip_range=args.clip_range)
    st.store_episode(eps, rs)
    update_normalizers(on, gn, [a[-2:] for a in eps], fp, rs, clip_obs=args.clip_obs)
    count = 0
    for i in range(n_steps):
        mb = oupd.minibatch_tensors(st.sample(batch, fp, rs)[0], on, gn, clip_obs=args.clip_obs)
        lo = _f64_gradients(learner.actor, learner.critic, learner.actor_target, learner.critic_target, *mb, max_action=amax,
                            gamma=args.gamma, action_l2=args.action_l2)["min_preact"]
        count += int(lo["actor"] < RELU_NOISE) + int(lo["critic"] < RELU_NOISE)
        learner.update(*mb)
        if i % polyak_every == polyak_every - 1:
            learner.soft_update()
    return count


@pytest.mark.parametrize("case", list(WIDTH_CASES))
def test_every_update_meets_the_bar_at_other_hidden_widths(case, monkeypatch):
    """Case E: HP at hidden widths 32 .. 512 and with a 263-column input, on the layer-per-launch engine, which is what
    hp_agent_create gives every such shape; the bars of the file, unchanged.  The wide input is 256 / 7 / 4, not 250 / 10 / 4:
    the HER sampler refuses goals of 8 or more components (her.py: bit-exact rewards are only claimed below numpy's pairwise
    summation), so the goal has 7 and the observation the normalizers' 256; the padded widths are the same 272 and 288."""
    hidden, batch, env, n_eps, seed = WIDTH_CASES[case]
    set_launch("default", monkeypatch)
    worst, agent, _ = _run(batch, 4, n_steps=CASE_STEPS, n_eps=n_eps, hp=HP, env_params=dict(env, hidden=hidden), polyak_every=4,
                           torch_seed=seed)
    expect_engine(agent, "default", "layers")
    assert agent.actor_network.fc2.weight.shape == (hidden, hidden) and agent.critic_network.fc1.weight.shape[0] == hidden
    _report(f"width {case} hidden {hidden} batch {batch} input {env['obs']}/{env['goal']}/{env['action']}", worst, agent, CASE_STEPS)


def _load_learner(learner, agent):
    """oracle state := device state (parameters, targets, Adam moments and step count), the inverse of _teach."""
    for slot, which in ((NET_ACTOR, "actor"), (NET_CRITIC, "critic"), (NET_ACTOR_TARGET, "actor_target"),
                        (NET_CRITIC_TARGET, "critic_target")):
        flat, off = agent._get_flat(slot), 0
        for t in getattr(learner, which).values():
            with torch.no_grad():
                t.copy_(torch.from_numpy(flat[off:off + t.numel()].reshape(t.shape)))
            off += t.numel()
    for slot, params, optim in ((NET_ACTOR, learner.actor, learner.actor_optim), (NET_CRITIC, learner.critic, learner.critic_optim)):
        m, v, step = agent.get_adam_state(slot)
        off = 0
        for p in params.values():
            n = p.numel()
            st = optim.state[p]
            st["exp_avg"].copy_(torch.from_numpy(m[off:off + n].reshape(p.shape)))
            st["exp_avg_sq"].copy_(torch.from_numpy(v[off:off + n].reshape(p.shape)))
            st["step"].fill_(step)
            off += n


@pytest.mark.parametrize("launch", ["default", "split", "slab32_dw64", "layers"])
def test_polyak_folded_into_the_last_update_at_other_polyak(launch, monkeypatch):
    """Case D: polyak 0.9 folded into the optimizer epilogue of a cycle's last update (slab engines; k_polyak on layers).
    The targets must equal (1-p) p_new + p t_old in float32 BIT FOR BIT (numpy float32: correctly rounded, unfused -- the
    expression of k_polyak_frag), p_new being the device's own post-step parameters; then, with the targets left as the
    cycle wrote them, one more update against the oracle loaded from the device's state meets the loss bar, which it
    cannot if the folded write reached the arena but not the forward-fragment copy the next update's target chains read."""
    set_launch(launch, monkeypatch)
    worst, agent, side = _run(256, 4, n_steps=4, hp=HP, env_params=HP_ENV, polyak_every=4, spare_eps=4)
    expect_engine(agent, launch, "slab32" if launch == "slab32_dw64" else "layers" if launch == "layers" else "slab8")
    learner, p = side.learner, np.float32(side.args.polyak)
    _teach(agent, learner)
    t_old = {s: agent._get_flat(s) for s in (NET_ACTOR_TARGET, NET_CRITIC_TARGET)}
    assert not np.array_equal(t_old[NET_ACTOR_TARGET], agent._get_flat(NET_ACTOR))
    new = make_episodes(4, seed=11, mode="walk")
    side.st.store_episode(new, side.rs)
    agent.train_cycle(new, n_batches=1)                     # store + normalizer + 1 update + polyak, one graph
    update_normalizers(side.on, side.gn, new, side.fp, side.rs, clip_obs=side.args.clip_obs)
    side.st.sample(256, side.fp, side.rs)
    for src, tgt in ((NET_ACTOR, NET_ACTOR_TARGET), (NET_CRITIC, NET_CRITIC_TARGET)):
        want = np.float32(1 - side.args.polyak) * agent._get_flat(src) + p * t_old[tgt]
        got = agent._get_flat(tgt)
        assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
            (launch, tgt, int(np.sum(got != want)), float(np.max(np.abs(got - want))))
    assert np.array_equal(agent.o_norm.mean, side.on.mean) and np.array_equal(agent.g_norm.std, side.gn.std)
    _load_learner(learner, agent)
    agent._update_network(1)
    got = agent.last_losses(1)[0]
    tr, _ = side.st.sample(256, side.fp, side.rs)
    res = learner.update(*oupd.minibatch_tensors(tr, side.on, side.gn, clip_obs=side.args.clip_obs))
    rel = [abs(float(got[j]) - res[nm]) / max(abs(res[nm]), 1e-3) for j, nm in enumerate(("actor_loss", "critic_loss"))]
    assert max(rel) <= LOSS_RTOL, (launch, got, res["actor_loss"], res["critic_loss"])
    assert state_equal(side.rng, *side.rs.get_state()[1:3])
    _report(f"folded polyak 0.9 {launch}", worst, agent, 4, f"; targets bit-exact, next update loss rel {max(rel):.2e}")
