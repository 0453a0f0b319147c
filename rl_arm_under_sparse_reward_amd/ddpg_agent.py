"""ddpg_agent -- the learner half of the reference's ddpg_agent.py on the MI355X.

Same wiring as ddpg_agent.py:18-53 (actor/critic + targets, Adam x2, her_sampler,
replay_buffer, two normalizers, optional demo preload) and the same method names for the
pieces on the hot path:

    _update_network()                 ddpg_agent.py:225-277   one sample + DDPG update
    _soft_update_target_network()     :220-222 (both nets at once, as :149-150 calls it twice)
    _update_normalizer(episode_batch) :187-212
    _preproc_og(o, g)                 :214-217
    _init_demo_buffer()               :82-90
    save_checkpoint()                 :158-161  (same 5-element list, same state_dict keys)

plus `train_cycle(episode_batch)`: lines :143-150 (store -> normalizer -> n_batches updates ->
polyak) as ONE cached hipGraph launch.  `learn()` (:92-161) is the epoch loop around both halves; the rollout half -- policy
calls, exploration, collection from host or device environments, evaluation -- is rollouts.py, the episode audits are
episode_audit.py, and the agent inherits both.

Data never leaves the device between sampling and the optimizer step; the methods that
return numpy (`buffer.sample`, normalizer attributes, `state_dict`) copy out on demand.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import threading
import time
from datetime import datetime

import numpy as np
import torch

from . import _lib
from . import random as _random
from ._lib import NET_ACTOR, NET_ACTOR_TARGET, NET_CRITIC, NET_CRITIC_TARGET      # (callers import them from here)
from .arguments import Args
from .episode_audit import EpisodeAudit
from .her import her_sampler
from .models import actor, critic
from .normalizer import normalizer
from .replay_buffer import replay_buffer
from .rollouts import Rollouts
from .utils import Communicator


class ddpg_agent(Rollouts, EpisodeAudit):
    def __init__(self, args, env, env_params, comm: Communicator | None = None, ctx=None, rng=None):
        self.savetime = 0
        self.args = args
        # one environment, or a list of them: the rollout / evaluation loops step a list in lockstep with one batched
        # policy call per timestep (the host feeder of SURVEY 8f N1)
        self.envs = list(env) if isinstance(env, (list, tuple)) else [env]
        self.env = self.envs[0]
        # a vectorised simulator in device memory (device_env.py): rollouts, evaluation and learn() take the device path
        self.vec_env = env if getattr(env, "is_device_vec_env", False) else None
        self._rollouts = {}              # DeviceEpisodes blocks by episode count
        self.explore_streams = None      # random.DeviceRandomStreams: one exploration stream per environment (enable_explore_streams)
        self.rollout_form = None         # 'fused' | 'stepped': how the most recent wave of collect_episodes_device was collected
        self.rollout_launches = None     # rollout launches of the most recent collect_episodes_device call (fused form)
        self.rollout_reason = None       # ... and, when stepped, why (device_env.fused_rollout_reason)
        self._slab8 = None               # whether policy calls are the one-launch slab kernel (_slab_shaped asks once)
        self._demo_preload_pending = False     # demo_source='device' with args.device_reset: the preload waits for learn()
        self.demo_stats = None           # demo_source='device': {'kept', 'attempted', 'launches'} of the generated demonstrations
        self.resumed_at = None           # (epoch, cycle) of the training state most recently loaded
        self._state_saves = 0            # saves of _save_epoch_state since the base was last rewritten
        self.env_params = env_params
        self.ctx = ctx or _lib.Context.default()
        self.lib = self.ctx.lib
        self.comm = comm or Communicator(self.ctx.device_id)
        if rng is None:
            # the reference draws from the process-global np.random, which train.py:36 seeds with seed + rank before it
            # builds the agent.  The device twin of that stream is seeded the same way unless the launch script already
            # did it (random.seed / random.set_state), so ranks never share a sampler stream by accident
            rng = _random.global_state()
            if not rng.seeded:
                rng.seed(int(args.seed) + self.comm.rank)
        self.rng = rng
        # networks: host containers initialised like the reference (consumes the torch RNG identically)
        self.actor_network = actor(env_params)
        self.critic_network = critic(env_params)
        self.actor_target_network = actor(env_params)       # re-initialised from the online nets below
        self.critic_target_network = critic(env_params)
        cfg = _lib.AgentCfg(
            obs_dim=env_params['obs'], goal_dim=env_params['goal'], act_dim=env_params['action'],
            hidden=int(env_params.get('hidden', 256)),
            batch=int(args.batch_size), grad_world_size=self.comm.world_size,
            max_action=float(env_params['action_max']), gamma=float(args.gamma), action_l2=float(args.action_l2),
            lr_actor=float(args.lr_actor), lr_critic=float(args.lr_critic), polyak=float(args.polyak),
            clip_obs=float(args.clip_obs), clip_range=float(args.clip_range),
            adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8)
        self.h = C.c_void_p()
        _lib.check(self.lib.hp_agent_create(self.ctx.h, C.byref(cfg), C.byref(self.h)))
        for slot, net in ((NET_ACTOR, self.actor_network), (NET_CRITIC, self.critic_network),
                          (NET_ACTOR_TARGET, self.actor_target_network),
                          (NET_CRITIC_TARGET, self.critic_target_network)):
            net.attach(self, slot)
        self.actor_network.push()
        self.critic_network.push()
        # data-parallel ranks on GPUs: the library exchanges gradients and normalizer sums itself, inside the cycle graph.
        # First choice: one-shot all-reduce over peer memory fused with the optimizer (csrc/peer.hip); else RCCL
        # (csrc/comm.hip); else torch.distributed from a host-driven loop.
        self._native_comm = None
        self._peer = None
        if self.comm.active:
            n = C.c_int64()
            p = C.c_void_p()
            _lib.check(self.lib.hp_agent_grad_buffer(self.h, C.byref(p), C.byref(n)))
            self._peer = self.comm.attach_peer(self.ctx, n.value)
            if self._peer is not None:
                # e.g. the layer-per-launch engine cannot use it.  The ranks decide TOGETHER, and an exchange nobody uses is
                # destroyed (not merely forgotten): `comm.peer` must not outlive it, or the fallback below would take the
                # peer start-up path while its gradients go through another transport
                ok = self.lib.hp_agent_set_peer(self.h, self._peer) == 0
                if not self.comm.agree(ok, self.ctx):
                    _lib.check(self.lib.hp_agent_set_peer(self.h, None))
                    self.comm.drop_peer()
                    self._peer = None
        if self._peer is None:
            self._native_comm = self.comm.attach_native(self.ctx)
            if self._native_comm is not None:
                _lib.check(self.lib.hp_agent_set_comm(self.h, self._native_comm))
        if self._arg("grad_reduce") not in ("sum", "mean"):
            raise ValueError("grad_reduce must be 'sum' (reference semantics) or 'mean'")
        self._grad_mean = self._arg("grad_reduce") == "mean"
        _lib.check(self.lib.hp_agent_set_grad_reduce(self.h, int(self._grad_mean)))
        self._broadcast_params(self.comm)                       # sync_networks x2 (ddpg_agent.py:27-28)
        _lib.check(self.lib.hp_agent_sync_targets(self.h))      # targets := online (ddpg_agent.py:33-34)
        # her sampler + replay buffer (ddpg_agent.py:45-47)
        reward_func = getattr(self.env, "compute_reward", None)
        owner = getattr(reward_func, "__self__", None)      # an environment that states its own threshold / reward type keeps it
        self.her_module = her_sampler(args.replay_strategy, args.replay_k, reward_func,
                                      distance_threshold=None if hasattr(owner, "distance_threshold") else self._arg("distance_threshold"),
                                      reward_type=None if hasattr(owner, "reward_type") else self._arg("reward_type"),
                                      rng=self.rng, goal_dim=env_params['goal'])
        self.buffer = replay_buffer(self.env_params, self.args.buffer_size, self.her_module.sample_her_transitions,
                                    rng=self.rng, ctx=self.ctx)
        if self._arg("add_demo"):
            self._init_demo_buffer()
        # normalizers (ddpg_agent.py:52-53)
        self.o_norm = normalizer(size=env_params['obs'], default_clip_range=self.args.clip_range, ctx=self.ctx,
                                 comm=self.comm)
        self.g_norm = normalizer(size=env_params['goal'], default_clip_range=self.args.clip_range, ctx=self.ctx,
                                 comm=self.comm)
        self._norm_stage = None          # staging buffer of _update_normalizer(episode_batch)
        self._pending_updates = 0              # argument-less _update_network() calls not issued yet (_lib.py: deferred updates)
        self._pending_parked = False           # their last flush failed: not retried until the caller asks (see _flush_updates)
        self._pending_site = "?"               # where the first of them was called: named if their flush fails
        self._defer_updates = os.environ.get("RLARM_DEFER_UPDATES", "1") != "0"
        self._stage_lock = threading.RLock()   # orders "store a wave, then sample ITS staged episodes" across feeder threads
        self.success_rates = []
        self.eval_metrics = []           # args.eval_metrics: one dict per evaluation, keyed by synthetic.EPISODE_SUMMARY
        self.eval_critic = []            # args.eval_critic: one dict per evaluation, keyed by synthetic.CRITIC_STATS
        self.policy_audit = []           # args.audit_policy: one dict per epoch, keyed by synthetic.POLICY_STATS
        self._policy_audit_pending = None
        self.actor_signal_audit = []     # args.audit_actor_signal: one dict per epoch, keyed by synthetic.SIGNAL_STATS
        self._actor_signal_pending = None
        self.bellman_audit = []          # args.audit_bellman: one dict per epoch, keyed by synthetic.BELLMAN_STATS
        self._bellman_pending = None
        self.model_path = os.path.join(self.args.save_dir, self.args.env_name)

    def _arg(self, name):
        """An optional argument: the caller's `args` value where it has one (the reference's Args lacks the newer fields), else the
        default `arguments.Args` states for that field, else None (`state_path`, `resume`: fields Args does not have)."""
        if hasattr(self.args, name):
            return getattr(self.args, name)
        field = Args.__dataclass_fields__.get(name)
        return field.default if field is not None else None

    @property
    def _library_exchanges(self):
        """Whether update sequences and cycles are the library's own launches: a single rank, or ranks whose gradients the library
        exchanges itself (RCCL or peer memory attached).  False: collectives go through torch.distributed from a host-driven loop."""
        return not self.comm.active or self._native_comm is not None or self._peer is not None

    def close_comm(self):
        """Detach and destroy the library-side RCCL communicator (call on every rank before
        torch.distributed.destroy_process_group / interpreter exit)."""
        self._flush_updates()         # deferred updates still exchange gradients: issue them while the transport exists
        if self._native_comm is not None or self._peer is not None or self.comm.peer is not None or self.comm.native is not None:
            self.ctx.synchronize()
            _lib.check(self.lib.hp_agent_set_comm(self.h, None))
            _lib.check(self.lib.hp_agent_set_peer(self.h, None))
            self._native_comm = None
            self._peer = None
            self.comm.close()

    def check_exchange(self):
        """Raise if the peer-memory exchange died (a rank late by more than RLARM_PEER_TIMEOUT_S, or gone): the optimizer
        steps from that update on were skipped, so the replicas are no longer in step.  train_cycle / _update_network raise
        the same at their next call without synchronising; learn() asks at every epoch boundary."""
        if self._peer is not None:
            err = C.c_uint32()
            _lib.check(self.lib.hp_peer_status(self._peer, C.byref(err)))
            if err.value:
                raise RuntimeError("peer-memory exchange timed out: a rank was late by more than RLARM_PEER_TIMEOUT_S or is "
                                   "gone; updates were skipped on this rank and the replicas are no longer in step")

    # ------------------------------------------------------------------ parameter plumbing
    def _count(self, slot):
        return int(self.lib.hp_agent_param_count(self.h, slot))

    def _get_flat(self, slot):
        out = np.empty(self._count(slot), np.float32)
        _lib.check(self.lib.hp_agent_get_params(self.h, slot, _lib.ptr(out, C.c_float), out.size))
        return out

    def _set_flat(self, slot, flat):
        flat = _lib.as_f32(flat)
        _lib.check(self.lib.hp_agent_set_params(self.h, slot, _lib.ptr(flat, C.c_float), flat.size))

    def get_flat_grads(self, slot):
        out = np.empty(self._count(slot), np.float32)
        _lib.check(self.lib.hp_agent_get_grads(self.h, slot, _lib.ptr(out, C.c_float), out.size))
        return out

    def get_adam_state(self, slot):
        n = self._count(slot)
        m, v, step = np.empty(n, np.float32), np.empty(n, np.float32), C.c_int64()
        _lib.check(self.lib.hp_agent_get_adam(self.h, slot, _lib.ptr(m, C.c_float), _lib.ptr(v, C.c_float), n,
                                              C.byref(step)))
        return m, v, step.value

    def set_adam_state(self, slot, m, v, step):
        """Load optimizer state (test hook, hp_agent_set_adam): torch.optim.Adam's exp_avg / exp_avg_sq in the flat order of
        utils.py:18-27 and the number of steps already taken (both optimizers step together)."""
        m, v = _lib.as_f32(m), _lib.as_f32(v)
        _lib.check(self.lib.hp_agent_set_adam(self.h, slot, _lib.ptr(m, C.c_float), _lib.ptr(v, C.c_float), m.size,
                                              int(step)))

    def debug_inputs(self, which=0):
        """The network inputs an update launch gathered for itself (test hook, hp_agent_debug_inputs; synchronises): input set
        `which` of the gather-ahead ping-pong as {'XA', 'XP', 'XT': float32 [Mp, ldx], 'R': float32 [Mp], 'B', 'Mp', 'ldx',
        'act_off', 'act_dim', 'xdim'}, padded rows and columns included."""
        dims = (C.c_int32 * 6)()
        _lib.check(self.lib.hp_agent_debug_inputs(self.h, int(which), None, None, None, None, dims))
        out = dict(zip(("B", "Mp", "ldx", "act_off", "act_dim", "xdim"), (int(d) for d in dims)))
        for key in ("XA", "XP", "XT"):
            out[key] = np.empty((out["Mp"], out["ldx"]), np.float32)
        out["R"] = np.empty(out["Mp"], np.float32)
        f = C.c_float
        _lib.check(self.lib.hp_agent_debug_inputs(self.h, int(which), _lib.ptr(out["XA"], f), _lib.ptr(out["XP"], f),
                                                  _lib.ptr(out["XT"], f), _lib.ptr(out["R"], f), dims))
        return out

    def _broadcast_params(self, comm):
        if not comm.active:
            return
        p, n = C.c_void_p(), C.c_int64()
        _lib.check(self.lib.hp_agent_param_buffer(self.h, C.byref(p), C.byref(n)))
        if comm.native is None and self._peer is not None and comm.peer is not None:
            # the library exchanges gradients itself over peer memory: only this one-off broadcast goes through
            # torch.distributed; the library keeps its own (capturable) stream, so order the two sides with full
            # synchronisations instead of moving the library onto torch's stream
            self.ctx.synchronize()
            comm.broadcast_device(p.value, n.value, 0)
            torch.cuda.synchronize(self.ctx.device_id)
            return
        if comm.native is None:
            # every exchange of this run goes through torch.distributed (host-driven loop): the library's kernels must be
            # stream-ordered with the collectives torch enqueues
            self.ctx.use_torch_stream()
        comm.broadcast_device(p.value, n.value, 0)

    def _allreduce_grads(self, comm):
        if not comm.active:
            return
        p, n = C.c_void_p(), C.c_int64()
        _lib.check(self.lib.hp_agent_grad_buffer(self.h, C.byref(p), C.byref(n)))
        if self._grad_mean:
            comm.allreduce_mean_device(p.value, n.value)
        else:
            comm.allreduce_sum_device(p.value, n.value)                  # utils.py:47

    def _actor_forward(self, slot, x):
        x = _lib.as_f32(x)
        x2 = x.reshape(-1, x.shape[-1])
        out = np.empty((x2.shape[0], self.env_params['action']), np.float32)
        _lib.check(self.lib.hp_agent_actor_forward(self.h, slot, _lib.ptr(x2, C.c_float), x2.shape[0],
                                                   _lib.ptr(out, C.c_float)))
        return out.reshape(x.shape[:-1] + (out.shape[-1],))

    def _critic_forward(self, slot, x, actions):
        x, actions = _lib.as_f32(x), _lib.as_f32(actions)
        x2, a2 = x.reshape(-1, x.shape[-1]), actions.reshape(-1, actions.shape[-1])
        if x2.shape[0] != a2.shape[0]:
            raise ValueError("critic forward: inputs and actions differ in length")
        out = np.empty((x2.shape[0], 1), np.float32)
        _lib.check(self.lib.hp_agent_critic_forward(self.h, slot, _lib.ptr(x2, C.c_float), _lib.ptr(a2, C.c_float),
                                                    x2.shape[0], _lib.ptr(out, C.c_float)))
        return out.reshape(x.shape[:-1] + (1,))

    # ------------------------------------------------------------------ hot path
    def _handles(self):
        return (self.h, self.buffer._dev.h, self.o_norm.h, self.g_norm.h, self.rng.h)

    def _update_network(self, n_updates=None):
        """ddpg_agent.py:225-277.  `_update_network(n)`: n updates back to back, issued now.  `_update_network()` -- the
        reference's call form, once per minibatch in its inner loop (:145-147) -- is only counted and issued together with the
        calls that follow it, as soon as anything else touches the library or `n_batches` of them have come (_lib.py,
        "deferred updates"): the same updates bit for bit, 40.5 instead of 51 us each at batch 256."""
        if n_updates is None:
            if self._defer_updates and self._library_exchanges:
                with _lib.pending_lock:
                    if self._pending_updates == 0:      # where the first of these deferred calls was made: named if their flush fails
                        f = sys._getframe(1)
                        self._pending_site = f"{f.f_code.co_filename}:{f.f_lineno}"
                    self._pending_updates += 1
                    self._pending_parked = False            # a new update call is the natural point to try the owed ones again
                    if self._pending_updates >= int(self.args.n_batches):
                        self._flush_updates()
                    else:
                        _lib.register_pending(self)
                return
            n_updates = 1
        with _lib.pending_lock:
            # owed updates that a failed flush parked come FIRST, like in the reference's sequential loop: an explicit call is a
            # point to try them again, exactly as the argument-less form above does (if they fail again this call raises and
            # issues nothing of its own)
            self._pending_parked = False
        self._flush_updates()
        self._issue_updates(int(n_updates))

    def _flush_updates(self):
        """Issue the counted `_update_network()` calls.  In chunks whose lengths are powers of two (at most n_batches): a loop
        that is flushed at irregular points would otherwise ask for a new sequence length -- a freshly captured graph -- every
        time and thrash the library's 8-entry graph cache.

        A failing flush raises ONCE, like the reference's `_update_network()` does at the same cause (e.g. `ValueError: high <=
        0` on an empty buffer, ddpg_agent.py:227): the error names the deferred call it belongs to, what could not be issued
        stays owed (`pending_updates`) but is PARKED -- no later library call retries it by itself, so every object stays usable
        and the caller can remove the cause (e.g. store an episode).  The owed updates are tried again by the next
        `_update_network()` / `_update_network(n)` call (in front of that call's own updates: the order of updates never
        changes), by `retry_pending_updates()`, or dropped by `discard_pending_updates()`.  Every OTHER caller of this method
        (train_cycle, weight reads, close_comm) leaves parked updates parked."""
        with _lib.pending_lock:
            if self._pending_parked:
                return
            n, self._pending_updates = self._pending_updates, 0
            _lib.unregister_pending(self)
            cap = max(1, int(self.args.n_batches))
            while n:
                chunk = n if n == cap else 1 << (min(n, cap).bit_length() - 1)
                try:
                    self._issue_updates(chunk)
                except Exception as e:
                    self._pending_updates += n                 # nothing of this chunk was enqueued: still owed ...
                    self._pending_parked = True                # ... but not retried behind the caller's back
                    note = (f"deferred _update_network() x {n}, first called at {self._pending_site} "
                            "(issued by a later library call, _lib.py 'deferred updates')")
                    if hasattr(e, "add_note"):
                        e.add_note(note)
                        raise
                    raise type(e)(f"{e} [{note}]") from e
                n -= chunk

    @property
    def pending_updates(self):
        """Argument-less `_update_network()` calls counted but not issued yet (parked ones included)."""
        return self._pending_updates

    def retry_pending_updates(self):
        """Issue the owed updates now (after a failed flush parked them and its cause has been removed).  Raises like the
        flush did if they fail again."""
        with _lib.pending_lock:
            self._pending_parked = False
            self._flush_updates()

    def discard_pending_updates(self):
        """Give up on the owed updates (what a caller that catches the reference's error and moves on does); returns how many."""
        with _lib.pending_lock:
            n, self._pending_updates, self._pending_parked = self._pending_updates, 0, False
            _lib.unregister_pending(self)
            return n

    def _issue_updates(self, n_updates):
        fp, sq = float(self.her_module.future_p), float(self.her_module.sq_threshold)
        if self._library_exchanges:
            # single rank, or the library exchanges the gradients itself between backward and Adam
            _lib.check(self.lib.hp_agent_sample_and_update(*self._handles(), fp, sq, int(n_updates)))
            return
        for _ in range(int(n_updates)):          # data-parallel ranks: grads are SUMmed between backward and Adam
            _lib.check(self.lib.hp_agent_forward_backward(*self._handles(), fp, sq))
            self._allreduce_grads(self.comm)
            _lib.check(self.lib.hp_agent_apply(self.h))

    def update_on_minibatch(self, x, x_next, actions, r):
        """One update on a caller-supplied normalised minibatch (parity hook); returns (actor_loss, critic_loss)."""
        x, xn, a = _lib.as_f32(x), _lib.as_f32(x_next), _lib.as_f32(actions)
        r = _lib.as_f32(r).reshape(-1)
        B = int(self.args.batch_size)
        if x.shape[0] != B or xn.shape != x.shape or a.shape[0] != B or r.shape[0] != B:
            raise ValueError("minibatch shapes do not match args.batch_size")
        losses = np.empty(2, np.float32)
        f = C.c_float
        _lib.check(self.lib.hp_agent_update_minibatch(self.h, _lib.ptr(x, f), _lib.ptr(xn, f), _lib.ptr(a, f),
                                                      _lib.ptr(r, f), _lib.ptr(losses, f)))
        return float(losses[0]), float(losses[1])

    def last_losses(self, n=1):
        """(actor_loss, critic_loss) of the n most recent updates, oldest first.  Synchronises."""
        out = np.empty(2 * n, np.float32)
        _lib.check(self.lib.hp_agent_get_losses(self.h, _lib.ptr(out, C.c_float), n))
        return out.reshape(n, 2)

    def _soft_update_target_network(self, target=None, source=None):
        """ddpg_agent.py:220-222.  The reference calls it once per net (:149-150); the device pass covers
        both nets, so it acts when called for the actor pair (or with no arguments) and is a no-op for the
        critic pair."""
        if target is None or target is self.actor_target_network:
            _lib.check(self.lib.hp_agent_soft_update(self.h))

    def _preproc_og(self, o, g):
        o = np.clip(o, -self.args.clip_obs, self.args.clip_obs)
        g = np.clip(g, -self.args.clip_obs, self.args.clip_obs)
        return o, g

    def _update_normalizer(self, episode_batch=None):
        """ddpg_agent.py:187-212: HER-sample T transitions out of `episode_batch`, clip, update both normalizers,
        recompute.  The given episodes are uploaded into a private staging buffer (the reference's `buffer_temp`), so
        the statistics come from exactly these episodes whatever was stored in between (e.g. by a feeder thread).
        `episode_batch=None` reuses the episodes the replay buffer staged in its most recent store_episode (no upload;
        the benchmark's cycle boundary) and raises if nothing was ever stored."""
        fp = float(self.her_module.future_p)
        if episode_batch is not None:
            if self._norm_stage is None:
                from .replay_buffer import DeviceEpisodeBuffer
                ep = self.env_params
                self._norm_stage = DeviceEpisodeBuffer(1, ep['max_timesteps'], ep['obs'], ep['goal'], ep['action'],
                                                       ctx=self.ctx)
            self._norm_stage.stage(episode_batch)
            src = self._norm_stage
        else:
            src = self.buffer._dev
        _lib.check(self.lib.hp_norm_update_from_staged(src.h, self.rng.h, self.o_norm.h, self.g_norm.h, fp,
                                                       float(self.args.clip_obs)))
        self.o_norm.recompute_stats()
        self.g_norm.recompute_stats()

    def train_cycle(self, episode_batch, n_batches=None):
        """ddpg_agent.py:143-150 as one hipGraph: store_episode, _update_normalizer, n_batches x
        _update_network, soft update of both targets.  Asynchronous.  With data-parallel ranks the graph
        contains the RCCL all-reduces (gradients every update, normalizer sums once) when the library owns the
        communicator; otherwise the loop is driven from the host."""
        n_batches = int(n_batches or self.args.n_batches)
        device_block = hasattr(episode_batch, "block") and hasattr(episode_batch, "numpy")    # device_env.DeviceEpisodes
        if not self._library_exchanges:      # collectives on torch.distributed: host-driven loop
            if device_block:
                with self._stage_lock:       # store + normalizer update on the episodes the store just staged, as one unit
                    self.buffer.store_episode(episode_batch)
                    self._update_normalizer()
            else:
                self.buffer.store_episode(episode_batch)
                self._update_normalizer(episode_batch)
            self._update_network(n_batches)
            self._soft_update_target_network()
            return
        if device_block:
            # the same cycle out of the device block (hp_agent_train_cycle_dev): a device-to-device copy instead of the upload
            _lib.check(self.lib.hp_agent_train_cycle_dev(
                *self._handles(), C.c_void_p(episode_batch.block), len(episode_batch),
                float(self.her_module.future_p), float(self.her_module.sq_threshold), n_batches))
            return
        # same shape validation as store_episode (a wrong T or dimension raises ValueError like numpy's broadcast at
        # replay_buffer.py:39-42 instead of letting the library read past the arrays)
        obs, ag, g, act, n_new = self.buffer._dev._checked(episode_batch)
        d = C.c_double
        _lib.check(self.lib.hp_agent_train_cycle(
            *self._handles(), _lib.ptr(obs, d), _lib.ptr(ag, d), _lib.ptr(g, d), _lib.ptr(act, d), n_new,
            float(self.her_module.future_p), float(self.her_module.sq_threshold), n_batches))

    def train_cycle_from_feeder(self, feeder, slot, n_batches=None):
        """ddpg_agent.py:143-150 on the episodes of a feeder wave: store_episode is an asynchronous DMA out of the feeder's
        registered shared-memory slot (no CPU copy), the normalizer samples the staged episodes, the updates replay their
        cached graph.  Asynchronous; ranks of a data-parallel group call it in step like train_cycle."""
        n_batches = int(n_batches or self.args.n_batches)
        if self._library_exchanges:
            # the whole cycle as one cached graph behind the DMA (hp_agent_train_cycle_pinned): same launches as train_cycle
            with self._stage_lock:
                feeder.train_cycle_wave(slot, n_batches)
            return
        with self._stage_lock:       # store + normalizer update as one unit: another thread's store_wave (e.g. a rollout
            feeder.store_wave(slot)  # thread) must not replace the staged episodes in between
            self._update_normalizer()
        self._update_network(n_batches)
        self._soft_update_target_network()

    def update_kernels(self, n_updates=None):
        """The kernels a sequence of `n_updates` updates enqueues on this agent as it is NOW -- engine, switches, attached
        transport -- read off the library's own launch logic (hp_agent_update_kernels: the logic runs under a discarded stream
        capture, nothing executes).  {'open': [...], 'prologue': [...], 'updates': [[...] per update], 'close': [...]}."""
        self._flush_updates()
        n = int(n_updates or self.args.n_batches)
        buf = C.create_string_buffer(1 << 16)
        _lib.check(self.lib.hp_agent_update_kernels(*self._handles(), float(self.her_module.future_p),
                                                    float(self.her_module.sq_threshold), n, 0 if self._library_exchanges else 1, buf, len(buf)))
        out, cur = {"open": [], "prologue": [], "updates": [], "close": []}, None
        for tok in buf.value.decode().split(","):
            if tok == "#update":
                out["updates"].append([])
                cur = out["updates"][-1]
            elif tok.startswith("#"):
                cur = out[tok[1:]]
            elif tok:
                cur.append(tok)
        return out

    def engine(self):
        """Kernels this agent's updates run (hp_agent_engine): e.g. {'engine': 'slab8', 'slab_rows': 4, 'weight_grad':
        'gemm_lds 32x32'} at the reference batch, {'engine': 'slab32', 'slab_rows': 32, 'weight_grad': 'dw64 split 3'} at 4096.
        `kernels_per_update`: the launches of one steady-state update of an n_batches sequence, by name, as the library
        enqueues them with the transport attached NOW (ask before close_comm)."""
        e, r, d, f = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self.lib.hp_agent_engine(self.h, C.byref(e), C.byref(r), C.byref(d)))
        _lib.check(self.lib.hp_agent_update_form(self.h, int(self.args.n_batches), C.byref(f)))
        out = {"engine": {0: "layers", 8: "slab8", 32: "slab32"}[e.value], "slab_rows": r.value,
               "weight_grad": f"dw64 split {d.value}" if d.value else "gemm_lds 32x32",
               "launches_per_update": {0: "chains | weight gradients (+ Adam, or exchange + Adam)",
                                       1: "split: chains (targets one update ahead) + critic weight gradients (+ exchange + Adam) | "
                                          "actor weight gradients (+ exchange + Adam)"}[f.value]}
        try:
            k = self.update_kernels()
            ups = k["updates"]
            out["kernels_per_update"] = ups[min(2, len(ups) - 1)]
            out["kernels_per_sequence_extra"] = k["open"] + k["prologue"] + k["close"]
        except _lib.HpError as err:      # e.g. the legacy stream cannot be captured: the form above still stands
            out["kernels_per_update"] = None
            out["kernels_error"] = str(err)
        return out

    def policy_snapshot(self):
        """Publish the current actor + normalizer statistics to feeders that call the policy while cycles run
        (hp_agent_act_snapshot): stream-ordered with the updates, no host wait."""
        _lib.check(self.lib.hp_agent_policy_snapshot(self.h, self.o_norm.h, self.g_norm.h))

    # ------------------------------------------------------------------ demos / checkpoints (formats preserved)
    def plot_success_rate(self):
        """ddpg_agent.py:73-80: dump the per-epoch success rates where the reference does; the plot itself needs
        matplotlib and a display, so it is drawn only when both are there."""
        saved_dir = 'test_rates/'
        os.makedirs(saved_dir, exist_ok=True)
        np.save(saved_dir + str(self.args.seed) + '_' + str(self.args.add_demo) + '_success_rates.npy',
                np.array(self.success_rates))
        if self._arg("eval_metrics"):      # [evaluations, 6] in the columns of synthetic.EPISODE_SUMMARY
            from .synthetic import EPISODE_SUMMARY
            np.save(saved_dir + str(self.args.seed) + '_' + str(self.args.add_demo) + '_eval_metrics.npy',
                    np.array([[m[k] for k in EPISODE_SUMMARY] for m in self.eval_metrics], dtype=np.float64).reshape(-1, len(EPISODE_SUMMARY)))
        try:
            import matplotlib.pyplot as plt
        except Exception:
            return
        plt.plot(self.success_rates)
        if os.environ.get("DISPLAY") or os.environ.get("MPLBACKEND"):
            plt.show()

    def _init_demo_buffer(self):
        """ddpg_agent.py:82-90: keys obs, acs, ag, g of a get_demo_data_*.py file (info is ignored).  With
        `args.demo_source == "device"` and a native vectorised environment the demonstrations are generated instead
        (`device_env.generate_demos`: args.demo_episodes successful episodes of the scripted push controller) and stored out of
        their device block, in order, as ONE store_episode call like the file's -- the device path has no size limit of its
        own -- and fewer kept than asked is an error.  If the environment is not reset on the device yet but args.device_reset
        asks for it, the preload waits for learn(), which enables the reset first."""
        arg = lambda name: ddpg_agent._arg(self, name)      # unbound: any object with `args` and `buffer` can be preloaded
        source = arg("demo_source")
        if source not in ("file", "device"):
            raise ValueError("demo_source must be 'file' (the reference's preload) or 'device'")
        if source == "device":
            from .device_env import generate_demos
            if self.vec_env is None or not getattr(self.vec_env, "is_native_device_env", False):
                raise ValueError("demo_source='device' needs a native vectorised device environment (device_env.py)")
            if getattr(self.vec_env, "reset_streams", None) is None and arg("device_reset"):
                self._demo_preload_pending = True
                return
            self._demo_preload_pending = False
            want = int(arg("demo_episodes"))
            demos = generate_demos(self.vec_env, want, max_episodes=int(arg("demo_max_episodes")), ctx=self.ctx)
            self.demo_stats = {"kept": demos.kept, "attempted": demos.attempted, "launches": demos.launches}
            if demos.kept < want:
                raise RuntimeError(f"demo_source='device': only {demos.kept} of {want} scripted episodes succeeded in "
                                   f"{demos.attempted} attempts")
            self.buffer.store_episode(demos.episodes)
            self.ctx.synchronize()           # the block is freed with `demos`: the store has read it
            return
        demo = np.load(self.args.demo_name, allow_pickle=True)
        self.buffer.store_episode([np.array(demo['obs']), np.array(demo['ag']), np.array(demo['g']),
                                   np.array(demo['acs'])])

    def checkpoint_payload(self):
        """The 5-element list the reference saves (ddpg_agent.py:158-161)."""
        return [self.o_norm.mean, self.o_norm.std, self.g_norm.mean, self.g_norm.std,
                self.actor_network.state_dict()]

    def save_checkpoint(self, path=None):
        if path is None:
            os.makedirs(self.model_path, exist_ok=True)
            self.savetime += 1
            path = os.path.join(self.model_path, f"{self.args.seed}_{self.args.add_demo}{self.savetime}_model.pt")
        torch.save(self.checkpoint_payload(), path)
        return path

    def load_checkpoint(self, path):
        """Warm start from a reference-format checkpoint (the block commented out at ddpg_agent.py:54-62)."""
        o_mean, o_std, g_mean, g_std, model = torch.load(path, map_location="cpu", weights_only=False)
        have, mine = int(model["fc2.weight"].shape[0]), int(self.env_params.get("hidden", 256))
        if have != mine:      # before load_state_dict: it copies the tensors that do fit (the head's bias) and then raises
            raise ValueError(f"load_checkpoint: {path} holds an actor with hidden width {have}, this agent's is {mine}")
        self.actor_network.load_state_dict(model)
        self.o_norm.set_stats(o_mean, o_std)
        self.g_norm.set_stats(g_mean, g_std)

    # ------------------------------------------------------------------ training state (train_state.py, csrc/state.hip)
    def save_training_state(self, path, wait=True, extra=None, epoch=0, cycle=0, base=None):
        """Everything a continued run needs -- what ddpg_agent.py:54-62 wished for ("load the data to continue the training") --
        in one .npz of named arrays: both networks and targets, Adam m / v / step, both normalizers, the device random stream,
        the replay buffer, and the host side (numpy's global stream, success_rates, savetime, `epoch` / `cycle` reached, the
        caller's opaque `extra` bytes, e.g. a pickled simulator).  Pending deferred updates are issued first.  The device part
        is snapshotted in stream order without a host wait; wait=False returns a handle whose `.result()` finishes the file
        while training goes on (one capture at a time: a second one before `.result()` raises).
        base=PATH of a full state this agent saved or loaded in this process: write a *delta* -- the small arrays, and the buffer
        as the episodes stored since that state (a few MB instead of the whole buffer; the device knows which slots were
        written).  Base + delta restore exactly what a full state taken now restores.  A base this agent does not know, or one
        older than a load_training_state done since, is refused before anything is captured."""
        from . import train_state
        return train_state.save(self, path, wait=wait, extra=extra, epoch=epoch, cycle=cycle, base=base)

    def load_training_state(self, path, base=None):
        """Continue from `save_training_state`'s file, in a fresh agent or in this one after more cycles (roll-back): the run
        that follows is bit-identical to the one that never stopped.  Refused, with nothing changed, when dims, capacity, T, rank
        or world size differ or the uploaded bytes do not sum on the device to what the file records.  Returns `extra`; the
        epoch / cycle the state was saved at are in `self.resumed_at`.  A delta is composed with its base on the host first
        (`base`, default: the file name the delta records, beside it)."""
        from . import train_state
        extra, manifest = train_state.load(self, path, base=base)
        self.resumed_at = (int(manifest["epoch"]), int(manifest["cycle"]))
        return extra

    def _resume_state(self, resume):
        """args.resume: the cumulative delta beside the base when it cites that base, otherwise the base alone."""
        from . import train_state as ts
        base = ts.rank_path(resume, self.comm.rank)
        delta = ts.rank_path(ts.delta_path(resume), self.comm.rank)
        take = base
        if os.path.exists(delta):
            try:
                if ts.cites(ts.read_manifest(delta), ts.read_manifest(base), where=base) is None:
                    take = delta
            except (ValueError, KeyError, TypeError):     # (StateError is a ValueError) a delta or base that cannot be read as one
                pass
        print("resuming from", take, "(delta over %s)" % base if take is delta else "(full state)")
        self.load_training_state(take, base=base if take is delta else None)

    def _save_epoch_state(self, state_path, epoch):
        """learn()'s save after an epoch.  args.state_full_every = k >= 1: every k-th save rewrites the base `state_path`, the
        saves between rewrite ONE cumulative delta beside it against that base; 0: every save is full."""
        from . import train_state as ts
        base = ts.rank_path(state_path, self.comm.rank)
        every = int(self._arg("state_full_every") or 0)
        if every <= 0:
            return self.save_training_state(base, epoch=epoch)
        delta = ts.rank_path(ts.delta_path(state_path), self.comm.rank)
        n = self._state_saves
        self._state_saves = n + 1
        if n % every != 0:
            try:
                ts.known_base(self, base)
            except ts.StateError:
                pass          # e.g. the first save after a resume from a delta: its base is older than the restore
            else:
                return self.save_training_state(delta, epoch=epoch, base=base)
        # re-base: the new base first, the stale delta after -- a crash between the two leaves a valid, newer, full state (and
        # a delta that cites another base, which a resume does not take)
        out = self.save_training_state(base, epoch=epoch)
        self._state_saves = 1
        if os.path.exists(delta):
            os.unlink(delta)
        return out

    def learn(self):
        """ddpg_agent.py:92-161 with the learner half on the device.

        The reference draws exploration noise (:177-183), overflow slots (replay_buffer.py:64,67) and HER indices
        (her.py:24-31) from ONE stream, numpy's global one.  With `args.share_numpy_stream` (default) that single stream
        is handed to the device for the learner phase of every cycle and taken back before the next rollout, so a run
        seeded like train.py:34-39 consumes exactly the reference's random words in the reference's order (with one
        environment; a list of environments is stepped in lockstep, which reorders the exploration draws).  The
        hand-back synchronises, which the next rollout needs anyway: it evaluates the updated actor.

        With a vectorised device environment every draw of a cycle comes from the device stream, so the stream stays on the device
        for the whole run: numpy's state is handed over once and handed back at the end and wherever a training state is saved,
        and nothing synchronises between the rollout and the learner phase of a cycle."""
        share, device = bool(self._arg("share_numpy_stream")), self.vec_env is not None
        # optional: args.resume = a training state to continue from (ddpg_agent.py:54-62), args.state_path = where to save one
        # after every epoch's evaluation; each rank has its own file (its buffer is its shard of the episodes)
        state_path, resume, first_epoch = self._arg("state_path"), self._arg("resume"), 0
        if device and self._arg("explore_streams") and self.explore_streams is None:
            self.enable_explore_streams()    # args.explore_streams: before a resume, whose state carries the streams' states
        if device and self._arg("device_reset") and getattr(self.vec_env, "reset_streams", None) is None:
            self.vec_env.enable_device_reset(self.ctx)   # args.device_reset: likewise before a resume
        if self._demo_preload_pending:
            self._init_demo_buffer()                     # demo_source='device': generated now that the reset is on the device
        if resume:
            self._resume_state(resume)
            first_epoch = self.resumed_at[0]
        print("initial buffer size:", self.buffer.current_size)                  # :97

        def hand_over():
            if share:
                self.rng.set_state(np.random.get_state())

        def hand_back():
            if share:
                np.random.set_state(self.rng.get_state())

        collect = self.collect_episodes_device if device else self.collect_episodes
        if device:
            hand_over()
        for epoch in range(first_epoch, self.args.n_epochs):
            start = time.time()
            episodes = None
            for _ in range(self.args.n_cycles):
                episodes = collect(n_rollouts=self.args.num_rollouts_per_mpi, epoch=epoch)
                if not device:
                    hand_over()
                self.train_cycle(episodes)
                if not device:
                    hand_back()
            self._queue_epoch_audits(episodes)       # args.audit_policy / audit_actor_signal / audit_bellman: recorded by _finish_epoch
            self._finish_epoch(epoch, start, state_path, before_save=hand_back if device else None)
        if device:
            hand_back()

    def _finish_epoch(self, epoch, start, state_path, before_save=None):
        """What closes an epoch of learn() on either path (:151-161): wait for its cycles, print the time they took, evaluate,
        checkpoint on rank 0, and save the training state where one is asked for (`before_save()` first)."""
        self.ctx.synchronize()
        self.check_exchange()
        print(str(time.time() - start))
        self._record_policy_audit()      # args.audit_policy: before the evaluation, which may collect into the same block
        self._record_actor_signal_audit()     # args.audit_actor_signal: likewise
        self._record_bellman_audit()          # args.audit_bellman: likewise
        rate = self._eval_agent()
        self.success_rates.append(rate)
        if self.comm.rank == 0:
            print('[{}] epoch is: {}, eval success rate is: {:.3f}'.format(datetime.now(), epoch, rate))
            self.save_checkpoint()
        if state_path:
            if before_save is not None:
                before_save()
            self._save_epoch_state(state_path, epoch + 1)

    def __del__(self):
        try:
            self._flush_updates()     # counted `_update_network()` calls are owed even if nobody looks at the result
        except Exception:
            pass
        try:
            _lib.unregister_pending(self)
            self.lib.hp_agent_destroy(self.h)
        except Exception:
            pass
