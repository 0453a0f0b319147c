"""The five audits of recorded episodes as the agent runs them: the metrics (hp_episode_stats*), the critic audit
(hp_episode_q*, hp_episode_returns*), the policy audit (hp_episode_policy*), the actor-signal audit (hp_episode_action_grad*,
hp_episode_signal_stats*) and the Bellman audit (hp_episode_bellman*), each on a `DeviceEpisodes` block in place or on
host episodes that are uploaded first, and what puts an epoch's summary onto the agent's lists.  `ddpg_agent` inherits these
methods; they use its `lib`, `ctx`, `h`, `o_norm`, `g_norm`, `args`, `_arg`, `env_params`, `vec_env` and `comm`."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, synthetic
from ._lib import NET_CRITIC, NET_CRITIC_TARGET


def _p(t):
    """a device tensor's address; None (an array the call does not take) stays None"""
    return None if t is None else C.c_void_p(t.data_ptr())


def _upload(agent, episode_batch, who, arrays=4):
    """The first `arrays` of (obs, ag, g, actions) of host episodes as float64 device tensors, refused under `who`'s name when their
    shapes do not belong together or (with obs and actions among them) differ from the agent's.  arrays=2: ag and g alone."""
    if arrays == 2:
        ag, g = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)) for a in episode_batch[1:3])
        if ag.ndim != 3 or g.ndim != 3 or ag.shape[0] != g.shape[0] or ag.shape[1] != g.shape[1] + 1 or ag.shape[2] != g.shape[2]:
            raise ValueError(f"{who}: ag [n, T+1, goal] and g [n, T, goal] expected")
        host = (ag, g)
    else:
        obs, ag, g, act = host = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)) for a in episode_batch[:4])
        if (any(a.ndim != 3 for a in host) or len({a.shape[0] for a in host}) != 1
                or not obs.shape[1] == ag.shape[1] == g.shape[1] + 1 == act.shape[1] + 1 or ag.shape[2] != g.shape[2]):
            raise ValueError(f"{who}: obs [n, T+1, obs], ag [n, T+1, goal], g [n, T, goal] and actions [n, T, act] expected")
        if (obs.shape[2], g.shape[2], act.shape[2]) != tuple(int(agent.env_params[k]) for k in ('obs', 'goal', 'action')):
            raise ValueError(f"{who}: the episodes' dimensions differ from the agent's")
    dev = torch.device("cuda", agent.ctx.device_id)
    return tuple(a.to(dev) for a in host)


def _span(episodes, first, n):
    """(first, n) of a call on a `DeviceEpisodes`: n defaults to the episodes from `first` on"""
    first = int(first)
    return first, (len(episodes) - first if n is None else int(n))


def _goal_mode(goal):
    """HP_GOAL_DESIRED / HP_GOAL_FINAL of a Bellman audit's `goal`"""
    if goal == "desired":
        return _lib.GOAL_DESIRED
    if goal == "final":
        return _lib.GOAL_FINAL
    raise ValueError(f"episode_bellman: goal {goal!r} is neither 'desired' nor 'final'")


def _record(agent, names, summary, onto):
    """One summary (this rank's means, in the columns `names`), averaged over the ranks like the success rate, onto the list"""
    local = torch.tensor(np.asarray(summary, dtype=np.float64), dtype=torch.float64)
    if agent.comm.world_size > 1:
        local = local.to(f"cuda:{agent.ctx.device_id}")
    agent.comm.allreduce_mean_(local)
    onto.append(dict(zip(names, (float(v) for v in local.cpu().numpy()))))


class EpisodeAudit:
    def episode_stats_host(self, episode_batch, distance_threshold):
        """The metrics of host episodes -- the four arrays `collect_episodes` returns, or a feeder slot's (obs, ag, g, actions) --
        from the kernel the device path uses (hp_episode_stats): `ag` and `g` are uploaded, the result comes back as numpy
        (stats [n, 6] float64 in the columns of `synthetic.EPISODE_STATS`, step_success [n, T] float32).  Synchronises."""
        ag, g = _upload(self, episode_batch, "episode_stats_host", arrays=2)
        n, T, gd = g.shape
        stats = torch.empty((n, _lib.EPISODE_STATS), dtype=torch.float64, device=g.device)
        flags = torch.empty((n, T), dtype=torch.float32, device=g.device)
        with self.ctx.torch_bridge():
            _lib.check(self.lib.hp_episode_stats(self.ctx.h, _p(ag), _p(g), n, T, gd, float(distance_threshold), _p(stats), _p(flags)))
        return stats.cpu().numpy(), flags.cpu().numpy()

    # ---- the two network forwards and the policy columns: one place per entry pair.  `episodes`: a DeviceEpisodes, whose
    # episodes [first, first + n) are read in place (the *_block entry); None: the uploaded arrays are (the plain entry)
    def _entry_pair(self, episodes, block, block_args, plain, plain_args):
        """One call of an entry pair on torch's current stream: `block(episodes.h, *block_args)` for a DeviceEpisodes, else
        `plain(*plain_args)`"""
        with self.ctx.torch_bridge():
            if episodes is not None:
                _lib.check(block(episodes.h, *block_args))
            else:
                _lib.check(plain(*plain_args))

    def _q(self, episodes, first, n, T, target, obs=None, g=None, act=None):
        q = torch.empty((max(n, 0), T), dtype=torch.float32, device=torch.device("cuda", self.ctx.device_id))
        nets = (self.h, self.o_norm.h, self.g_norm.h, NET_CRITIC_TARGET if target else NET_CRITIC)
        tail = (float(self.args.clip_obs), _p(q))
        self._entry_pair(episodes, self.lib.hp_episode_q_block, (*nets, first, n, *tail),
                         self.lib.hp_episode_q, (*nets, _p(obs), _p(g), _p(act), n, T, *tail))
        return q

    def _policy(self, episodes, first, n, T, target, obs=None, g=None):
        dev = torch.device("cuda", self.ctx.device_id)
        pi = torch.empty((max(n, 0), T, int(self.env_params['action'])), dtype=torch.float32, device=dev)
        q_pi = torch.empty((max(n, 0), T), dtype=torch.float32, device=dev)
        nets = (self.h, self.o_norm.h, self.g_norm.h, 1 if target else 0)
        tail = (float(self.args.clip_obs), _p(pi), _p(q_pi))
        self._entry_pair(episodes, self.lib.hp_episode_policy_block, (*nets, first, n, *tail),
                         self.lib.hp_episode_policy, (*nets, _p(obs), _p(g), n, T, *tail))
        return pi, q_pi

    def _policy_columns(self, episodes, first, pi, q_pi, q, sat, act=None):
        n, T, ad = pi.shape
        stats = torch.empty((n, _lib.POLICY_STATS), dtype=torch.float64, device=q.device)
        tail = (float(self.env_params['action_max']), float(sat), _p(stats))
        self._entry_pair(episodes, self.lib.hp_episode_policy_stats_block, (_p(pi), _p(q_pi), _p(q), first, n, *tail),
                         self.lib.hp_episode_policy_stats, (self.ctx.h, _p(pi), _p(q_pi), _p(act), _p(q), n, T, ad, *tail))
        return stats

    def episode_q(self, episodes, target=False, first=0, n=None):
        """What the critic believes of episodes [first, first + n) of a `DeviceEpisodes` (a collection's, an evaluation's, or
        `generate_demos(...).episodes`: what the critic thinks of the demonstrations): Q(s_t, a_t) of every recorded step, a
        float32 device tensor [n, T], from one launch on torch's current stream (hp_episode_q_block) -- the training chain's
        critic forward on rows that enter it exactly as they enter an update (clip_obs from `args`, the normalizers' current
        statistics, the recorded action over max_action).  `target=True`: the target critic.  No copy, no synchronisation."""
        return self._q(episodes, *_span(episodes, first, n), episodes.T, target)

    def episode_critic_stats(self, episodes, distance_threshold=None, target=False, tail="persist", first=0, n=None):
        """The critic audited on episodes [first, first + n) of a `DeviceEpisodes`: (stats [n, 6] float64 in the columns of
        `synthetic.CRITIC_STATS`, q [n, T] float32, returns [n, T] float64), device tensors from two launches (`episode_q`,
        `DeviceEpisodes.returns`).  The threshold defaults to `vec_env.distance_threshold`; gamma and reward_type are `args`'."""
        if distance_threshold is None:
            distance_threshold = self.vec_env.distance_threshold
        q = self.episode_q(episodes, target=target, first=first, n=n)
        returns, stats = episodes.returns(distance_threshold, float(self.args.gamma), self._arg("reward_type"),
                                          tail, first=first, n=n, q=q)
        return stats, q, returns

    def episode_critic_stats_host(self, episode_batch, distance_threshold, target=False, tail="persist"):
        """`episode_critic_stats` for host episodes -- the four arrays `collect_episodes` returns, or a feeder slot's (obs, ag, g,
        actions): they are uploaded, the same kernels run (hp_episode_q, hp_episode_returns) and the result comes back as numpy
        (stats [n, 6] float64, q [n, T] float32, returns [n, T] float64).  Synchronises."""
        from .synthetic import _reward_kind, _tail_kind
        obs, ag, g, act = _upload(self, episode_batch, "episode_critic_stats_host")
        n, T, gd = g.shape
        q = self._q(None, 0, n, T, target, obs, g, act)
        returns = torch.empty((n, T), dtype=torch.float64, device=g.device)
        stats = torch.empty((n, _lib.CRITIC_STATS), dtype=torch.float64, device=g.device)
        with self.ctx.torch_bridge():
            _lib.check(self.lib.hp_episode_returns(self.ctx.h, _p(ag), _p(g), n, T, gd, float(distance_threshold),
                                                   _reward_kind(self._arg("reward_type")), float(self.args.gamma),
                                                   _tail_kind(tail), _p(returns), _p(q), _p(stats)))
        return stats.cpu().numpy(), q.cpu().numpy(), returns.cpu().numpy()

    def episode_policy(self, episodes, target=False, first=0, n=None):
        """What the actor's objective sees of episodes [first, first + n) of a `DeviceEpisodes`: (pi [n, T, act] float32, the
        policy's action at every recorded state, q_pi [n, T] float32, Q(s_t, pi(s_t))), device tensors from one launch on
        torch's current stream (hp_episode_policy_block) -- the forward half of an update's actor-side chain on rows that enter
        it exactly as they enter an update.  `target=True`: target actor and target critic.  No copy, no synchronisation."""
        return self._policy(episodes, *_span(episodes, first, n), episodes.T, target)

    def episode_policy_stats(self, episodes, target=False, sat=0.99, first=0, n=None):
        """The policy audited on episodes [first, first + n) of a `DeviceEpisodes` (a collection's, an evaluation's, or
        `generate_demos(...).episodes`, where the q_filter_share column is the Q-filter rate): (stats [n, 6] float64 in the
        columns of `synthetic.POLICY_STATS`, pi, q_pi, q), device tensors from three launches (`episode_q`, `episode_policy`,
        the columns: hp_episode_policy_stats_block).  No copy, no synchronisation."""
        q = self.episode_q(episodes, target=target, first=first, n=n)
        pi, q_pi = self.episode_policy(episodes, target=target, first=first, n=n)
        return self._policy_columns(episodes, int(first), pi, q_pi, q, sat), pi, q_pi, q

    def episode_policy_stats_host(self, episode_batch, target=False, sat=0.99):
        """`episode_policy_stats` for host episodes -- the four arrays `collect_episodes` returns, or a feeder slot's (obs, ag, g,
        actions): they are uploaded, the same kernels run (hp_episode_q, hp_episode_policy, hp_episode_policy_stats) and the
        result comes back as numpy (stats [n, 6] float64, pi [n, T, act] float32, q_pi [n, T] float32, q [n, T] float32).
        Synchronises."""
        obs, _, g, act = _upload(self, episode_batch, "episode_policy_stats_host")
        n, T, _ = act.shape
        q = self._q(None, 0, n, T, target, obs, g, act)
        pi, q_pi = self._policy(None, 0, n, T, target, obs, g)
        stats = self._policy_columns(None, 0, pi, q_pi, q, sat, act)
        return stats.cpu().numpy(), pi.cpu().numpy(), q_pi.cpu().numpy(), q.cpu().numpy()

    # ---- the actor signal: dQ/du of every step (hp_episode_action_grad*) and its columns (hp_episode_signal_stats*)
    def _action_grad(self, episodes, first, n, T, target, at, obs=None, g=None, act=None):
        if at not in ("policy", "recorded"):
            raise ValueError(f"episode_action_grad: at {at!r} is neither 'policy' nor 'recorded'")
        dev = torch.device("cuda", self.ctx.device_id)
        ad, at_policy = int(self.env_params['action']), at == "policy"
        dq_du = torch.empty((max(n, 0), T, ad), dtype=torch.float32, device=dev)
        pi = torch.empty((max(n, 0), T, ad), dtype=torch.float32, device=dev) if at_policy else None
        q = torch.empty((max(n, 0), T), dtype=torch.float32, device=dev)
        nets = (self.h, self.o_norm.h, self.g_norm.h, 1 if target else 0, 0 if at_policy else 1)
        tail = (float(self.args.clip_obs), _p(pi), _p(q), _p(dq_du))
        self._entry_pair(episodes, self.lib.hp_episode_action_grad_block, (*nets, first, n, *tail),
                         self.lib.hp_episode_action_grad, (*nets, _p(obs), _p(g), _p(act), n, T, *tail))
        return dq_du, pi, q

    def _signal_columns(self, episodes, first, pi, dq_du, flat, act=None):
        n, T, ad = pi.shape
        stats = torch.empty((n, _lib.SIGNAL_STATS), dtype=torch.float64, device=pi.device)
        tail = (float(self.env_params['action_max']), float(self.args.action_l2), float(flat), _p(stats))
        self._entry_pair(episodes, self.lib.hp_episode_signal_stats_block, (_p(pi), _p(dq_du), first, n, *tail),
                         self.lib.hp_episode_signal_stats, (self.ctx.h, _p(pi), _p(dq_du), _p(act), n, T, ad, *tail))
        return stats

    def episode_action_grad(self, episodes, target=False, at="policy", first=0, n=None):
        """The quantity that moves the actor, on episodes [first, first + n) of a `DeviceEpisodes`: (dq_du [n, T, act] float32,
        pi [n, T, act] float32 or None, q [n, T] float32), device tensors from one launch on torch's current stream
        (hp_episode_action_grad_block) -- an update's actor-side chain up to the action columns of the critic's input gradient,
        seeded with 1 per row.  dq_du is the derivative with respect to the critic's action input u = a / max_action; dQ/da is
        dq_du / max_action.  at="policy": at u = pi(s) / max_action; pi and q = Q(s, pi(s)) are `episode_policy`'s bits.
        at="recorded": at the recorded action; pi is None and q = Q(s, a) is `episode_q`'s bits.  `target=True` is refused by
        the library: the target networks keep no dX-order fragments.  No copy, no synchronisation."""
        return self._action_grad(episodes, *_span(episodes, first, n), episodes.T, target, at)

    def episode_signal_stats(self, episodes, flat=1e-3, first=0, n=None):
        """The actor's learning signal audited on episodes [first, first + n) of a `DeviceEpisodes`: (stats [n, 6] float64 in
        the columns of `synthetic.SIGNAL_STATS`, dq_du, pi, q_pi), device tensors from two launches (`episode_action_grad` at
        the policy, the columns: hp_episode_signal_stats_block, with `args.action_l2` as the regulariser's weight).  No copy, no
        synchronisation."""
        dq_du, pi, q_pi = self.episode_action_grad(episodes, first=first, n=n)
        return self._signal_columns(episodes, int(first), pi, dq_du, flat), dq_du, pi, q_pi

    def episode_signal_stats_host(self, episode_batch, flat=1e-3):
        """`episode_signal_stats` for host episodes -- the four arrays `collect_episodes` returns, or a feeder slot's (obs, ag, g,
        actions): they are uploaded, the same kernels run (hp_episode_action_grad, hp_episode_signal_stats) and the result comes
        back as numpy (stats [n, 6] float64, dq_du [n, T, act] float32, pi [n, T, act] float32, q_pi [n, T] float32).
        Synchronises."""
        obs, _, g, act = _upload(self, episode_batch, "episode_signal_stats_host")
        n, T, _ = act.shape
        dq_du, pi, q_pi = self._action_grad(None, 0, n, T, False, "policy", obs, g, act)
        stats = self._signal_columns(None, 0, pi, dq_du, flat, act)
        return stats.cpu().numpy(), dq_du.cpu().numpy(), pi.cpu().numpy(), q_pi.cpu().numpy()

    # ---- the Bellman residual: Q, Q' of the next state, reward and target of every step (hp_episode_bellman*) and its columns
    def _bellman(self, episodes, first, n, T, goal, distance_threshold, obs=None, ag=None, g=None, act=None):
        from .synthetic import _reward_kind
        mode = _goal_mode(goal)
        dev = torch.device("cuda", self.ctx.device_id)
        q, q_next, r, y = out = tuple(torch.empty((max(n, 0), T), dtype=torch.float32, device=dev) for _ in range(4))
        tail = (float(distance_threshold), _reward_kind(self._arg("reward_type")), float(self.args.clip_obs), *(_p(v) for v in out))
        nets = (self.h, self.o_norm.h, self.g_norm.h, mode)
        self._entry_pair(episodes, self.lib.hp_episode_bellman_block, (*nets, first, n, *tail),
                         self.lib.hp_episode_bellman, (*nets, _p(obs), _p(ag), _p(g), _p(act), n, T, *tail))
        return out

    def _bellman_columns(self, q, q_next, r, y):
        stats = torch.empty((q.shape[0], _lib.BELLMAN_STATS), dtype=torch.float64, device=q.device)
        with self.ctx.torch_bridge():
            _lib.check(self.lib.hp_episode_bellman_stats(self.ctx.h, _p(q), _p(q_next), _p(r), _p(y), q.shape[0], q.shape[1],
                                                         float(self.args.gamma), _p(stats)))
        return stats

    def episode_bellman(self, episodes, goal="desired", distance_threshold=None, first=0, n=None):
        """The quantity the critic is trained on, on episodes [first, first + n) of a `DeviceEpisodes` (a collection's, an
        evaluation's, or `generate_demos(...).episodes`): (q, q_next, r, y), float32 device tensors [n, T] from one launch on
        torch's current stream (hp_episode_bellman_block) -- q = Q(s_t, a_t) of the online critic, q_next =
        Q'(s_{t+1}, pi'(s_{t+1})) of the target networks, r the transition's reward and y = clamp(r + gamma q_next,
        -1 / (1 - gamma), 0) by an update's own float32 operations; the TD error is y - q.  goal="desired": under the block's own
        goals, as an unrelabelled transition enters an update (q is `episode_q`'s bits).  goal="final": every step of an episode
        under the goal the episode achieved last, the hindsight relabel under which every episode ends in success.  The
        threshold defaults to `vec_env.distance_threshold`; gamma and reward_type are `args`'.  No copy, no synchronisation."""
        if distance_threshold is None:
            distance_threshold = self.vec_env.distance_threshold
        return self._bellman(episodes, *_span(episodes, first, n), episodes.T, goal, distance_threshold)

    def episode_bellman_stats(self, episodes, goal="desired", distance_threshold=None, first=0, n=None):
        """The Bellman residual audited on episodes [first, first + n) of a `DeviceEpisodes`: (stats [n, 6] float64 in the
        columns of `synthetic.BELLMAN_STATS`, q, q_next, r, y), device tensors from two launches (`episode_bellman`, the columns:
        hp_episode_bellman_stats).  No copy, no synchronisation."""
        out = self.episode_bellman(episodes, goal=goal, distance_threshold=distance_threshold, first=first, n=n)
        return (self._bellman_columns(*out), *out)

    def episode_bellman_stats_host(self, episode_batch, distance_threshold, goal="desired"):
        """`episode_bellman_stats` for host episodes -- the four arrays `collect_episodes` returns, or a feeder slot's (obs, ag, g,
        actions): they are uploaded, the same kernels run (hp_episode_bellman, hp_episode_bellman_stats) and the result comes
        back as numpy (stats [n, 6] float64, q, q_next, r, y [n, T] float32).  Synchronises."""
        obs, ag, g, act = _upload(self, episode_batch, "episode_bellman_stats_host")
        n, T, _ = g.shape
        out = self._bellman(None, 0, n, T, goal, distance_threshold, obs, ag, g, act)
        return tuple(v.cpu().numpy() for v in (self._bellman_columns(*out), *out))

    def _column_means(self, entry, rows):
        """The column means of a per-episode table on the device, a float64 device tensor of rows.shape[1] values from one launch
        of `entry` (hp_episode_stats_summary, hp_episode_critic_summary, hp_episode_policy_summary, hp_episode_signal_summary or
        hp_episode_bellman_summary)"""
        summary = torch.empty(rows.shape[1], dtype=torch.float64, device=rows.device)
        with self.ctx.torch_bridge():
            _lib.check(entry(self.ctx.h, _p(rows), rows.shape[0], _p(summary)))
        return summary

    def _queue_epoch_audits(self, episodes):
        """args.audit_policy / args.audit_actor_signal / args.audit_bellman: queue an epoch's last exploring episodes for
        `_record_policy_audit` / `_record_actor_signal_audit` / `_record_bellman_audit`, under the networks as they now stand.  A
        `DeviceEpisodes`: the columns and their means are launched now behind the cycle (four launches for the policy, then three
        for the signal: dQ/du at the policy, the columns, their means; then three for the Bellman residual), nothing waits, and the summary tensor is kept -- its 48 bytes are read behind the epoch's synchronise.
        Host arrays are kept as they are and audited there."""
        if episodes is None:
            return
        span = dict(first=0, n=len(episodes)) if hasattr(episodes, "block") else None      # a DeviceEpisodes: all of its episodes
        if self._arg("audit_policy"):
            self._policy_audit_pending = episodes if span is None else self._column_means(
                self.lib.hp_episode_policy_summary, self.episode_policy_stats(episodes, **span)[0])
        if self._arg("audit_actor_signal"):
            self._actor_signal_pending = episodes if span is None else self._column_means(
                self.lib.hp_episode_signal_summary, self.episode_signal_stats(episodes, **span)[0])
        goal = self._arg("audit_bellman")
        if goal:
            _goal_mode(goal)
            self._bellman_pending = episodes if span is None else self._column_means(
                self.lib.hp_episode_bellman_summary, self.episode_bellman_stats(episodes, goal=goal, **span)[0])

    def _bellman_host_stats(self, eps):
        """`episode_bellman_stats_host` at the environment's threshold, as the host evaluation takes it, under args.audit_bellman"""
        thr = self.env.distance_threshold if hasattr(self.env, "distance_threshold") else self._arg("distance_threshold")
        return self.episode_bellman_stats_host(eps, thr, goal=self._arg("audit_bellman"))

    # an epoch's audit: the pending attribute, the columns and the summary of `synthetic` (the objects themselves: a wrong name fails
    # when the module is imported), the host path's audit -- looked up on the agent at the call, so that whoever wraps an agent's
    # `episode_*_stats_host` sees the call -- and the target list
    _EPOCH_AUDITS = {
        "policy": ("_policy_audit_pending", synthetic.POLICY_STATS, synthetic.episode_policy_summary,
                   lambda agent, eps: agent.episode_policy_stats_host(eps), "policy_audit"),
        "actor_signal": ("_actor_signal_pending", synthetic.SIGNAL_STATS, synthetic.episode_signal_summary,
                         lambda agent, eps: agent.episode_signal_stats_host(eps), "actor_signal_audit"),
        "bellman": ("_bellman_pending", synthetic.BELLMAN_STATS, synthetic.episode_bellman_summary,
                    lambda agent, eps: agent._bellman_host_stats(eps), "bellman_audit"),
    }

    def _record_epoch_audit(self, which):
        """An epoch's pending audit -- the device path's summary (six means, already computed) or the host path's episodes (audited
        now) -- averaged over the ranks like the success rate, onto its list; None: nothing is pending"""
        attr, names, summary, host_stats, onto = self._EPOCH_AUDITS[which]
        pending = getattr(self, attr)
        setattr(self, attr, None)
        if pending is not None:
            means = pending.cpu().numpy() if isinstance(pending, torch.Tensor) else summary(host_stats(self, pending)[0])
            _record(self, names, means, getattr(self, onto))

    def _record_policy_audit(self):
        """args.audit_policy: the epoch's pending audit (host episodes: `episode_policy_stats_host`) onto `policy_audit`"""
        self._record_epoch_audit("policy")

    def _record_actor_signal_audit(self):
        """args.audit_actor_signal: the epoch's pending audit (host episodes: `episode_signal_stats_host`) onto `actor_signal_audit`"""
        self._record_epoch_audit("actor_signal")

    def _record_bellman_audit(self):
        """args.audit_bellman: the epoch's pending audit (host episodes: `episode_bellman_stats_host`) onto `bellman_audit`"""
        self._record_epoch_audit("bellman")

    def _record_eval_metrics(self, summary):
        """One evaluation's summary (this rank's six means), averaged over the ranks like the success rate, onto `eval_metrics`"""
        from .synthetic import EPISODE_SUMMARY
        _record(self, EPISODE_SUMMARY, summary, self.eval_metrics)

    def _record_eval_critic(self, summary):
        """One evaluation's critic summary (this rank's six means), averaged over the ranks like the success rate, onto `eval_critic`"""
        from .synthetic import CRITIC_STATS
        _record(self, CRITIC_STATS, summary, self.eval_critic)
