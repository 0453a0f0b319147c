"""The rollout side of the agent: the batched policy call, exploration, collection of episodes from host
environments stepped in lockstep or from a vectorised device environment in its three forms, and both evaluations.  `ddpg_agent`
inherits these methods; they use its `lib`, `ctx`, `h`, `o_norm`, `g_norm`, `rng`, `buffer`, `args`, `env_params`, `envs`, `env`,
`vec_env`, `comm`, `explore_streams`, the `rollout_*` fields, `_rollouts`, `_slab8`, `_arg` and `_flush_updates`, and
`EpisodeAudit`'s `episode_critic_stats*`, `_column_means` and `_record_eval_*`."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import random as _random
from ._lib import NET_ACTOR, NET_ACTOR_TARGET


def lockstep_episodes(envs, n, T, policy, to_action, follow_goal=False):
    """`n` episodes of `T` steps from the environments `envs`, stepped in lockstep with one `policy(obs_stack, g_stack) ->
    float32 [k, act]` call per timestep (the rollout loop of the reference's learn(), ddpg_agent.py:105-137, and of its
    _eval_agent, :280-304).  Returns ([obs [n, T+1, obs], ag [n, T+1, goal], g [n, T, goal], actions [n, T, act]] float64, the
    success flag of each episode's last step as float64 [n]).  What the two callers differ in:
      action type     `to_action(policy_row)` is what `env.step` is handed.  Collection passes the explored action, or
                      `row.astype(np.float64)` when not exploring, with the +-0.15 clip from epoch 100; evaluation passes the
                      float32 policy row itself, unclipped.
      recorded action `np.array(action, dtype=np.float64)` of what was stepped.
      desired goal    collection keeps the desired goal of the reset for the whole episode (follow_goal=False, :105-137);
                      evaluation follows `observation_new['desired_goal']` every step (follow_goal=True, :280-304).
      success flag    `info.get('is_success', previous)`, 0.0 before the first step; collection ignores it.
      draw order      environments are stepped in list order within a timestep, so the draws `to_action` makes (e.g.
                      `_select_actions` on numpy's global stream) come in environment order.
      short last wave episodes come in waves of len(envs); a last wave of fewer uses the first environments."""
    mb, wins, done = ([], [], [], []), [], 0
    while done < n:
        wave = envs[:n - done]
        first = [env.reset() for env in wave]
        obs = [o['observation'] for o in first]
        ag = [o['achieved_goal'] for o in first]
        g = [o['desired_goal'] for o in first]
        ep = [([], [], [], []) for _ in wave]
        last = [0.0] * len(wave)
        for _t in range(T):
            pi = policy(np.stack(obs), np.stack(g))
            for i, env in enumerate(wave):
                action = to_action(pi[i])
                observation_new, _, _, info = env.step(action)
                for dst, v in zip(ep[i], (obs[i], ag[i], g[i], action)):
                    dst.append(np.array(v, dtype=np.float64))
                obs[i], ag[i] = observation_new['observation'], observation_new['achieved_goal']
                if follow_goal:
                    g[i] = observation_new['desired_goal']
                last[i] = float(info.get('is_success', last[i]))
        for i in range(len(wave)):
            ep[i][0].append(np.array(obs[i], dtype=np.float64)); ep[i][1].append(np.array(ag[i], dtype=np.float64))
            for dst, src in zip(mb, ep[i]):
                dst.append(src)
        wins.extend(last)
        done += len(wave)
    return [np.array(a) for a in mb], np.array(wins, dtype=np.float64)


class Rollouts:
    def _preproc_inputs(self, obs, g):
        inputs = np.concatenate([self.o_norm.normalize(obs), self.g_norm.normalize(g)])
        return torch.tensor(inputs, dtype=torch.float32).unsqueeze(0)

    def act(self, obs, g, target=False, clip_obs=0.0):
        """_preproc_inputs (:163-171) + actor (:114-116) for a stack of environments in ONE device call: obs [n, obs] and
        g [n, goal] float64 (or single rows) -> actions [n, action] float32.  clip_obs > 0 also clips the raw values to
        +-clip_obs first, which is what the checkpoint reader demo_push.py:15-22 does (the rollouts do not)."""
        obs, g = _lib.as_f64(obs), _lib.as_f64(g)
        o2, g2 = obs.reshape(-1, obs.shape[-1]), g.reshape(-1, g.shape[-1])
        if o2.shape[0] != g2.shape[0]:
            raise ValueError("act: observation and goal stacks differ in length")
        out = np.empty((o2.shape[0], self.env_params['action']), np.float32)
        d = C.c_double
        _lib.check(self.lib.hp_agent_act(self.h, self.o_norm.h, self.g_norm.h, NET_ACTOR_TARGET if target else NET_ACTOR,
                                         _lib.ptr(o2, d), _lib.ptr(g2, d), o2.shape[0], float(clip_obs),
                                         _lib.ptr(out, C.c_float)))
        return out.reshape(obs.shape[:-1] + (out.shape[-1],))

    def act_device(self, obs_t, g_t, target=False, clip_obs=0.0):
        """`act` for float64 device tensors [n, obs] / [n, goal] (or single rows): the same kernels on the tensors' memory, a
        float32 device tensor back.  Runs in torch's current stream order; no copy, no synchronisation."""
        if obs_t.dtype != torch.float64 or g_t.dtype != torch.float64 or not obs_t.is_cuda or not g_t.is_cuda:
            raise ValueError("act_device: float64 tensors on the context's device expected")
        o2 = obs_t.reshape(-1, obs_t.shape[-1]).contiguous()
        g2 = g_t.reshape(-1, g_t.shape[-1]).contiguous()
        if o2.shape[0] != g2.shape[0]:
            raise ValueError("act: observation and goal stacks differ in length")
        out = torch.empty((o2.shape[0], self.env_params['action']), dtype=torch.float32, device=o2.device)
        self._flush_updates()
        with self.ctx.torch_bridge():
            _lib.check(self.lib.hp_agent_act_dev(self.h, self.o_norm.h, self.g_norm.h, NET_ACTOR_TARGET if target else NET_ACTOR,
                                                 C.c_void_p(o2.data_ptr()), C.c_void_p(g2.data_ptr()), o2.shape[0],
                                                 float(clip_obs), C.c_void_p(out.data_ptr())))
        return out.reshape(tuple(obs_t.shape[:-1]) + (out.shape[-1],))

    def enable_explore_streams(self, base_seed=None, seeds=None):
        """Give every environment of the vectorised simulator its own exploration stream (random.DeviceRandomStreams,
        hp_rollout_step_streams): env i draws `_select_actions` out of `RandomState(seeds[i])` alone -- n reference workers
        (one environment and one stream seeded `seed + rank` each, train.py:34-39) side by side -- so its trajectory depends
        neither on n_envs nor on the wave it is part of, and the draw of a timestep is one wave per environment instead of one
        wave for all.  Default seeds: base_seed + i with base_seed = args.seed + rank * n_envs, distinct over all environments
        of all ranks.  `self.rng` then serves the learner alone (overflow slots, HER indices)."""
        if self.vec_env is None:
            raise ValueError("enable_explore_streams: the agent has no vectorised device environment")
        n = int(self.vec_env.n_envs)
        if seeds is None and base_seed is None:
            base_seed = int(self.args.seed) + self.comm.rank * n
        self.explore_streams = _random.DeviceRandomStreams(n, seeds=seeds, base_seed=base_seed, ctx=self.ctx)
        return self.explore_streams

    def collect_episodes_device(self, vec_env=None, n_rollouts=None, epoch=0, explore=True, success_out=None, stats_out=None):
        """`collect_episodes` for a vectorised device environment (device_env.py): `n_rollouts` episodes (default: one wave of
        vec_env.n_envs) on torch's current stream, no host copy and no host wait per timestep, in one of three forms with the
        same bits; `self.rollout_form` / `self.rollout_reason` say which the call took and why, `self.rollout_launches` how many
        launches a fused call was.
          stepped (`_collect_wave_stepped`): waves of n_envs, T timesteps of two launches each (csrc/rollout.hip).
          fused, one launch per wave (`_collect_wave_fused`): a native environment, a slab-shaped agent and draws that are
            independent across environments (`device_env.fused_rollout_reason`).
          fused, all waves in one launch (`_collect_all_waves`): the same with an environment that is reset on the device
            (`vec_env.enable_device_reset()`); calls no `vec_env.reset()`, hands `success_out` one tensor of n_rollouts flags,
            and the launch cap may make a few launches of it.
        Exploration (:174-184, the +-0.15 clip from epoch 100) is drawn on the device from `self.rng`, for env 0 .. n-1 in turn
        like the host lockstep path -- or, after `enable_explore_streams`, for every environment from its own stream (a wave of
        k < n_envs rows advances the streams of those k only).  Returns a `DeviceEpisodes` handle for `train_cycle` /
        `buffer.store_episode`; `.numpy()` gives the four arrays `collect_episodes` returns.
        `stats_out`: a list that receives ONE device tensor [n_rollouts, 6] per call, the metrics of this call's episodes
        (`DeviceEpisodes.stats` at `vec_env.distance_threshold`: one more small launch behind the rollout, in any of the three
        forms, no host wait); with None nothing more is launched."""
        from .device_env import DeviceEpisodes, binomial1_qn, fused_rollout_reason
        vec_env = vec_env or self.vec_env
        n_total = int(n_rollouts or vec_env.n_envs)
        eps = self._rollouts.get(n_total)
        if eps is None:
            eps = self._rollouts[n_total] = DeviceEpisodes(self.ctx, self.buffer._dev, n_total)
        qn = binomial1_qn(self.args.random_eps)[0] if explore else 1.0
        clip_abs = 0.15 if epoch >= 100 else 0.0                                  # ddpg_agent.py:118-119
        self._flush_updates()
        streams = self.explore_streams
        if streams is not None and len(streams) != vec_env.n_envs:
            raise ValueError(f"collect_episodes_device: {len(streams)} exploration streams for {vec_env.n_envs} environments")
        self.rollout_reason = fused_rollout_reason(getattr(vec_env, "is_native_device_env", False), self._slab_shaped(), explore,
                                                   streams is not None)
        self.rollout_form = 'fused' if self.rollout_reason is None else 'stepped'
        self.rollout_launches = 0 if self.rollout_form == 'fused' else None
        # what every entry takes behind its handles: the explore flag, the constants of _select_actions, the clip
        how = (1 if explore else 0, float(self.args.noise_eps), float(self.args.random_eps), qn, clip_abs)
        if self.rollout_form == 'fused' and getattr(vec_env, "reset_streams", None) is not None:
            success = self._collect_all_waves(vec_env, eps, n_total, streams, how)
            if success_out is not None:
                success_out.append(success)
            if stats_out is not None:
                stats_out.append(eps.stats(vec_env.distance_threshold, 0, n_total))
            return eps
        done = 0
        while done < n_total:
            k = min(vec_env.n_envs, n_total - done)
            o = vec_env.reset() if k == vec_env.n_envs else vec_env.reset(k)
            if self.rollout_form == 'fused':
                success = self._collect_wave_fused(vec_env, eps, done, k, streams, how)
            else:
                success = self._collect_wave_stepped(vec_env, eps, done, k, o, streams, how)
            if success_out is not None:
                success_out.append(success)
            done += k
        if explore and streams is None:     # (the streams keep no host copy of their cached normals: nothing to invalidate)
            self.rng.mark_normals_drawn()
        if stats_out is not None:
            stats_out.append(eps.stats(vec_env.distance_threshold, 0, n_total))
        return eps

    def _collect_all_waves(self, vec_env, eps, n_total, streams, how):
        """All `n_total` episodes as one launch (hp_rollout_waves), or the few the launch cap dictates; the environments are
        reset inside it.  Returns the n_total success flags."""
        env = vec_env.env_desc()
        success = torch.empty(n_total, dtype=torch.float32, device=vec_env.device)
        launches = C.c_int32()
        with self.ctx.torch_bridge():
            _lib.check(self.lib.hp_rollout_begin(eps.h, 0, n_total))
            _lib.check(self.lib.hp_rollout_waves(eps.h, self.h, self.o_norm.h, self.g_norm.h,
                                                 streams.h if streams is not None else None, vec_env.reset_streams.h,
                                                 C.byref(env), vec_env.n_envs, *how, C.c_void_p(success.data_ptr()),
                                                 C.byref(launches)))
        self.rollout_launches = int(launches.value)
        vec_env.active = (n_total - 1) % vec_env.n_envs + 1      # the environments of the last wave
        return success

    def _collect_wave_fused(self, vec_env, eps, first, k, streams, how):
        """Episodes [first, first + k) out of the k environments just reset, as one launch (hp_rollout_episodes).  Returns their
        success flags."""
        env = vec_env.env_desc()
        success = torch.empty(k, dtype=torch.float32, device=vec_env.device)
        with self.ctx.torch_bridge():
            _lib.check(self.lib.hp_rollout_begin(eps.h, first, k))
            _lib.check(self.lib.hp_rollout_episodes(eps.h, self.h, self.o_norm.h, self.g_norm.h,
                                                    streams.h if streams is not None else None, C.byref(env), *how,
                                                    C.c_void_p(success.data_ptr())))
        self.rollout_launches += 1
        return success

    def _collect_wave_stepped(self, vec_env, eps, first, k, o, streams, how):
        """Episodes [first, first + k) out of the k environments just reset (`o`: what the reset returned), two launches per
        timestep around `vec_env.step` and one closing record.  Returns the success flags of the last step."""
        p = lambda t: C.c_void_p(t.data_ptr())
        step, stream_h = ((self.lib.hp_rollout_step_streams, streams.h) if streams is not None
                          else (self.lib.hp_rollout_step, self.rng.h))
        actions = torch.empty((k, int(self.env_params['action'])), dtype=torch.float32, device=o['observation'].device)
        with self.ctx.torch_bridge():       # the whole wave in torch's stream order, between the environment's own kernels
            _lib.check(self.lib.hp_rollout_begin(eps.h, first, k))
            for t in range(int(self.env_params['max_timesteps'])):
                obs, ag, g = (o[key].contiguous() for key in ('observation', 'achieved_goal', 'desired_goal'))
                _lib.check(step(eps.h, self.h, self.o_norm.h, self.g_norm.h, stream_h, t, p(obs), p(ag), p(g), *how, p(actions)))
                o, _, _, info = vec_env.step(actions)
            obs, ag = o['observation'].contiguous(), o['achieved_goal'].contiguous()
            _lib.check(self.lib.hp_rollout_finish(eps.h, p(obs), p(ag)))
        return info['is_success']

    def _slab_shaped(self):
        """Whether policy calls on this agent are the one-launch slab kernel (hp_agent_engine reports the 4x4x1 slab engine)."""
        if self._slab8 is None:
            e = C.c_int32()
            _lib.check(self.lib.hp_agent_engine(self.h, C.byref(e), None, None))
            self._slab8 = e.value == 8
        return self._slab8

    def _select_actions(self, pi):
        """ddpg_agent.py:174-184: Gaussian noise, clip, epsilon-random (numpy global RNG, like the reference).  `action`
        stays the float32 array the policy returned and is updated in place, so every step rounds to float32 exactly
        where the reference's `action += ...` does."""
        amax = self.env_params['action_max']
        action = (pi.cpu().numpy() if isinstance(pi, torch.Tensor) else np.array(pi, dtype=np.float32)).squeeze()
        action += self.args.noise_eps * amax * np.random.randn(*action.shape)
        action = np.clip(action, -amax, amax)
        random_actions = np.random.uniform(low=-amax, high=amax, size=self.env_params['action'])
        action += np.random.binomial(1, self.args.random_eps, 1)[0] * (random_actions - action)
        return action

    def collect_episodes(self, n_rollouts, epoch=0, explore=True):
        """Rollout half of learn() (:101-137) for `n_rollouts` episodes; returns the four episode arrays.  The
        environments in self.envs are stepped in lockstep, one batched policy call per timestep (`lockstep_episodes`); with a
        single environment this is the reference's loop, including the order of its draws from numpy's global stream."""
        def to_action(row):
            action = self._select_actions(row) if explore else row.astype(np.float64)
            return np.clip(action, -0.15, 0.15) if epoch >= 100 else action      # ddpg_agent.py:118-119

        return lockstep_episodes(self.envs, n_rollouts, int(self.env_params['max_timesteps']), self.act, to_action)[0]

    def _eval_agent(self):
        """ddpg_agent.py:280-304: success at the last step of n_test_rollouts noise-free episodes, averaged over ranks;
        the environments in self.envs run in lockstep with one batched policy call per timestep (`lockstep_episodes`)."""
        if self.vec_env is not None:
            return self._eval_agent_device()
        batch, wins = lockstep_episodes(self.envs, int(self.args.n_test_rollouts), int(self.env_params['max_timesteps']),
                                        self.act, lambda row: row, follow_goal=True)
        rate = self._success_rate(wins)
        thr = self.env.distance_threshold if hasattr(self.env, "distance_threshold") else self._arg("distance_threshold")
        if self._arg("eval_metrics"):       # args.eval_metrics: from the achieved goals [T + 1] and desired goals [T] of every episode
            from .synthetic import episode_stats, episode_stats_summary
            self._record_eval_metrics(episode_stats_summary(episode_stats(batch[1], batch[2], thr)[0]))
        if self._arg("eval_critic"):        # args.eval_critic: observations [T + 1] and actions [T] beside them
            from .synthetic import episode_critic_summary
            self._record_eval_critic(episode_critic_summary(self.episode_critic_stats_host(batch, thr)[0]))
        return rate

    def _eval_agent_device(self):
        """_eval_agent on the device path: noise-free lockstep rollouts, the success flags of each wave's last step gathered on
        the device and copied to the host once at the end."""
        flags, remaining = [], int(self.args.n_test_rollouts)
        stats = [] if self._arg("eval_metrics") else None
        critic = [] if self._arg("eval_critic") else None
        while remaining > 0:
            # one call per wave; with reset on the device one call for all of them (one launch: hp_rollout_waves)
            k = remaining if getattr(self.vec_env, "reset_streams", None) is not None else min(self.vec_env.n_envs, remaining)
            eps = self.collect_episodes_device(n_rollouts=k, explore=False, success_out=flags, stats_out=stats)
            if critic is not None:       # args.eval_critic: two more launches behind the call, before the next one rewrites the block
                critic.append(self.episode_critic_stats(eps, first=0, n=k)[0])
            remaining -= k
        wins = torch.cat([f.reshape(-1).to(torch.float64) for f in flags])
        if stats is None and critic is None:
            return self._success_rate(wins.cpu().numpy())
        # args.eval_metrics / args.eval_critic: the summaries of all evaluation episodes (hp_episode_stats_summary,
        # hp_episode_critic_summary) ride behind the flags in the one copy to the host; what is done with the flags is unchanged
        riders = [self._column_means(entry, rows[0] if len(rows) == 1 else torch.cat(rows))
                  for rows, entry in ((stats, self.lib.hp_episode_stats_summary), (critic, self.lib.hp_episode_critic_summary))
                  if rows is not None]
        both, n_wins = torch.cat([wins, *riders]).cpu().numpy(), wins.numel()
        rate = self._success_rate(both[:n_wins])
        if stats is not None:
            self._record_eval_metrics(both[n_wins:n_wins + _lib.EPISODE_SUMMARY])
        if critic is not None:
            self._record_eval_critic(both[-_lib.CRITIC_STATS:])
        return rate

    def _success_rate(self, wins):
        """The mean of this rank's success flags, averaged over the ranks"""
        local = torch.tensor([float(np.mean(wins))], dtype=torch.float64)
        if self.comm.world_size > 1:
            local = local.to(f"cuda:{self.ctx.device_id}")
        self.comm.allreduce_mean_(local)
        return float(local.item())
