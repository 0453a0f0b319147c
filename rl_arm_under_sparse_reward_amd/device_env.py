"""Rollouts collected on the device, for simulators whose state already lives there.

**Vectorised device GoalEnv protocol.**  `ddpg_agent` takes, in place of a gym-GoalEnv-like object, one object `env` with

    env.is_device_vec_env == True
    env.n_envs, env.env_params, env.distance_threshold, env.reward_type
    env.reset()              -> {'observation': [n, obs], 'achieved_goal': [n, goal], 'desired_goal': [n, goal]}
    env.step(actions_f32)    -> (obs_dict, reward, done, {'is_success': tensor[n]})

where every array is a contiguous float64 torch tensor on the context's device and `actions_f32` is the float32 tensor
[n, action] the library wrote.  The environment runs on torch's current stream; the library enqueues its own kernels of a rollout
wave on that same stream (`Context.torch_bridge`, hp_ctx_borrow_stream) and orders its own stream behind it when the learner next
runs -- events on the device, never a host wait.  The tensors an environment returns must stay valid until the next `step` /
`reset` call (the library reads them in stream order and keeps no reference).

With such an environment `ddpg_agent.collect_episodes_device` runs T timesteps of two launches each (csrc/rollout.hip) with no
host copy in between, the exploration noise of ddpg_agent.py:174-184 drawn on the device from the reference's MT19937 stream, and
returns a `DeviceEpisodes` handle that `train_cycle` / `buffer.store_episode` consume without the episodes ever visiting the host.

**Native environments.**  An environment whose dynamics the library evaluates itself (csrc/env_device.h) additionally has

    env.is_native_device_env == True
    env.native_desc()        -> {'kind': int, 'params': [float, ...], 'state': [tensor, ...]}     (hp_env_desc)

and a whole wave of its episodes is ONE launch (hp_rollout_episodes: every workgroup loops over the T timesteps of its four rows)
whenever `fused_rollout_reason` finds nothing against it; `reset` stays on the host, `step` stays available, and after a fused
wave the state tensors hold what T `step` calls would have left.  `NativePointMassVecEnv` is the first such environment and
`NativePushBlockVecEnv` the second: a kinematic planar push whose achieved goal is a block that moves only on contact, and whose
reset is a rejection loop (a data-dependent number of draws).  `env.state_names` lists the attributes that hold the state tensors,
in the order of `native_desc()['state']`.

**Reset on the device** (opt-in: `env.enable_device_reset()`, `args.device_reset`).  The environment's reset generators move into
one device stream per environment (`env.reset_streams`, a `random.DeviceRandomStreams` holding the very states of `env.rs`), and
`reset(k)` becomes one launch (hp_env_reset) with no host loop, no upload and no host wait.  `collect_episodes_device` then
issues ALL waves of a call as one launch (hp_rollout_waves: the kernel resets an environment between two of its episodes), or the
few launches `_lib.ROLLOUT_MAX_LAUNCH_TIMESTEPS` dictates; `agent.rollout_launches` says how many.  Same bits as the host reset.

Draw order with n environments: per timestep, for env i = 0 .. n-1: randn(action), uniform(action), binomial(1) -- the order of
the host lockstep path (`collect_episodes` on a list of environments); with one environment it is the reference's own order.

**Demonstrations.**  `generate_demos(vec_env, n_demos)` runs the reference's scripted push controller
(`synthetic.scripted_action`, get_demo_data_push.py:39-61) on a native environment that is reset on the device and keeps the
successful episodes in order -- whole episodes, all waves of a round in one launch (hp_demo_episodes), the filter one more
(hp_demo_compact), no policy and no weights; `synthetic.scripted_demos` on host twins seeded alike gives the same bits.

With a `synthetic.PickScript` the controller is the reference's pick-and-place schedule (`synthetic.pick_scripted_action`,
get_demo_data_pick.py:54-67; hp_demo_episodes_pick); `script=None` takes the environment's own `default_demo_script()`.

`NativePickPlaceVecEnv` is the third native environment: a kinematic pick-and-place whose fourth action component moves the
fingers, whose block is grasped by closing open fingers around it and never released, and whose reset is the rejection loop in
three dimensions.

`PointMassVecEnv` is the tensor twin of `synthetic.PointMassGoalEnv`, `PushBlockVecEnv` that of `synthetic.PushBlockGoalEnv`,
`PickPlaceVecEnv` that of `synthetic.PickPlaceGoalEnv`; what
they share (`_GoalVecEnv`) includes the rule that an environment works on the first `active` rows of its state tensors, and the
two gripper-and-block twins share their state, reset and observation columns one level below it (`_GripBlockVecEnv`).  A native
class is one of them behind `_NativeEnv` -- descriptor, device reset -- plus the constant of its kind.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .synthetic import (DemoScript, rejection_reset, write_demo_npz_from, push_separated, PUSH_RESET_ATTEMPTS, PUSH_RESET_BOUNDS, PUSH_START_Z,
                        PUSH_X_HI, PUSH_X_LO, PUSH_Y_HI, PUSH_Y_LO, PUSH_Z_HI)
from .synthetic import (PickScript, pick_separated, PICK_FINGER_MAX, PICK_GRASP_WIDTH, PICK_RESET_ATTEMPTS, PICK_RESET_BOUNDS, PICK_START_Z,
                        PICK_TOOL, PICK_X_HI, PICK_X_LO, PICK_Y_HI, PICK_Y_LO, PICK_Z_HI)


def wave_layout(n_envs, T, obs, goal, act):
    """Offsets (float64 elements) of obs | ag | g | actions inside a wave block and its length: the staging layout of the host
    feeder (feeder._Layout), which is what hp_rollout_create allocates."""
    o_ag = n_envs * (T + 1) * obs
    o_g = o_ag + n_envs * (T + 1) * goal
    o_act = o_g + n_envs * T * goal
    return {"obs": 0, "ag": o_ag, "g": o_g, "actions": o_act, "elems": o_act + n_envs * T * act}


def binomial1_qn(p):
    """(qn, reflected) of numpy's legacy binomial(1, p): the inversion runs on p' = p for p <= 0.5 and on p' = 1 - p otherwise
    (the result is then 1 - X); qn = exp(1 * log(1 - p')) is computed here once, by the host's libm like numpy's own."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError("p < 0, p > 1 or p is NaN")
    reflected = not (p <= 0.5)
    pe = 1.0 - p if reflected else p
    return math.exp(math.log(1.0 - pe)), reflected


def fused_rollout_reason(env_native, agent_slab, explore, has_streams):
    """Why a wave cannot be collected by the one-launch form (hp_rollout_episodes), or None when it can.  The single shared
    stream with explore=True stays per-step: its walk visits the environments one after the other by definition."""
    if not env_native:
        return "the environment is not native: its dynamics run in torch, one launch boundary per timestep"
    if not agent_slab:       # the rule is require_slab_shaped's (csrc/policy_call.h); this sentence restates it
        return "the agent is not slab-shaped (hidden 256, padded input width <= 48, at most 4 action components)"
    if explore and not has_streams:
        return "exploring from the single shared stream is a sequential walk across the environments (enable_explore_streams)"
    return None


class DeviceEpisodes:
    """Episodes collected by `collect_episodes_device`: a device block [obs | ag | g | actions] of `n` episodes (hp_rollout).
    `.numpy()` copies the four arrays `collect_episodes` returns to the host (synchronises).  The block belongs to the agent and
    is rewritten by its next `collect_episodes_device` call for the same number of episodes."""

    def __init__(self, ctx, buffer_dev, n):
        self.ctx, self.lib, self.n = ctx, ctx.lib, int(n)
        self.T, self.dims = buffer_dev.T, dict(buffer_dev.dims)
        self.h = C.c_void_p()
        _lib.check(self.lib.hp_rollout_create(ctx.h, buffer_dev.h, self.n, C.byref(self.h)))
        p = C.c_void_p()
        _lib.check(self.lib.hp_rollout_block(self.h, C.byref(p), None, None, None))
        self.block = p.value

    def __len__(self):
        return self.n

    def numpy(self):
        n, T, d = self.n, self.T, self.dims
        out = [np.empty((n, T + 1, d["obs"])), np.empty((n, T + 1, d["ag"])), np.empty((n, T, d["g"])),
               np.empty((n, T, d["actions"]))]
        for which, a in enumerate(out):
            _lib.check(self.lib.hp_rollout_read(self.h, which, _lib.ptr(a, C.c_double)))
        return out

    def stats(self, distance_threshold, first=0, n=None, step_success=False):
        """The metrics of episodes [first, first + n) (default: all of them behind `first`), computed where they lie
        (hp_episode_stats_block): a float64 device tensor [n, 6] in the columns of `synthetic.EPISODE_STATS` -- and, with
        `step_success=True`, the float32 flags [n, T] of every step beside it.  One launch on torch's current stream; no copy and
        no synchronisation.  `synthetic.episode_stats` on `.numpy()` gives the same bits."""
        first = int(first)
        n = self.n - first if n is None else int(n)
        dev = torch.device("cuda", self.ctx.device_id)
        stats = torch.empty((max(n, 0), _lib.EPISODE_STATS), dtype=torch.float64, device=dev)
        flags = torch.empty((max(n, 0), self.T), dtype=torch.float32, device=dev) if step_success else None
        with self.ctx.torch_bridge():
            _lib.check(self.lib.hp_episode_stats_block(self.h, first, n, float(distance_threshold), C.c_void_p(stats.data_ptr()),
                                                       C.c_void_p(flags.data_ptr()) if step_success else None))
        return (stats, flags) if step_success else stats

    def returns(self, distance_threshold, gamma, reward_type="sparse", tail="persist", first=0, n=None, q=None):
        """The discounted return every step of episodes [first, first + n) went on to collect, computed where they lie
        (hp_episode_returns_block): a float64 device tensor [n, T].  `reward_type` 'sparse' | 'dense' is compute_reward's; `tail`
        'persist' holds the last step's reward for ever (G_T = r_{T-1} / (1 - gamma), what an infinite-horizon critic is trained
        towards), 'zero' ends the sum with the episode.  With `q` (a float32 device tensor [n, T], `ddpg_agent.episode_q`) the
        same launch also fills the critic columns: returns (returns, stats [n, 6] in the columns of `synthetic.CRITIC_STATS`).
        One launch on torch's current stream; no copy and no synchronisation.  `synthetic.episode_returns` /
        `episode_critic_stats` on `.numpy()` give the same bits."""
        from .synthetic import _reward_kind, _tail_kind
        first = int(first)
        n = self.n - first if n is None else int(n)
        dev = torch.device("cuda", self.ctx.device_id)
        out = torch.empty((max(n, 0), self.T), dtype=torch.float64, device=dev)
        stats = None
        if q is not None:
            if q.dtype != torch.float32 or tuple(q.shape) != tuple(out.shape) or not q.is_contiguous() or q.device != out.device:
                raise ValueError(f"DeviceEpisodes.returns: q must be a contiguous float32 device tensor [{max(n, 0)}, {self.T}]")
            stats = torch.empty((max(n, 0), _lib.CRITIC_STATS), dtype=torch.float64, device=dev)
        with self.ctx.torch_bridge():
            _lib.check(self.lib.hp_episode_returns_block(self.h, first, n, float(distance_threshold), _reward_kind(reward_type),
                                                         float(gamma), _tail_kind(tail), C.c_void_p(out.data_ptr()),
                                                         C.c_void_p(q.data_ptr()) if q is not None else None,
                                                         C.c_void_p(stats.data_ptr()) if q is not None else None))
        return out if q is None else (out, stats)

    def __del__(self):
        try:
            self.lib.hp_rollout_destroy(self.h)
        except Exception:
            pass


class _GoalVecEnv:
    """What the vectorised environments share: n environments as float64 tensors, env i reset from RandomState(seed + i) on the
    host; `reset`, `step` and `_observation` of a subclass work on the first `active` rows of its state tensors, in place -- all
    of them unless the tensors were widened to n_envs rows for good (`_NativeEnv.enable_device_reset`).  A subclass has
    `state_names`, the attributes that hold the state tensors (`goal` among them), and `_observation()`."""

    is_device_vec_env = True

    def __init__(self, n_envs, seed, device, max_timesteps, distance_threshold, reward_type, step_scale):
        self.n_envs = int(n_envs)
        self.device = torch.device(device)
        self.rs = [np.random.RandomState(seed + i) for i in range(self.n_envs)]
        self.max_timesteps = int(max_timesteps)
        self.distance_threshold = float(distance_threshold)
        self.reward_type = reward_type
        self.step_scale = float(step_scale)
        self.active = self.n_envs

    @property
    def env_params(self):
        return {'obs': 27, 'goal': 3, 'action': 4, 'action_max': 0.5, 'max_timesteps': self.max_timesteps}

    def _n_active(self, n_active):
        """The `n_active` of a reset (default: all environments), validated"""
        k = self.n_envs if n_active is None else int(n_active)
        if not 0 < k <= self.n_envs:
            raise ValueError("n_active outside [1, n_envs]")
        return k

    def _rows(self, *names):
        """The first `active` rows of the named state tensors -- the tensors themselves where that is all their rows, which
        spares the per-step path (host-bound: a dozen small kernels per timestep) one slice per tensor and call"""
        k = self.active
        return [t if t.shape[0] == k else t[:k] for t in (getattr(self, name) for name in names)]

    def _distance(self, a, b):
        d = a - b
        # numpy's norm over three components: a left-to-right sum of squares, then the square root
        return torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])

    def compute_reward(self, achieved_goal, goal, info):
        """Tensors in, tensors out; numpy arrays (what her_sampler probes a reward function with) take the host environment's
        own arithmetic."""
        if not torch.is_tensor(achieved_goal):
            d = np.linalg.norm(np.asarray(achieved_goal) - np.asarray(goal), axis=-1)
            return -(d > self.distance_threshold).astype(np.float32) if self.reward_type == 'sparse' else -d
        d = self._distance(achieved_goal, goal)
        if self.reward_type == 'sparse':
            return -(d > self.distance_threshold).to(torch.float32)
        return -d

    def _stepped(self):
        """What `step` returns, out of the state it has just written"""
        goal, = self._rows("goal")
        observation = self._observation()
        success = (self._distance(observation['achieved_goal'], goal) < self.distance_threshold).to(torch.float32)
        info = {'is_success': success}
        return observation, self.compute_reward(observation['achieved_goal'], goal, info), False, info


class PointMassVecEnv(_GoalVecEnv):
    """n `synthetic.PointMassGoalEnv`s as tensors: env i resets from RandomState(seed + i) on the host (one upload per episode),
    `step` is elementwise float64 torch -- multiply and add as separate ops, so the bits are the host environment's.  State:
    `pos`, `vel`, `goal` [rows, 3].  Works with device="cpu" too."""

    state_names = ("pos", "vel", "goal")     # the attributes that hold the state tensors

    def __init__(self, n_envs, seed=0, device="cuda", max_timesteps=100, distance_threshold=0.05, reward_type='sparse',
                 step_scale=0.1):
        super().__init__(n_envs, seed, device, max_timesteps, distance_threshold, reward_type, step_scale)
        z = torch.zeros((self.n_envs, 3), dtype=torch.float64, device=self.device)
        self.pos, self.vel, self.goal = z, z.clone(), z.clone()

    def params(self):
        """hp_env_desc.params of the kind"""
        return [self.step_scale, self.distance_threshold]

    def _observation(self):
        pos, vel, goal = self._rows("pos", "vel", "goal")
        obs = torch.zeros((self.active, 27), dtype=torch.float64, device=self.device)
        obs[:, 0:3] = pos
        obs[:, 3:6] = vel
        obs[:, 12:15] = pos
        return {'observation': obs, 'achieved_goal': pos.clone(), 'desired_goal': goal.clone()}

    def reset(self, n_active=None):
        """Reset the first `n_active` environments (default: all) -- only those draw from their streams, like the host lockstep
        path, which resets only the environments of the wave -- and step those from now on."""
        k = self._n_active(n_active)
        both = np.empty((2, k, 3))
        for i in range(k):
            both[0, i] = self.rs[i].uniform(0.0, 0.5, 3)
            both[1, i] = self.rs[i].uniform(0.0, 0.5, 3)
        dev = torch.from_numpy(both).to(self.device)
        self.pos, self.goal = dev[0].contiguous(), dev[1].contiguous()
        self.vel = torch.zeros_like(self.pos)
        self.active = k
        return self._observation()

    def step(self, actions):
        pos, vel = self._rows("pos", "vel")
        a = torch.clamp(actions.to(torch.float64), -0.5, 0.5)
        scaled = self.step_scale * a[:, :3]                 # multiply, then add: two roundings, like numpy
        new = torch.clamp(pos + scaled, 0.0, 0.5)
        torch.sub(new, pos, out=vel)                        # vel = new - pos, then pos = new: written into the rows
        pos.copy_(new)
        return self._stepped()


class _GripBlockVecEnv(_GoalVecEnv):
    """What the tensor twins of the two gripper-and-block tasks share: the constructor arguments of the table, the state tensors
    `grip`, `blk`, `goal` [rows, 3] and a fourth one -- named by `state_names[3]`, `_aux_width` columns, the gripper's and the
    block's velocity in its first six -- the rejection reset on the host with its upload, and the observation's common columns.
    A subclass has `_reset = (bounds, attempts, separated, gripper start z)`, `params()` and `step`."""

    def __init__(self, n_envs, seed, device, max_timesteps, distance_threshold, reward_type, step_scale, half_width, min_separation,
                 table_z, grip_start):
        super().__init__(n_envs, seed, device, max_timesteps, distance_threshold, reward_type, step_scale)
        self.half_width = float(half_width)
        self.min_separation, self.table_z = float(min_separation), float(table_z)
        self.grip_start = (float(grip_start[0]), float(grip_start[1]))
        self.reset_attempts = [0] * self.n_envs      # attempts the last host reset of each environment took
        z = torch.zeros((self.n_envs, 3), dtype=torch.float64, device=self.device)
        self.grip, self.blk, self.goal = z, z.clone(), z.clone()
        setattr(self, self.state_names[3], torch.zeros((self.n_envs, self._aux_width), dtype=torch.float64, device=self.device))

    @property
    def pos(self):
        """The gripper's position (nothing in the package reads it)."""
        return self.grip

    def _observation(self):
        k = self.active
        grip, blk, vel = self.grip[:k], self.blk[:k], getattr(self, self.state_names[3])[:k]
        obs = torch.zeros((k, 27), dtype=torch.float64, device=self.device)
        obs[:, 0:3] = grip
        obs[:, 6:9] = vel[:, 0:3]
        obs[:, 12:15] = blk
        obs[:, 18:21] = blk - grip
        obs[:, 21:24] = vel[:, 3:6]
        return {'observation': obs, 'achieved_goal': blk.clone(), 'desired_goal': self.goal[:k].clone()}

    def reset(self, n_active=None):
        """Reset the first `n_active` environments (default: all): only those draw from their streams."""
        k = self._n_active(n_active)
        bounds, attempts, separated, start_z = self._reset
        fresh = np.empty((3, k, 3))
        for i in range(k):
            u, self.reset_attempts[i] = rejection_reset(self.rs[i], bounds, attempts, lambda *u: separated(self, *u))
            fresh[0, i] = (self.grip_start[0], self.grip_start[1], start_z)
            fresh[1, i] = (u[0], u[1], self.table_z)
            fresh[2, i] = (u[2], u[3], u[4] if len(u) > 4 else self.table_z)     # a fifth draw is the goal's height
        dev = torch.from_numpy(fresh).to(self.device)
        self.grip, self.blk, self.goal = dev[0].contiguous(), dev[1].contiguous(), dev[2].contiguous()
        setattr(self, self.state_names[3], torch.zeros((k, self._aux_width), dtype=torch.float64, device=self.device))
        self.active = k
        return self._observation()


class PushBlockVecEnv(_GripBlockVecEnv):
    """n `synthetic.PushBlockGoalEnv`s as tensors: env i resets from RandomState(seed + i) on the host -- the same rejection loop,
    four scalars per attempt -- and `step` is the host environment's operations elementwise in float64, one torch op per
    rounding, `torch.where` for its branches.  State: `grip`, `blk`, `goal` [rows, 3] and `vel` [rows, 6] (gripper, then block).
    Works with device="cpu" too."""

    state_names, _aux_width = ("grip", "blk", "goal", "vel"), 6
    _reset = (PUSH_RESET_BOUNDS, PUSH_RESET_ATTEMPTS, push_separated, PUSH_START_Z)

    def __init__(self, n_envs, seed=0, device="cuda", max_timesteps=100, distance_threshold=0.05, reward_type='sparse',
                 step_scale=0.1, half_width=0.04, z_touch=0.25, min_separation=0.15, table_z=0.2, grip_start=(0.25, 0.1)):
        super().__init__(n_envs, seed, device, max_timesteps, distance_threshold, reward_type, step_scale, half_width, min_separation,
                         table_z, grip_start)
        self.z_touch = float(z_touch)

    def params(self):
        """hp_env_desc.params of the kind"""
        return [self.step_scale, self.distance_threshold, self.half_width, self.z_touch, self.min_separation, self.table_z,
                self.grip_start[0], self.grip_start[1]]

    def step(self, actions):
        k, r = self.active, self.half_width
        grip, blk = self.grip[:k], self.blk[:k]
        lo = torch.tensor([PUSH_X_LO, PUSH_Y_LO, self.table_z], dtype=torch.float64, device=self.device)
        hi = torch.tensor([PUSH_X_HI, PUSH_Y_HI, PUSH_Z_HI], dtype=torch.float64, device=self.device)
        a = torch.clamp(actions.to(torch.float64), -0.5, 0.5)
        scaled = self.step_scale * a[:, :3]                 # multiply, then add: two roundings, like numpy
        new = torch.minimum(torch.maximum(grip + scaled, lo), hi)
        gvel = new - grip
        dx, dy = blk[:, 0] - new[:, 0], blk[:, 1] - new[:, 1]
        adx, ady = dx.abs(), dy.abs()
        contact = (new[:, 2] < self.z_touch) & (adx < r) & (ady < r)
        along_x = (r - adx) <= (r - ady)                    # the axis of least penetration
        plus, minus = torch.full_like(dx, r), torch.full_like(dx, -r)
        bx = torch.where(contact & along_x, new[:, 0] + torch.where(dx >= 0, plus, minus), blk[:, 0])
        by = torch.where(contact & ~along_x, new[:, 1] + torch.where(dy >= 0, plus, minus), blk[:, 1])
        bx = torch.where(contact, torch.clamp(bx, PUSH_X_LO, PUSH_X_HI), bx)
        by = torch.where(contact, torch.clamp(by, PUSH_Y_LO, PUSH_Y_HI), by)
        moved = torch.stack([bx, by, blk[:, 2]], dim=1)
        bvel = moved - blk
        self.grip[:k], self.blk[:k] = new, moved
        self.vel[:k, 0:3], self.vel[:k, 3:6] = gvel, bvel
        return self._stepped()


class PickPlaceVecEnv(_GripBlockVecEnv):
    """n `synthetic.PickPlaceGoalEnv`s as tensors: env i resets from RandomState(seed + i) on the host -- the same rejection loop,
    five scalars per attempt -- and `step` is the host environment's operations elementwise in float64, one torch op per
    rounding, `torch.where` for its branches.  State: `grip`, `blk`, `goal` [rows, 3] and `aux` [rows, 8] = gripper velocity,
    block velocity, finger opening, held (0.0 or 1.0).  Works with device="cpu" too."""

    state_names, _aux_width = ("grip", "blk", "goal", "aux"), 8
    _reset = (PICK_RESET_BOUNDS, PICK_RESET_ATTEMPTS, pick_separated, PICK_START_Z)

    def __init__(self, n_envs, seed=0, device="cuda", max_timesteps=100, distance_threshold=0.05, reward_type='sparse',
                 step_scale=0.2, half_width=0.04, finger_scale=0.05, min_separation=0.15, table_z=0.2, grip_start=(0.25, 0.1)):
        super().__init__(n_envs, seed, device, max_timesteps, distance_threshold, reward_type, step_scale, half_width, min_separation,
                         table_z, grip_start)
        self.finger_scale = float(finger_scale)

    def params(self):
        """hp_env_desc.params of the kind"""
        return [self.step_scale, self.distance_threshold, self.half_width, self.finger_scale, self.min_separation, self.table_z,
                self.grip_start[0], self.grip_start[1]]

    def _observation(self):
        o = super()._observation()
        o['observation'][:, 9:11] = self.aux[:self.active, 6:8]      # finger opening, held
        return o

    def _pads_inside(self, grip, blk):
        tool = torch.tensor(PICK_TOOL, dtype=torch.float64, device=self.device)
        return ((blk - (grip + tool)).abs() < self.half_width).all(dim=1)

    def step(self, actions):
        k = self.active
        grip, blk, aux = self.grip[:k], self.blk[:k], self.aux[:k]
        lo = torch.tensor([PICK_X_LO, PICK_Y_LO, self.table_z], dtype=torch.float64, device=self.device)
        hi = torch.tensor([PICK_X_HI, PICK_Y_HI, PICK_Z_HI], dtype=torch.float64, device=self.device)
        a = torch.clamp(actions.to(torch.float64), -0.5, 0.5)
        held, f_old = aux[:, 7] != 0, aux[:, 6]
        near = held | self._pads_inside(grip, blk)          # the finger lock, on the state before the move
        a3 = torch.where(near, torch.full_like(f_old, -1.0), a[:, 3])
        finger = torch.clamp(f_old + self.finger_scale * a3, 0.0, PICK_FINGER_MAX)
        scaled = self.step_scale * a[:, :3]                 # multiply, then add: two roundings, like numpy
        new = torch.minimum(torch.maximum(grip + scaled, lo), hi)
        gvel = new - grip
        carried = torch.minimum(torch.maximum(blk + gvel, lo), hi)
        moved = torch.where(held[:, None], carried, blk)
        grasp = ~held & self._pads_inside(new, blk) & (f_old > PICK_GRASP_WIDTH) & (finger <= PICK_GRASP_WIDTH)
        bvel = moved - blk
        self.aux[:k] = torch.cat([gvel, bvel, finger[:, None], (held | grasp).to(torch.float64)[:, None]], dim=1)
        self.grip[:k], self.blk[:k] = new, moved
        return self._stepped()


class _NativeEnv:
    """What the native environments share: the descriptor, and the switch to reset on the device.  Mixed in before a
    `_GoalVecEnv` that has `params()`; the subclass names the library's kind."""

    is_native_device_env = True
    kind = None              # _lib.ENV_*: the struct of csrc/env_device.h that evaluates the same float64 operations
    reset_streams = None     # random.DeviceRandomStreams after enable_device_reset(): reset stream i = the state of rs[i]

    default_demo_script = DemoScript   # the script type `generate_demos` runs here when the caller names none: the task's own

    def native_desc(self):
        """hp_env_desc of the environments stepped now: kind, `params()`, and the state tensors in the order of `state_names`
        (float64, made contiguous; a launch reads all of them and writes them in place).  They have `active` rows, or n_envs
        rows for good with device reset -- the environments stepped now are then their first `active` rows."""
        for name in self.state_names:
            setattr(self, name, getattr(self, name).contiguous())
        return {"kind": self.kind, "params": self.params(), "state": [getattr(self, name) for name in self.state_names]}

    def env_desc(self):
        """`native_desc()` as the library's struct (hp_env_desc)."""
        desc = self.native_desc()
        env = _lib.EnvDesc(kind=int(desc["kind"]))
        for i, v in enumerate(desc["params"]):
            env.params[i] = float(v)
        for i, t in enumerate(desc["state"]):
            env.state_dev[i] = t.data_ptr()
        return env

    def enable_device_reset(self, ctx=None):
        """Reset on the device from now on (hp_env_reset; inside the launch of hp_rollout_waves): reset stream i takes over the
        current state of `self.rs[i]`, so enabling it mid-run continues the same sequence -- on a fresh environment stream i is
        RandomState(seed + i) -- and the host generators are not advanced any more.  The state tensors become [n_envs, ...] for the
        life of the environment (the rows stepped now keep their values); `reset(k)`, `step` and `_observation` work on the
        first k rows.  `ctx`: the library context of the agent that collects from this environment (default: the default one)."""
        from .random import DeviceRandomStreams
        if self.device.type != "cuda":
            raise ValueError(f"enable_device_reset: the environment lives on device '{self.device}': a reset on the device needs "
                             "a GPU environment (device='cuda')")
        if self.reset_streams is not None:
            return self.reset_streams
        self.ctx = ctx or _lib.Context.default()
        streams = DeviceRandomStreams(self.n_envs, ctx=self.ctx)
        streams.set_states([r.get_state() for r in self.rs])
        for name in self.state_names:
            t = getattr(self, name)
            f = torch.zeros((self.n_envs,) + tuple(t.shape[1:]), dtype=torch.float64, device=self.device)
            f[:t.shape[0]] = t
            setattr(self, name, f)
        self.reset_streams = streams
        return streams

    def reset(self, n_active=None):
        """The host reset -- or, after `enable_device_reset`, one launch (hp_env_reset) on torch's current stream, in order with
        the environment's own kernels"""
        if self.reset_streams is None:
            return super().reset(n_active)
        k = self._n_active(n_active)
        env = self.env_desc()
        with self.ctx.torch_bridge():
            _lib.check(self.ctx.lib.hp_env_reset(self.ctx.h, C.byref(env), self.reset_streams.h, k))
        self.active = k
        return self._observation()


class NativePointMassVecEnv(_NativeEnv, PointMassVecEnv):
    """`PointMassVecEnv` whose dynamics the library also evaluates itself (PointMassEnvDev, csrc/env_device.h: the same float64
    operations, one by one): `collect_episodes_device` collects a wave of its episodes in one launch.  `step` is the parent's,
    so the per-step protocol works on it unchanged -- and with device="cpu" it is simply the parent."""

    kind = _lib.ENV_POINT_MASS


class NativePushBlockVecEnv(_NativeEnv, PushBlockVecEnv):
    """`PushBlockVecEnv` whose dynamics the library also evaluates itself (PushBlockEnvDev, csrc/env_device.h: the same float64
    operations, one by one): `collect_episodes_device` collects a wave of its episodes in one launch, and after
    `enable_device_reset()` the rejection loop of its reset runs on the device too -- every environment for as many attempts as its
    own draws ask for.  `step` is the parent's, so the per-step protocol works on it unchanged."""

    kind = _lib.ENV_PUSH_BLOCK


class NativePickPlaceVecEnv(_NativeEnv, PickPlaceVecEnv):
    """`PickPlaceVecEnv` whose dynamics the library also evaluates itself (PickPlaceEnvDev, csrc/env_device.h: the same float64
    operations, one by one): one launch per wave, the three-dimensional rejection loop of its reset on the device after
    `enable_device_reset()`, and the reference's pick-and-place schedule as its scripted controller.  `step` is the parent's, so
    the per-step protocol works on it unchanged."""

    kind = _lib.ENV_PICK_PLACE

    default_demo_script = PickScript


# ---- demonstrations from the scripted controller ---------------------------------------------------------------------------------
DEMO_ROUND_EPISODES = 2048       # episodes a round of generate_demos aims at by default (a block of 56 MB at T = 100)


def default_round_waves(n_demos, n_envs):
    """Waves per round of `generate_demos` when the caller names none: a rule of (n_demos, n_envs) alone.  A round should hold
    about twice the demonstrations asked for -- at the ten per cent or so of scripted push episodes that succeed, a handful of
    rounds -- but no more than DEMO_ROUND_EPISODES episodes, and at least one wave:
    clamp(ceil(2 n_demos / n_envs), 1, max(1, DEMO_ROUND_EPISODES // n_envs))."""
    n_demos, n_envs = int(n_demos), int(n_envs)
    return max(1, min(-(-2 * n_demos // n_envs), max(1, DEMO_ROUND_EPISODES // n_envs)))


# a script type's struct, and the fields both carry under the same names: the arrays, the scalars
_DEMO_SCRIPT_FIELDS = (_lib.DemoScriptDesc, ("phase_end", "lift", "waypoint"), ("behind", "stop_radius"))
_PICK_SCRIPT_FIELDS = (_lib.PickScriptDesc, ("phase_end", "lift", "approach", "grasp"), ("open",))


def script_desc(script=None):
    """`synthetic.DemoScript` (None: the reference's numbers) as the library's struct (hp_demo_script), or a
    `synthetic.PickScript` as its own (hp_pick_script)."""
    s = script or DemoScript()
    struct, arrays, scalars = _PICK_SCRIPT_FIELDS if isinstance(s, PickScript) else _DEMO_SCRIPT_FIELDS
    d = struct()
    for name in arrays:
        for i, v in enumerate(getattr(s, name)):
            getattr(d, name)[i] = v
    for name in scalars:
        setattr(d, name, getattr(s, name))
    return d


class DeviceDemos:
    """What `generate_demos` returns: `.episodes`, a `DeviceEpisodes` of the `.kept` successful episodes in order (None if none
    was kept) -- `buffer.store_episode` / `train_cycle` take it as it is; `.info`, their is_success flags after every step
    (float32 tensor [kept, T]); `.attempted`, the episodes run; `.launches`, the launches of hp_demo_episodes.  `.numpy()`
    copies (obs, ag, g, actions, info) to the host; `.save(path)` writes them in the reference's demo schema."""

    def __init__(self, episodes, info, kept, attempted, launches, shapes):
        self.episodes, self.info, self.kept, self.attempted, self.launches = episodes, info, kept, attempted, launches
        self._shapes = shapes

    def __len__(self):
        return self.kept

    def numpy(self):
        if self.episodes is None:
            return [np.empty((0,) + s, dtype=np.float32 if j == 4 else np.float64) for j, s in enumerate(self._shapes)]
        return [*self.episodes.numpy(), self.info.cpu().numpy()]

    def stats(self, distance_threshold, step_success=False):
        """`DeviceEpisodes.stats` of the kept episodes ([0, 6] and [0, T] when none was kept): how close the scripted
        controller came, when it first succeeded -- its `step_success` is `.info` computed again from the block."""
        if self.episodes is None:
            dev = self.info.device
            stats = torch.empty((0, _lib.EPISODE_STATS), dtype=torch.float64, device=dev)
            return (stats, torch.empty((0,) + self._shapes[4], dtype=torch.float32, device=dev)) if step_success else stats
        return self.episodes.stats(distance_threshold, 0, self.kept, step_success=step_success)

    def save(self, path):
        """A demo file in the schema of get_demo_data_push.py:91-94 (`synthetic.write_demo_npz_from`): it preloads through
        `ddpg_agent._init_demo_buffer` and through the reference's own."""
        obs, ag, g, actions, info = self.numpy()
        write_demo_npz_from(path, obs, ag, g, actions, info)


def generate_demos(vec_env, n_demos, round_waves=None, max_episodes=10000, script=None, ctx=None, *, launch_cap=None):
    """`n_demos` successful episodes of a scripted controller -- `script`: a `synthetic.DemoScript` (the push schedule,
    hp_demo_episodes) or a `synthetic.PickScript` (the pick-and-place schedule, hp_demo_episodes_pick); None: the environment's
    `default_demo_script()`, the reference's numbers for its task -- on the native environment `vec_env`, generated and filtered
    on the device: the device form of `synthetic.scripted_demos`, bit for bit what that returns for host twins in the states of
    `vec_env`'s reset streams.

    Rounds as there: a round attempts n_envs * round_waves episodes, cut to what `max_episodes` leaves (episode e = w * n_envs
    + i is environment i's w-th of the round, reset from reset stream i) as one launch of hp_demo_episodes -- or the few the
    launch cap dictates -- and hp_demo_compact appends its successes, in order, behind those kept so far; whole rounds until
    n_demos are kept or max_episodes attempted.  The result is a pure function of (environment parameters and reset-stream
    states, n_demos, round_waves, max_episodes, script).  `round_waves=None`: `default_round_waves(n_demos, n_envs)`.

    The count of kept episodes is read back ONCE PER ROUND (4 bytes, synchronising): generation is a one-off at start-up and
    the host has to know when to stop.  Nothing else visits the host.  Touches no exploration stream and no sampler stream; the
    environment's state tensors hold the last episode's final state afterwards, like after `collect_episodes_device`.

    Needs a native environment with `enable_device_reset()` done (ValueError otherwise).  Returns a `DeviceDemos`;
    `kept < n_demos` there says max_episodes ran out.  `launch_cap` (tests): the timesteps one launch may hold
    (hp_rollout_debug_set_launch_cap on the round's block) in place of `_lib.ROLLOUT_MAX_LAUNCH_TIMESTEPS`."""
    if not getattr(vec_env, "is_native_device_env", False):
        raise ValueError("generate_demos: the environment is not native (device_env.NativePointMassVecEnv, NativePushBlockVecEnv): "
                         "scripted episodes on the device need dynamics the library evaluates itself")
    if getattr(vec_env, "reset_streams", None) is None:
        raise ValueError("generate_demos: the environment is not reset on the device: call vec_env.enable_device_reset() first "
                         "(args.device_reset)")
    n_demos, max_episodes, n_envs = int(n_demos), int(max_episodes), int(vec_env.n_envs)
    if n_demos < 1:
        raise ValueError("generate_demos: n_demos must be positive")
    round_waves = default_round_waves(n_demos, n_envs) if round_waves is None else int(round_waves)
    if round_waves < 1:
        raise ValueError("generate_demos: round_waves must be positive")
    ctx = ctx or vec_env.ctx
    lib, dev = ctx.lib, vec_env.device
    from .replay_buffer import DeviceEpisodeBuffer
    p, T = vec_env.env_params, int(vec_env.max_timesteps)
    shape = DeviceEpisodeBuffer(1, T, p['obs'], p['goal'], p['action'], ctx=ctx)     # T and the dimensions of the blocks
    per_round = min(n_envs * round_waves, max(max_episodes, 1))
    src, dst = DeviceEpisodes(ctx, shape, per_round), DeviceEpisodes(ctx, shape, n_demos)
    if launch_cap is not None:
        _lib.check(lib.hp_rollout_debug_set_launch_cap(src.h, int(launch_cap)))
    success = torch.zeros(per_round, dtype=torch.float32, device=dev)
    step_success = torch.zeros((per_round, T), dtype=torch.float32, device=dev)
    info = torch.zeros((n_demos, T), dtype=torch.float32, device=dev)
    kept_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    if script is None and hasattr(vec_env, "default_demo_script"):
        script = vec_env.default_demo_script()
    sd, launches = script_desc(script), C.c_int32()
    demo_episodes = lib.hp_demo_episodes_pick if isinstance(sd, _lib.PickScriptDesc) else lib.hp_demo_episodes
    ptr = lambda t: C.c_void_p(t.data_ptr())
    kept = attempted = total_launches = 0
    while kept < n_demos and attempted < max_episodes:
        n = min(n_envs * round_waves, max_episodes - attempted)
        env = vec_env.env_desc()
        with ctx.torch_bridge():
            _lib.check(demo_episodes(ctx.h, C.byref(env), vec_env.reset_streams.h, C.byref(sd), n_envs, 0, n, T, src.h,
                                     ptr(success), ptr(step_success), C.byref(launches)))
            _lib.check(lib.hp_demo_compact(ctx.h, src.h, ptr(success), ptr(step_success), n, dst.h, ptr(info), n_demos, kept,
                                           ptr(kept_dev)))
        vec_env.active = (n - 1) % n_envs + 1                 # the environments of the round's last wave
        kept = int(kept_dev.item())                           # the one synchronising read of the round
        attempted += n
        total_launches += int(launches.value)
    shapes = ((T + 1, p['obs']), (T + 1, p['goal']), (T, p['goal']), (T, p['action']), (T,))
    if kept == n_demos:
        return DeviceDemos(dst, info, kept, attempted, total_launches, shapes)
    if kept == 0:
        return DeviceDemos(None, info[:0], 0, attempted, total_launches, shapes)
    # fewer than asked: a block of exactly `kept` episodes (what store_episode takes), by the filter with every flag set
    short, short_info = DeviceEpisodes(ctx, shape, kept), torch.zeros((kept, T), dtype=torch.float32, device=dev)
    ones = torch.ones(kept, dtype=torch.float32, device=dev)
    with ctx.torch_bridge():
        _lib.check(lib.hp_demo_compact(ctx.h, dst.h, ptr(ones), ptr(info), kept, short.h, ptr(short_info), kept, 0, ptr(kept_dev)))
    torch.cuda.current_stream(dev).synchronize()              # `dst` and `ones` go out of scope here
    return DeviceDemos(short, short_info, kept, attempted, total_launches, shapes)
