"""Seeded synthetic experience in the reference's episode layout (host-side, numpy only).

There is no PyBullet on the benchmark box, so bench.py, the tests and the golden
generator all draw episodes from here.  The recipe is the one BASELINE.md section 3
/ SURVEY.md section 8(d) fix for the headline metric:

    rs = RandomState(seed);  obs ~ U(-1,1) [N, T+1, 27];  ag = obs[:, :, 12:15]
    g  = one U(0,0.5)^3 goal per episode repeated over T;  actions ~ U(-0.5,0.5) [N, T, 4]

Shapes follow what ddpg_agent.py:138-143 hands to replay_buffer.store_episode:
obs [N,T+1,obs], ag [N,T+1,goal], g [N,T,goal], actions [N,T,action], all float64.

`mode="walk"` replaces the iid achieved goals by a slow random walk so that a useful
fraction of relabelled goals lands within the 0.05 success radius (exercises both
reward values and near-threshold distances in the parity tests).
"""
from __future__ import annotations

import math

import numpy as np

ENV_PARAMS = {"obs": 27, "goal": 3, "action": 4, "action_max": 0.5, "max_timesteps": 100}


def make_episodes(n_episodes, seed=1, T=100, obs_dim=27, goal_dim=3, act_dim=4, mode="iid"):
    rs = np.random.RandomState(seed)
    obs = rs.uniform(-1.0, 1.0, size=(n_episodes, T + 1, obs_dim))
    if mode == "walk":
        start = rs.uniform(0.0, 0.5, size=(n_episodes, 1, goal_dim))
        steps = rs.normal(0.0, 0.012, size=(n_episodes, T + 1, goal_dim))
        steps[:, 0, :] = 0.0
        obs[:, :, 12:12 + goal_dim] = start + np.cumsum(steps, axis=1)
    elif mode != "iid":
        raise ValueError("mode must be 'iid' or 'walk'")
    ag = obs[:, :, 12:12 + goal_dim].copy()
    goal = rs.uniform(0.0, 0.5, size=(n_episodes, 1, goal_dim))
    g = np.repeat(goal, T, axis=1)
    actions = rs.uniform(-0.5, 0.5, size=(n_episodes, T, act_dim))
    return [np.ascontiguousarray(obs), ag, np.ascontiguousarray(g), np.ascontiguousarray(actions)]


def episode_checksum(episode_batch) -> float:
    """Exact, platform-independent checksum of the float64 bit patterns (integer arithmetic only, so it
    cannot depend on BLAS/libm code paths); returned as a float64-representable integer < 2^53."""
    acc = 0
    for i, a in enumerate(episode_batch):
        u = np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64)
        w = (np.arange(u.size, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(i + 1)) | np.uint64(1)
        with np.errstate(over="ignore"):
            acc = (acc + int(np.sum(u * w, dtype=np.uint64))) & ((1 << 64) - 1)
    return float(acc >> 11)


def write_demo_npz(path, n_episodes=8, seed=7, T=100):
    """Write a demo file in the schema get_demo_data_push.py:91-94 produces
    (keys acs, obs, info, g, ag; `info` is an object array of per-step dicts)."""
    obs, ag, g, actions = make_episodes(n_episodes, seed=seed, T=T, mode="walk")
    info = np.empty((n_episodes, T), dtype=object)
    for e in range(n_episodes):
        for t in range(T):
            d = float(np.linalg.norm(ag[e, t + 1] - g[e, t]))
            info[e, t] = {"is_success": np.float32(d < 0.05)}
    np.savez_compressed(path, acs=actions, obs=obs, info=info, g=g, ag=ag)
    return obs, ag, g, actions


class _HostGoalEnv:
    """What the host environments share: the environment's own RandomState, the GoalEnv surface that does not depend on the
    task -- `env_params`, `compute_reward` vectorised over leading dims (bmirobot_env_push_F.py:84-90), `_is_success` (:243-245)
    -- and what `step` returns once the task has moved its state (:103-108).  A task has `goal`, `_observation()`, `reset()` and
    `step(action)`."""

    def __init__(self, seed, max_timesteps, distance_threshold, reward_type, step_scale):
        self.rs = np.random.RandomState(seed)
        self.max_timesteps = int(max_timesteps)
        self.distance_threshold = float(distance_threshold)
        self.reward_type = reward_type
        self.step_scale = float(step_scale)

    @property
    def env_params(self):
        return {'obs': 27, 'goal': 3, 'action': 4, 'action_max': 0.5, 'max_timesteps': self.max_timesteps}

    def compute_reward(self, achieved_goal, goal, info):
        diff = np.asarray(achieved_goal) - np.asarray(goal)
        d = np.linalg.norm(diff, axis=-1)
        if self.reward_type == 'sparse':
            return -(d > self.distance_threshold).astype(np.float32)
        return -d

    def _is_success(self, achieved_goal, desired_goal):
        return (np.linalg.norm(achieved_goal - desired_goal, axis=-1) < self.distance_threshold).astype(np.float32)

    def _stepped(self):
        """What `step` returns, out of the state it has just written"""
        observation = self._observation()
        info = {'is_success': self._is_success(observation['achieved_goal'], self.goal)}
        reward = self.compute_reward(observation['achieved_goal'], self.goal, info)
        return observation, reward, False, info


def rejection_reset(rs, bounds, attempts, accept):
    """The rejection loop of a reset (bmirobot_env_push_F.py:117-132): at most `attempts` times, one `rs.uniform(low, high)` per
    pair of `bounds`, in order, until `accept(*draws)`; the last attempt is kept either way.  Returns (draws, attempts taken).
    The host environments and the host reset of their tensor twins (device_env.py) draw through it."""
    for attempt in range(attempts):
        draws = tuple(rs.uniform(low, high) for low, high in bounds)
        if accept(*draws):
            break
    return draws, attempt + 1


class PointMassGoalEnv(_HostGoalEnv):
    """Stand-in for the PyBullet arm environments (the real ones need pybullet + gym, absent here): the
    gym GoalEnv surface the learner's rollout loop uses -- reset() / step(action) returning the dict observation
    {'observation', 'achieved_goal', 'desired_goal'} (bmirobot_env_push_F.py:233-237), step's 4-tuple with
    info['is_success'] (:103-108) and a compute_reward vectorised over leading dims (:84-90) -- around a point mass
    that the first three action components push through a 0.5 m box.  The observation keeps the bmirobot layout
    (27 = 9 blocks of 3, achieved goal = block 4, :214,228).  It has its own RandomState so it never draws from
    numpy's global stream, which belongs to the exploration noise."""

    def __init__(self, seed=0, max_timesteps=100, distance_threshold=0.05, reward_type='sparse', step_scale=0.1):
        super().__init__(seed, max_timesteps, distance_threshold, reward_type, step_scale)
        self.pos = np.zeros(3)
        self.vel = np.zeros(3)
        self.goal = np.zeros(3)

    def _observation(self):
        obs = np.zeros(27)
        obs[0:3] = self.pos                  # "gripper" block
        obs[3:6] = self.vel
        obs[12:15] = self.pos                # the block whose position is the achieved goal
        return {'observation': obs, 'achieved_goal': self.pos.copy(), 'desired_goal': self.goal.copy()}

    def reset(self):
        self.pos = self.rs.uniform(0.0, 0.5, 3)
        self.goal = self.rs.uniform(0.0, 0.5, 3)
        self.vel = np.zeros(3)
        return self._observation()

    def step(self, action):
        action = np.clip(np.asarray(action, dtype=np.float64), -0.5, 0.5)
        new = np.clip(self.pos + self.step_scale * action[:3], 0.0, 0.5)
        self.vel = new - self.pos
        self.pos = new
        return self._stepped()


# the workspace of the push-block environments (synthetic.PushBlockGoalEnv, device_env.PushBlockVecEnv, PushBlockEnvDev in
# csrc/env_device.h): x, y of gripper and block; the gripper's z runs from the table up to PUSH_Z_HI and starts at PUSH_START_Z
PUSH_X_LO, PUSH_X_HI, PUSH_Y_LO, PUSH_Y_HI, PUSH_Z_HI, PUSH_START_Z = 0.0, 0.5, 0.0, 0.7, 0.5, 0.3
# the four draws of one reset attempt, in draw order: block x, y, goal x, y (low, high)
PUSH_RESET_BOUNDS = ((0.15, 0.35), (0.2, 0.5), (0.0, 0.35), (0.2, 0.5))
PUSH_RESET_ATTEMPTS = 100


def push_separated(env, bx, by, gx, gy):
    """Whether one attempt of the push block's reset stands: block and target `env.min_separation` apart on the table"""
    ddx, ddy = bx - gx, by - gy
    return np.sqrt(ddx * ddx + ddy * ddy) >= env.min_separation


class PushBlockGoalEnv(_HostGoalEnv):
    """A kinematic planar push with the GoalEnv surface of `PointMassGoalEnv`: the setting of the reference's Push task
    (bmirobot_env_push_F.py) in which the achieved goal is a block that moves only on contact, so that most actions leave it
    where it is and the reward is sparse in earnest.  The block is a square of half width `half_width` resting on the table; the
    first three action components move the gripper (the fourth, the fingers, is ignored: :94); while the gripper is below
    `z_touch` and inside the square, the block is pushed out along the axis of least penetration.  `step` is adds, subtracts,
    multiplies, compares and clamps only -- no division, no square root -- so that the tensor twin and the device struct agree
    with it bit for bit by construction.  `reset` redraws block and target until they are `min_separation` apart (:117-132, at
    most 100 attempts; the last attempt is kept either way), four scalars per attempt from the environment's own RandomState."""

    def __init__(self, seed=0, max_timesteps=100, distance_threshold=0.05, reward_type='sparse', step_scale=0.1, half_width=0.04,
                 z_touch=0.25, min_separation=0.15, table_z=0.2, grip_start=(0.25, 0.1)):
        super().__init__(seed, max_timesteps, distance_threshold, reward_type, step_scale)
        self.half_width, self.z_touch = float(half_width), float(z_touch)
        self.min_separation, self.table_z = float(min_separation), float(table_z)
        self.grip_start = (float(grip_start[0]), float(grip_start[1]))
        self.grip, self.blk, self.goal = np.zeros(3), np.zeros(3), np.zeros(3)
        self.gvel, self.bvel = np.zeros(3), np.zeros(3)
        self.reset_attempts = 0              # attempts the last reset took

    def _observation(self):
        obs = np.zeros(27)                   # the bmirobot layout (:208-222): nine blocks of three
        obs[0:3] = self.grip
        obs[6:9] = self.gvel
        obs[12:15] = self.blk
        obs[18:21] = self.blk - self.grip
        obs[21:24] = self.bvel
        return {'observation': obs, 'achieved_goal': self.blk.copy(), 'desired_goal': self.goal.copy()}

    def reset(self):
        (bx, by, gx, gy), self.reset_attempts = rejection_reset(self.rs, PUSH_RESET_BOUNDS, PUSH_RESET_ATTEMPTS,
                                                                 lambda *u: push_separated(self, *u))
        self.blk = np.array([bx, by, self.table_z])
        self.goal = np.array([gx, gy, self.table_z])
        self.grip = np.array([self.grip_start[0], self.grip_start[1], PUSH_START_Z])
        self.gvel, self.bvel = np.zeros(3), np.zeros(3)
        return self._observation()

    def step(self, action):
        r = self.half_width
        action = np.clip(np.asarray(action, dtype=np.float64), -0.5, 0.5)
        lo = np.array([PUSH_X_LO, PUSH_Y_LO, self.table_z])
        hi = np.array([PUSH_X_HI, PUSH_Y_HI, PUSH_Z_HI])
        new = np.clip(self.grip + self.step_scale * action[:3], lo, hi)
        self.gvel = new - self.grip
        self.grip = new
        old = self.blk.copy()
        dx, dy = self.blk[0] - self.grip[0], self.blk[1] - self.grip[1]
        if self.grip[2] < self.z_touch and abs(dx) < r and abs(dy) < r:
            px, py = r - abs(dx), r - abs(dy)          # how deep the gripper is inside the block, per axis
            if px <= py:                               # out along the axis of least penetration
                self.blk[0] = self.grip[0] + (r if dx >= 0 else -r)
            else:
                self.blk[1] = self.grip[1] + (r if dy >= 0 else -r)
            self.blk[0] = min(max(self.blk[0], PUSH_X_LO), PUSH_X_HI)
            self.blk[1] = min(max(self.blk[1], PUSH_Y_LO), PUSH_Y_HI)
        self.bvel = self.blk - old
        return self._stepped()


# the workspace of the pick-and-place environments (synthetic.PickPlaceGoalEnv, device_env.PickPlaceVecEnv, PickPlaceEnvDev in
# csrc/env_device.h): x, y, z of gripper and block alike, z from the table up to PICK_Z_HI; the gripper starts at PICK_START_Z
PICK_X_LO, PICK_X_HI, PICK_Y_LO, PICK_Y_HI, PICK_Z_HI, PICK_START_Z = 0.0, 0.5, 0.0, 0.7, 0.6, 0.3
# the finger pads relative to the reported gripper position: the offsets of get_demo_data_pick.py:62-63 negated, so that the
# scripted grasp pose puts the pads on the block centre
PICK_TOOL = (0.0, 0.05, -0.05)
PICK_FINGER_MAX, PICK_GRASP_WIDTH = 0.08, 0.04
# the five draws of one reset attempt, in draw order: block x, y, goal x, y, z (low, high)
PICK_RESET_BOUNDS = ((0.15, 0.35), (0.2, 0.5), (0.0, 0.35), (0.3, 0.55), (0.3, 0.5))
PICK_RESET_ATTEMPTS = 100


def pick_separated(env, bx, by, gx, gy, gz):
    """Whether one attempt of the pick-and-place's reset stands: the block on the table and the target `env.min_separation` apart"""
    ddx, ddy, ddz = bx - gx, by - gy, env.table_z - gz
    return np.sqrt(ddx * ddx + ddy * ddy + ddz * ddz) >= env.min_separation


class PickPlaceGoalEnv(_HostGoalEnv):
    """A kinematic pick-and-place with the GoalEnv surface of `PushBlockGoalEnv`: the setting of the reference's PickAndPlace task
    (bmirobot_env_pickandplace_v2.py), in which the goal hangs in the air and the block gets there only in a closed hand.  The
    block is a cube of half width `half_width`; the finger pads sit at grip + PICK_TOOL.  The first three action components move
    the gripper, the fourth opens (+) and closes (-) the fingers, `finger_scale` per unit.  While the pads are inside the cube --
    or the block is held -- the environment overwrites the fourth component with -1 behind the clip (the reference's finger lock,
    :93-95).  The block is grasped in the step in which fingers wider than PICK_GRASP_WIDTH close to it or below with the pads
    inside the cube, and a held block follows the gripper from the next step on.  The lock keeps closing a held block's fingers,
    so a grasp never opens: the reference's quirk, kept (release and gravity are not modelled).  A gripper that arrives closed
    passes through the block.  `step` is adds, subtracts, multiplies, compares and clamps only, so that the tensor twin and the
    device struct agree with it bit for bit by construction.  `reset` redraws block and target until they are `min_separation`
    apart in three dimensions (:116-131 without the orientation draws; at most 100 attempts, the last one kept either way), five
    scalars per attempt from the environment's own RandomState."""

    def __init__(self, seed=0, max_timesteps=100, distance_threshold=0.05, reward_type='sparse', step_scale=0.2, half_width=0.04,
                 finger_scale=0.05, min_separation=0.15, table_z=0.2, grip_start=(0.25, 0.1)):
        super().__init__(seed, max_timesteps, distance_threshold, reward_type, step_scale)
        self.half_width, self.finger_scale = float(half_width), float(finger_scale)
        self.min_separation, self.table_z = float(min_separation), float(table_z)
        self.grip_start = (float(grip_start[0]), float(grip_start[1]))
        self.grip, self.blk, self.goal = np.zeros(3), np.zeros(3), np.zeros(3)
        self.gvel, self.bvel = np.zeros(3), np.zeros(3)
        self.finger, self.held = 0.0, 0.0    # the opening of the fingers; 1.0 once the block is grasped
        self.reset_attempts = 0              # attempts the last reset took

    def _observation(self):
        obs = np.zeros(27)                   # the bmirobot layout: nine blocks of three
        obs[0:3] = self.grip
        obs[6:9] = self.gvel
        obs[9] = self.finger
        obs[10] = self.held
        obs[12:15] = self.blk
        obs[18:21] = self.blk - self.grip
        obs[21:24] = self.bvel
        return {'observation': obs, 'achieved_goal': self.blk.copy(), 'desired_goal': self.goal.copy()}

    def reset(self):
        (bx, by, gx, gy, gz), self.reset_attempts = rejection_reset(self.rs, PICK_RESET_BOUNDS, PICK_RESET_ATTEMPTS,
                                                                     lambda *u: pick_separated(self, *u))
        self.blk = np.array([bx, by, self.table_z])
        self.goal = np.array([gx, gy, gz])
        self.grip = np.array([self.grip_start[0], self.grip_start[1], PICK_START_Z])
        self.gvel, self.bvel = np.zeros(3), np.zeros(3)
        self.finger, self.held = 0.0, 0.0
        return self._observation()

    def _pads_inside(self):
        """Every finger pad coordinate is less than half_width from the block centre"""
        return all(abs(self.blk[c] - (self.grip[c] + PICK_TOOL[c])) < self.half_width for c in range(3))

    def step(self, action):
        action = np.clip(np.asarray(action, dtype=np.float64), -0.5, 0.5)
        if self.held != 0.0 or self._pads_inside():          # :93-95 the finger lock, behind the clip
            action[3] = -1.0
        f_old = self.finger
        self.finger = min(max(self.finger + self.finger_scale * action[3], 0.0), PICK_FINGER_MAX)
        lo = np.array([PICK_X_LO, PICK_Y_LO, self.table_z])
        hi = np.array([PICK_X_HI, PICK_Y_HI, PICK_Z_HI])
        new = np.clip(self.grip + self.step_scale * action[:3], lo, hi)
        self.gvel = new - self.grip
        self.grip = new
        old = self.blk.copy()
        if self.held != 0.0:                                  # carried: the gripper's clipped displacement, clipped again
            self.blk = np.clip(self.blk + self.gvel, lo, hi)
        elif self._pads_inside() and f_old > PICK_GRASP_WIDTH and self.finger <= PICK_GRASP_WIDTH:
            self.held = 1.0                                   # grasped; the block moves from the next step on
        self.bvel = self.blk - old
        return self._stepped()


# ---- demonstrations from a scripted controller (the reference's get_demo_data_push.py) ------------------------------------------
def _check_phase_ends(name, phase_end):
    """The rule of both schedules: the first phase end is not negative and every later one lies behind the one before it"""
    if phase_end[0] < 0 or any(b <= a for a, b in zip(phase_end, phase_end[1:])):
        raise ValueError(f"{name}: the phase ends {phase_end} must be increasing")


class DemoScript:
    """The numbers of the reference's push schedule (get_demo_data_push.py:39-61); the defaults are the reference's.
    `phase_end`: the last timestep, counted from 1, of phases one to five (:43, :45, :49, :51, :53; the sixth runs to T);
    `lift`: the constant action of phase one (:44); `waypoint`: where phase four takes the gripper (:52); `behind`: the factor
    that places the gripper behind the block (:46-48); `stop_radius`: block-to-goal distance under which the action is zero
    (:59-61).  hp_demo_script of include/rlarm_hip.h holds the same fields."""

    def __init__(self, phase_end=(10, 20, 40, 60, 80), lift=(0.0, -0.1, 0.1, 0.0), waypoint=(0.241, 0.3265, 0.294), behind=-0.5,
                 stop_radius=0.05):
        self.phase_end = tuple(int(e) for e in phase_end)
        self.lift = tuple(float(v) for v in lift)
        self.waypoint = tuple(float(v) for v in waypoint)
        self.behind, self.stop_radius = float(behind), float(stop_radius)
        if len(self.phase_end) != 5 or len(self.lift) != 4 or len(self.waypoint) != 3:
            raise ValueError("DemoScript: five phase ends, four lift components, three waypoint components")
        _check_phase_ends("DemoScript", self.phase_end)


def scripted_action(t, obs, g, script=None):
    """The reference's push controller (get_demo_data_push.py:39-61) for timestep t = 1 .. T: the float64 action [4], unclipped,
    out of the observation row -- gripper obs[0:3], block obs[12:15] -- and the desired goal.  It reads the bmirobot layout only,
    so it serves every environment that keeps it.  One float64 operation per rounding, sums left to right: csrc/demo_episodes.h
    (demo_action) repeats them one by one."""
    s = script or DemoScript()
    grip = [float(obs[0]), float(obs[1]), float(obs[2])]
    b = [float(obs[12]), float(obs[13]), float(obs[14])]
    g = [float(g[0]), float(g[1]), float(g[2])]
    e = s.phase_end
    k = s.behind
    if t <= e[0]:                                     # :43-44 lift and retreat
        action = list(s.lift)
    elif t <= e[1] or e[3] < t <= e[4]:               # :45-48, :53-56 go behind the block
        action = [(g[0] - b[0]) * k + b[0] - grip[0],
                  (g[1] - b[1]) * k + b[1] - grip[1],
                  b[2] + (g[2] - b[2]) * k - grip[2], 0.0]
    elif e[2] < t <= e[3]:                            # :51-52 return to the waypoint
        action = [s.waypoint[0] - grip[0], s.waypoint[1] - grip[1], s.waypoint[2] - grip[2], 0.0]
    else:                                             # :49-50, :57-58 push
        action = [g[0] - b[0], g[1] - b[1], g[2] - b[2], 0.0]
    dx, dy, dz = b[0] - g[0], b[1] - g[1], b[2] - g[2]
    if np.sqrt(dx * dx + dy * dy + dz * dz) < s.stop_radius:     # :59-61 the stop rule, on top of every phase
        action = [0.0, 0.0, 0.0, 0.0]
    return np.array(action, dtype=np.float64)


class PickScript:
    """The numbers of the reference's pick-and-place schedule (get_demo_data_pick.py:54-67); the defaults are the reference's.
    `phase_end`: the last timestep, counted from 1, of phases one to five (the sixth runs to T); `lift`: the constant action of
    phase one (:55); `approach`: what phase two adds to block - gripper (:57-58); `grasp`: what phase four adds to it (:62-63);
    `open`: the finger action of phase three (:60), and negated that of phase five (:65).  hp_pick_script of include/rlarm_hip.h
    holds the same fields."""

    def __init__(self, phase_end=(10, 30, 50, 70, 90), lift=(0.0, -0.1, 0.1, 0.0), approach=(0.0, -0.2, 0.1), grasp=(0.0, -0.05, 0.05),
                 open=0.1):
        self.phase_end = tuple(int(e) for e in phase_end)
        self.lift = tuple(float(v) for v in lift)
        self.approach = tuple(float(v) for v in approach)
        self.grasp = tuple(float(v) for v in grasp)
        self.open = float(open)
        if len(self.phase_end) != 5 or len(self.lift) != 4 or len(self.approach) != 3 or len(self.grasp) != 3:
            raise ValueError("PickScript: five phase ends, four lift components, three approach and three grasp components")
        _check_phase_ends("PickScript", self.phase_end)


def pick_scripted_action(t, obs, g, script=None):
    """The reference's pick-and-place controller (get_demo_data_pick.py:54-67) for timestep t = 1 .. T: the float64 action [4],
    unclipped, out of the observation row -- gripper obs[0:3], block obs[12:15] -- and the desired goal.  No stop rule.  One
    float64 operation per rounding; the offset is always added, also where it is 0.0: csrc/demo_episodes.h (demo_action_pick)
    repeats the operations one by one."""
    s = script or PickScript()
    grip = [float(obs[0]), float(obs[1]), float(obs[2])]
    b = [float(obs[12]), float(obs[13]), float(obs[14])]
    g = [float(g[0]), float(g[1]), float(g[2])]
    e = s.phase_end
    if t <= e[0]:                                     # :54-55 lift and retreat
        action = list(s.lift)
    elif t <= e[1]:                                   # :56-58 above and in front of the block
        action = [(b[c] - grip[c]) + s.approach[c] for c in range(3)] + [0.0]
    elif t <= e[2]:                                   # :59-60 open the fingers
        action = [0.0, 0.0, 0.0, s.open]
    elif t <= e[3]:                                   # :61-63 the pads onto the block
        action = [(b[c] - grip[c]) + s.grasp[c] for c in range(3)] + [0.0]
    elif t <= e[4]:                                   # :64-65 close the fingers
        action = [0.0, 0.0, 0.0, -s.open]
    else:                                             # :66-67 carry the block to the goal
        action = [g[0] - b[0], g[1] - b[1], g[2] - b[2], 0.0]
    return np.array(action, dtype=np.float64)


def scripted_episode(env, script=None):
    """One episode of a scripted controller on a host environment, reset from its own `rs` (get_demo_data_push.py:34-74) --
    `pick_scripted_action` with a `PickScript`, `scripted_action` with a `DemoScript` or None:
    (obs [T+1, obs], ag [T+1, goal], g [T, goal], actions [T, act], is_success after every step [T])."""
    T = int(env.max_timesteps)
    controller = pick_scripted_action if isinstance(script, PickScript) else scripted_action
    o = env.reset()
    obs, ag, g = o['observation'], o['achieved_goal'], o['desired_goal']
    ep_obs, ep_ag, ep_g, ep_act, ep_ok = [], [], [], [], []
    for t in range(1, T + 1):
        action = controller(t, obs, g, script)
        o, _, _, info = env.step(action)
        ep_obs.append(obs.copy()); ep_ag.append(ag.copy()); ep_g.append(g.copy()); ep_act.append(action)
        ep_ok.append(np.float32(info['is_success']))
        obs, ag = o['observation'], o['achieved_goal']
    ep_obs.append(obs.copy()); ep_ag.append(ag.copy())
    return np.array(ep_obs), np.array(ep_ag), np.array(ep_g), np.array(ep_act), np.array(ep_ok, dtype=np.float32)


def scripted_demos(envs, n_demos, round_waves, max_episodes=10000, script=None):
    """Successful scripted episodes of the host environments `envs` (PointMassGoalEnv / PushBlockGoalEnv / PickPlaceGoalEnv;
    `script`: a `DemoScript`, a `PickScript` or None as in `scripted_episode`), a pure function of its
    inputs -- the host statement of `device_env.generate_demos`.  A round attempts len(envs) * round_waves episodes, cut to what
    `max_episodes` leaves; episode e = w * n_envs + i of a round is environment i's w-th, reset from that environment's own `rs`
    (the numbering of hp_rollout_waves).  An episode is kept if `is_success` is 1 after its last step; kept episodes stay in
    order of round, then of e, and the first `n_demos` are returned.  Rounds are whole: the surplus of the last round is dropped
    but its resets are consumed.  Generation stops when n_demos are kept or max_episodes attempted.  Returns
    (obs [k, T+1, obs], ag [k, T+1, goal], g [k, T, goal], actions [k, T, act], info [k, T] float32, attempted).  With one
    environment this is the reference's loop (get_demo_data_push.py:27-90) with its order of kept episodes."""
    n_envs, n_demos, round_waves = len(envs), int(n_demos), int(round_waves)
    if n_envs < 1 or n_demos < 1 or round_waves < 1:
        raise ValueError("scripted_demos: at least one environment, one demonstration and one wave per round")
    kept, attempted = [], 0
    while len(kept) < n_demos and attempted < max_episodes:
        n = min(n_envs * round_waves, max_episodes - attempted)
        for e in range(n):
            ep = scripted_episode(envs[e % n_envs], script)
            if ep[4][-1] == 1.0:
                kept.append(ep)
        attempted += n
    kept = kept[:n_demos]
    T, p = int(envs[0].max_timesteps), envs[0].env_params
    shapes = ((T + 1, p['obs']), (T + 1, p['goal']), (T, p['goal']), (T, p['action']), (T,))
    out = [np.array([ep[j] for ep in kept], dtype=np.float32 if j == 4 else np.float64).reshape((len(kept),) + shapes[j])
           for j in range(5)]
    return (*out, attempted)


EPISODE_STATS = ("ret", "final_distance", "min_distance", "first_success_step", "success_steps", "final_success")
EPISODE_SUMMARY = ("ret", "final_distance", "min_distance", "first_success_step", "success_rate", "any_success_rate")


def episode_stats(ag, g, distance_threshold):
    """The host twin of hp_episode_stats, in plain numpy: `ag` [n, T+1, goal] and `g` [n, T, goal] -> (stats [n, 6] float64 in the
    columns of EPISODE_STATS, step_success [n, T] float32).  Step t compares ag[t + 1] with g[t] (her.py:38); the distance is the
    root of the squares summed left to right over the goal components, which is `np.linalg.norm(a - b, axis=-1)` for fewer than
    8 of them; success is d < threshold (_is_success) and the reward -(d > threshold) in float32 (compute_reward, sparse).  `ret`
    is numpy's own sum of those rewards: +0.0 for an episode that succeeds at every step.  first_success_step is T where there
    is no success."""
    ag, g = np.asarray(ag, dtype=np.float64), np.asarray(g, dtype=np.float64)
    if ag.ndim != 3 or g.ndim != 3 or ag.shape[0] != g.shape[0] or ag.shape[1] != g.shape[1] + 1 or ag.shape[2] != g.shape[2]:
        raise ValueError("episode_stats: ag [n, T+1, goal] and g [n, T, goal] expected")
    n, T, thr = g.shape[0], g.shape[1], float(distance_threshold)
    diff = ag[:, 1:] - g
    sq = diff * diff
    s = sq[..., 0]
    for c in range(1, sq.shape[-1]):
        s = s + sq[..., c]
    d = np.sqrt(s)
    ok = d < thr
    reward = -(d > thr).astype(np.float32)
    stats = np.empty((n, len(EPISODE_STATS)), dtype=np.float64)
    stats[:, 0] = reward.astype(np.float64).sum(axis=1)
    stats[:, 1] = d[:, -1]
    stats[:, 2] = d.min(axis=1)
    stats[:, 3] = np.where(ok.any(axis=1), ok.argmax(axis=1), T)
    stats[:, 4] = ok.sum(axis=1)
    stats[:, 5] = ok[:, -1]
    return stats, ok.astype(np.float32)


def episode_stats_summary(stats):
    """The host twin of hp_episode_stats_summary: the columns of EPISODE_SUMMARY, each a left-to-right float64 sum over the rows
    of `stats` in order, divided by their number -- the device's loop, not numpy's pairwise mean."""
    stats = np.asarray(stats, dtype=np.float64)
    if stats.ndim != 2 or stats.shape[1] != len(EPISODE_STATS) or stats.shape[0] < 1:
        raise ValueError("episode_stats_summary: stats [n >= 1, 6] expected")
    total = np.zeros(len(EPISODE_SUMMARY), dtype=np.float64)
    for row in stats:
        total[0] += row[0]
        total[1] += row[1]
        total[2] += row[2]
        total[3] += row[3]
        total[4] += row[5]
        total[5] += 1.0 if row[4] > 0.0 else 0.0
    return total / np.float64(stats.shape[0])


CRITIC_STATS = ("q_mean", "return_mean", "bias", "abs_error", "max_abs_error", "floor_steps")


def _reward_kind(reward_type):
    if reward_type in ("sparse", 0):
        return 0
    if reward_type in ("dense", 1):
        return 1
    raise ValueError(f"reward_type {reward_type!r} is neither 'sparse' nor 'dense'")


def _tail_kind(tail):
    if tail in ("zero", 0):
        return 0
    if tail in ("persist", 1):
        return 1
    raise ValueError(f"tail {tail!r} is neither 'zero' nor 'persist'")


def _check_gamma(gamma, tail):
    gamma = float(gamma)
    if not 0.0 <= gamma <= 1.0:
        raise ValueError(f"gamma {gamma} outside [0, 1]")
    if gamma == 1.0 and tail == 1:
        raise ValueError("gamma 1 with tail 'persist' has no finite return")
    return np.float64(gamma)


def episode_returns(ag, g, distance_threshold, gamma, reward_type="sparse", tail="persist"):
    """The host twin of hp_episode_returns, as plain loops: `ag` [n, T+1, goal] and `g` [n, T, goal] -> G [n, T] float64, the
    discounted return every step went on to collect.  r[t] is compute_reward's on (ag[t + 1], g[t]) in float64 -- sparse:
    -(d > threshold) (the float32 of `episode_stats`, widened), dense: -d -- with d the root of the squares summed left to right.
    G[T] = +0.0 (tail 'zero') or r[T-1] / (1 - gamma) (tail 'persist': the last step's reward held for ever, what an
    infinite-horizon critic is trained towards); G[t] = r[t] + gamma * G[t+1], one rounding per operation.  gamma must lie in
    [0, 1]; gamma = 1 with tail 'persist' raises."""
    ag, g = np.asarray(ag, dtype=np.float64), np.asarray(g, dtype=np.float64)
    if ag.ndim != 3 or g.ndim != 3 or ag.shape[0] != g.shape[0] or ag.shape[1] != g.shape[1] + 1 or ag.shape[2] != g.shape[2]:
        raise ValueError("episode_returns: ag [n, T+1, goal] and g [n, T, goal] expected")
    kind, tail = _reward_kind(reward_type), _tail_kind(tail)
    gamma = _check_gamma(gamma, tail)
    n, T, thr = g.shape[0], g.shape[1], float(distance_threshold)
    diff = ag[:, 1:] - g
    sq = diff * diff
    s = sq[..., 0]
    for c in range(1, sq.shape[-1]):
        s = s + sq[..., c]
    d = np.sqrt(s)
    r = (-(d > thr).astype(np.float32)).astype(np.float64) if kind == 0 else -d
    G = np.empty((n, T), dtype=np.float64)
    gamma = float(gamma)                     # Python floats from here on: IEEE float64, one rounding per operation
    for e in range(n):
        row = r[e].tolist()
        acc = row[T - 1] / (1.0 - gamma) if tail == 1 else 0.0
        for t in range(T - 1, -1, -1):
            acc = row[t] + gamma * acc
            row[t] = acc
        G[e] = row
    return G


def episode_critic_stats(q, returns, gamma):
    """The host twin of the critic columns of hp_episode_returns: `q` [n, T] float32 and `returns` [n, T] float64 -> [n, 6]
    float64 in the columns of CRITIC_STATS.  One accumulator per column, Q widened to float64, summed in the order of the
    recursion -- t = T-1 down to 0 -- and divided by T; max_abs_error and floor_steps (steps with Q <= -1 / (1 - gamma), the target
    clip of ddpg_agent.py:259-260; 0 when gamma = 1) are not divided.  The device's loop, not numpy's pairwise mean."""
    q, returns = np.asarray(q), np.asarray(returns, dtype=np.float64)
    if q.dtype != np.float32 or q.ndim != 2 or q.shape != returns.shape or q.shape[1] < 1:
        raise ValueError("episode_critic_stats: q [n, T] float32 and returns [n, T] float64 expected")
    gamma = float(_check_gamma(gamma, 0))    # Python floats from here on: IEEE float64, one rounding per operation
    has_floor = gamma < 1.0
    floor = -(1.0 / (1.0 - gamma)) if has_floor else 0.0
    n, T = q.shape
    out = np.empty((n, len(CRITIC_STATS)), dtype=np.float64)
    for e in range(n):
        qs, Gs = q[e].astype(np.float64).tolist(), returns[e].tolist()
        sum_q = sum_g = sum_b = sum_a = max_a = 0.0
        steps = 0
        for t in range(T - 1, -1, -1):
            qd, G = qs[t], Gs[t]
            d = qd - G
            a = abs(d)
            sum_q = sum_q + qd
            sum_g = sum_g + G
            sum_b = sum_b + d
            sum_a = sum_a + a
            max_a = a if a > max_a else max_a
            steps += 1 if (has_floor and qd <= floor) else 0
        dT = float(T)
        out[e] = (sum_q / dT, sum_g / dT, sum_b / dT, sum_a / dT, max_a, float(steps))
    return out


def _column_means(who, names, stats):
    """The one loop behind episode_critic_summary and episode_policy_summary: left-to-right float64 sums in episode order"""
    stats = np.asarray(stats, dtype=np.float64)
    if stats.ndim != 2 or stats.shape[1] != len(names) or stats.shape[0] < 1:
        raise ValueError(f"{who}: stats [n >= 1, {len(names)}] expected")
    total = np.zeros(len(names), dtype=np.float64)
    for row in stats:
        for k in range(len(names)):
            total[k] = total[k] + row[k]
    return total / np.float64(stats.shape[0])


def episode_critic_summary(stats):
    """The host twin of hp_episode_critic_summary: the six column means over the episodes, each a left-to-right float64 sum in
    episode order divided by their number."""
    return _column_means("episode_critic_summary", CRITIC_STATS, stats)


POLICY_STATS = ("q_pi_mean", "advantage_mean", "q_filter_share", "action_gap_mean", "saturated_share", "action_l2_mean")


def episode_policy_stats(pi, q_pi, actions, max_action, q=None, sat=0.99):
    """The host twin of hp_episode_policy_stats, as plain loops: `pi` [n, T, act] float32 (the policy's actions), `q_pi` [n, T]
    float32 (Q(s, pi(s))), `actions` [n, T, act] float64 (the recorded ones) and optionally `q` [n, T] float32 (Q(s, a),
    `episode_q` of the same episodes) -> [n, 6] float64 in the columns of POLICY_STATS.  max_action is the networks' float32,
    widened; every float32 is widened, every sum starts at 0 and runs in ascending t (inner j ascending), one rounding per
    operation, and is divided once at the end: q_pi_mean; advantage_mean, the mean of Q(s, pi(s)) - Q(s, a); q_filter_share, the
    share of steps with Q(s, a) > Q(s, pi(s)) compared in float32; action_gap_mean, (sum of the Euclidean distances a - pi) /
    max_action / T; saturated_share, the share of components with |pi| >= sat * max_action; action_l2_mean, the mean over t of
    sum_j (pi_j / max_action)^2 / act -- the regulariser's term of the actor loss (ddpg_agent.py:267).  Without `q` the second and
    third column are NaN."""
    pi, q_pi, actions = np.asarray(pi), np.asarray(q_pi), np.asarray(actions, dtype=np.float64)
    if (pi.dtype != np.float32 or q_pi.dtype != np.float32 or pi.ndim != 3 or q_pi.shape != pi.shape[:2] or actions.shape != pi.shape
            or pi.shape[1] < 1 or pi.shape[2] < 1):
        raise ValueError("episode_policy_stats: pi [n, T, act] float32, q_pi [n, T] float32 and actions [n, T, act] expected")
    if q is not None:
        q = np.asarray(q)
        if q.dtype != np.float32 or q.shape != q_pi.shape:
            raise ValueError("episode_policy_stats: q [n, T] float32 expected")
    sat = float(sat)
    if not 0.0 <= sat <= 1.0:
        raise ValueError(f"sat {sat} outside [0, 1]")
    ma = float(np.float32(max_action))       # Python floats from here on: IEEE float64, one rounding per operation
    if not (ma > 0.0 and math.isfinite(ma)):
        raise ValueError(f"max_action {max_action} is not a positive number")
    bound = sat * ma
    n, T, ad = pi.shape
    out = np.empty((n, len(POLICY_STATS)), dtype=np.float64)
    for e in range(n):
        ps, acts, qps = pi[e].astype(np.float64).tolist(), actions[e].tolist(), q_pi[e].astype(np.float64).tolist()
        qs = q[e].astype(np.float64).tolist() if q is not None else None
        sum_qpi = sum_adv = sum_gap = sum_l2 = 0.0
        filtered = saturated = 0
        for t in range(T):
            sum_qpi = sum_qpi + qps[t]
            if qs is not None:
                sum_adv = sum_adv + (qps[t] - qs[t])
                filtered += 1 if q[e, t] > q_pi[e, t] else 0
            dd = vv = 0.0
            for j in range(ad):
                p = ps[t][j]
                d = acts[t][j] - p
                v = p / ma
                dd = dd + d * d
                vv = vv + v * v
                saturated += 1 if abs(p) >= bound else 0
            sum_gap = sum_gap + math.sqrt(dd)
            sum_l2 = sum_l2 + vv / float(ad)
        dT = float(T)
        out[e] = (sum_qpi / dT, sum_adv / dT if qs is not None else float("nan"),
                  float(filtered) / dT if qs is not None else float("nan"), sum_gap / ma / dT,
                  float(saturated) / float(T * ad), sum_l2 / dT)
    return out


def episode_policy_summary(stats):
    """The host twin of hp_episode_policy_summary: the six column means over the episodes, each a left-to-right float64 sum in
    episode order divided by their number."""
    return _column_means("episode_policy_summary", POLICY_STATS, stats)


SIGNAL_STATS = ("grad_norm", "flat_share", "reg_share", "toward_recorded", "linear_adv", "trunk_signal")


def episode_signal_stats(pi, dq_du, actions, max_action, action_l2=1.0, flat=1e-3):
    """The host twin of hp_episode_signal_stats, as plain loops: `pi` [n, T, act] float32 (the policy's actions), `dq_du`
    [n, T, act] float32 (dQ/du at u = pi / max_action, `episode_action_grad` of the same episodes) and `actions` [n, T, act]
    float64 (the recorded ones) -> [n, 6] float64 in the columns of SIGNAL_STATS.  max_action is the networks' float32, widened;
    every float32 is widened, every sum starts at 0 and runs in ascending t (inner j ascending), one rounding per operation, and
    is divided once at the end.  Per step g_j = dq_du_j, v_j = pi_j / M, d_j = (a_j - pi_j) / M, |x| = sqrt(sum_j x_j x_j):
    grad_norm, the mean of |g|; flat_share, the share of steps with |g| < flat; reg_share, the share with
    (action_l2 * (2 / act)) * |v| > |g| -- the regulariser outweighs the critic; toward_recorded, the mean of
    (sum_j g_j d_j) / (|g| * |d|), a step counting 0 where that product is 0; linear_adv, the mean of sum_j g_j d_j -- the
    first-order estimate of Q(s, a) - Q(s, pi(s)); trunk_signal, the mean of |s| with
    s_j = (g_j - ((action_l2 * 2) * v_j) / act) * (1 - v_j v_j), what reaches the actor's trunk behind the tanh
    (ddpg_agent.py:265-267)."""
    pi, dq_du, actions = np.asarray(pi), np.asarray(dq_du), np.asarray(actions, dtype=np.float64)
    if (pi.dtype != np.float32 or dq_du.dtype != np.float32 or pi.ndim != 3 or dq_du.shape != pi.shape or actions.shape != pi.shape
            or pi.shape[1] < 1 or pi.shape[2] < 1):
        raise ValueError("episode_signal_stats: pi [n, T, act] float32, dq_du [n, T, act] float32 and actions [n, T, act] expected")
    ma, lam, flat = float(np.float32(max_action)), float(action_l2), float(flat)
    if not (ma > 0.0 and math.isfinite(ma)):
        raise ValueError(f"max_action {max_action} is not a positive number")
    if not (lam >= 0.0 and math.isfinite(lam)):
        raise ValueError(f"action_l2 {action_l2} is not a finite number >= 0")
    if not (flat >= 0.0 and math.isfinite(flat)):
        raise ValueError(f"flat {flat} is not a finite number >= 0")
    n, T, ad = pi.shape
    dad = float(ad)
    lam2, reg_scale = lam * 2.0, lam * (2.0 / dad)
    out = np.empty((n, len(SIGNAL_STATS)), dtype=np.float64)
    for e in range(n):
        ps, gs, acts = pi[e].astype(np.float64).tolist(), dq_du[e].astype(np.float64).tolist(), actions[e].tolist()
        sum_gn = sum_cos = sum_dot = sum_trunk = 0.0
        n_flat = n_reg = 0
        for t in range(T):
            gg = vv = dd = dot = ss = 0.0
            for j in range(ad):
                p, gj = ps[t][j], gs[t][j]
                v = p / ma
                d = (acts[t][j] - p) / ma
                gg = gg + gj * gj
                vv = vv + v * v
                dd = dd + d * d
                dot = dot + gj * d
                s = (gj - (lam2 * v) / dad) * (1.0 - v * v)
                ss = ss + s * s
            gn, vn = math.sqrt(gg), math.sqrt(vv)
            den = gn * math.sqrt(dd)
            n_flat += 1 if gn < flat else 0
            n_reg += 1 if reg_scale * vn > gn else 0
            sum_gn = sum_gn + gn
            sum_cos = sum_cos + (dot / den if den > 0.0 else 0.0)
            sum_dot = sum_dot + dot
            sum_trunk = sum_trunk + math.sqrt(ss)
        dT = float(T)
        out[e] = (sum_gn / dT, float(n_flat) / dT, float(n_reg) / dT, sum_cos / dT, sum_dot / dT, sum_trunk / dT)
    return out


def episode_signal_summary(stats):
    """The host twin of hp_episode_signal_summary: the six column means over the episodes, each a left-to-right float64 sum in
    episode order divided by their number."""
    return _column_means("episode_signal_summary", SIGNAL_STATS, stats)


BELLMAN_STATS = ("td_mean", "td_abs", "td_sq", "target_mean", "clipped_share", "reward_mean")


def bellman_constants(gamma):
    """(gamma32, clip32): the two float32 values an agent with `args.gamma` hands its update kernels -- gamma narrowed, and
    1 / (1 - gamma) formed in float64 and narrowed (ddpg_agent.py:259)."""
    gamma = float(gamma)
    if not 0.0 <= gamma < 1.0:
        raise ValueError(f"gamma {gamma} outside [0, 1)")
    return np.float32(gamma), np.float32(1.0 / (1.0 - gamma))


def episode_bellman_targets(q_next, r, gamma32, clip32):
    """The host twin of the target of hp_episode_bellman: `q_next` and `r` [n, T] float32 -> y [n, T] float32 by the update's two
    float32 operations, y = r + gamma32 * q_next; y = min(max(y, -clip32), 0) (ddpg_agent.py:256-260), one rounding each."""
    q_next, r = np.asarray(q_next), np.asarray(r)
    if q_next.dtype != np.float32 or r.dtype != np.float32 or q_next.ndim != 2 or r.shape != q_next.shape:
        raise ValueError("episode_bellman_targets: q_next [n, T] float32 and r [n, T] float32 expected")
    gamma32, clip32 = np.float32(gamma32), np.float32(clip32)
    y = r + gamma32 * q_next
    return np.minimum(np.maximum(y, -clip32), np.float32(0.0))


def episode_bellman_stats(q, q_next, r, y, gamma32):
    """The host twin of hp_episode_bellman_stats, as plain loops: `q`, `q_next`, `r`, `y` [n, T] float32 -> [n, 6] float64 in the
    columns of BELLMAN_STATS.  With d = float64(y) - float64(q) per step: td_mean, the mean of d; td_abs, the mean of |d|; td_sq,
    the mean of d * d -- the critic loss of these rows; target_mean, the mean of y; clipped_share, the share of steps where
    r + gamma32 * q_next, the target's own float32 expression, is not y -- the clamp changed the value; reward_mean, the mean of
    r.  Every sum starts at 0 and runs in ascending t, one rounding per operation, and is divided once at the end (so a mean of
    rewards that are all -0.0 is +0.0: the sums begin at +0.0)."""
    q, q_next, r, y = (np.asarray(v) for v in (q, q_next, r, y))
    if any(v.dtype != np.float32 or v.shape != q.shape for v in (q, q_next, r, y)) or q.ndim != 2 or q.shape[1] < 1:
        raise ValueError("episode_bellman_stats: q, q_next, r and y [n, T] float32 expected")
    gamma32 = np.float32(gamma32)
    if not 0.0 <= float(gamma32) <= 1.0:
        raise ValueError(f"gamma {float(gamma32)} outside [0, 1]")
    n, T = q.shape
    raw = r + gamma32 * q_next               # float32, one rounding per operation
    changed = (raw != y).tolist()
    out = np.empty((n, len(BELLMAN_STATS)), dtype=np.float64)
    for e in range(n):
        qs, ys, rs = (v[e].astype(np.float64).tolist() for v in (q, y, r))    # Python floats from here on: IEEE float64
        sum_d = sum_abs = sum_sq = sum_y = sum_r = 0.0
        clipped = 0
        for t in range(T):
            d = ys[t] - qs[t]
            sum_d = sum_d + d
            sum_abs = sum_abs + abs(d)
            sum_sq = sum_sq + d * d
            sum_y = sum_y + ys[t]
            sum_r = sum_r + rs[t]
            clipped += 1 if changed[e][t] else 0
        dT = float(T)
        out[e] = (sum_d / dT, sum_abs / dT, sum_sq / dT, sum_y / dT, float(clipped) / dT, sum_r / dT)
    return out


def episode_bellman_summary(stats):
    """The host twin of hp_episode_bellman_summary: the six column means over the episodes, each a left-to-right float64 sum in
    episode order divided by their number."""
    return _column_means("episode_bellman_summary", BELLMAN_STATS, stats)


def write_demo_npz_from(path, obs, ag, g, actions, info):
    """Write episodes in the schema get_demo_data_push.py:91-94 produces: keys acs, obs, info, g, ag, with `info` an object
    array [n, T] of per-step dicts {'is_success': float32} (`info` here: the flags [n, T]).  Such a file preloads through
    `ddpg_agent._init_demo_buffer` and through the reference's own."""
    flags = np.asarray(info)
    boxed = np.empty(flags.shape, dtype=object)
    for idx in np.ndindex(*flags.shape):
        boxed[idx] = {"is_success": np.float32(flags[idx])}
    np.savez_compressed(path, acs=np.asarray(actions, dtype=np.float64), obs=np.asarray(obs, dtype=np.float64), info=boxed,
                        g=np.asarray(g, dtype=np.float64), ag=np.asarray(ag, dtype=np.float64))
