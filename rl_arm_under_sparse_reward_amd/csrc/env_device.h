// env_device.h -- environments the library steps itself: the seam of k_rollout_episodes (rollout_episodes.h).
//
// An environment kind is one struct of __device__ functions over the state of ONE environment; the kernel keeps one instance per
// row of its slab in LDS and calls every function from one lane (lane 0 of the row's wave):
//     static constexpr int OBS, GOAL, ACT     dimensions, compared with the block's on the host before the launch (the kind's row)
//     load(desc, i)                            state of environment i out of the arrays of hp_env_desc (and the parameters)
//     observe(obs, ag, g)                      write the current observation row [OBS], achieved goal [GOAL], desired goal [GOAL]
//     step(action_f32)                         advance by one timestep with the float32 action [ACT] the policy side produced
//     step(action_f64)                         the same operations on a float64 action (a scripted controller's: demo_episodes.h);
//                                              both are step_with, whose first operation widens the component to float64
//     is_success()                             the `is_success` flag of the state just reached
//     store(desc, i)                           write the state back (every array: a reset on the device changes the goal too)
//     static constexpr int STATE_ARRAYS         how many arrays of hp_env_desc.state_dev the kind uses (the null check on the host)
// A kind that can be reset on the device (hp_env_reset, the wave loop of k_rollout_episodes) also declares
//     static constexpr int RESET_DRAWS         uniform draws of one reset ATTEMPT, taken from the environment's own reset stream
//     reset_bounds(k, low, range)              draw k = random_uniform(low, range) = low + range * next_double, in draw order
//                                              (range is the float64 difference high - low, as numpy computes it, never a literal)
//     reset(u)                                 the fresh state out of those RESET_DRAWS values
// and RESET_DRAWS = 0 says the kind has no device reset.  The row's wave draws (env_reset_draw below, mw_draw_uniform) and hands the
// values to lane 0 through LDS.
// A reset with a data-dependent number of draws (a rejection loop on the host: redraw until the state is acceptable) declares
//     static constexpr int RESET_ATTEMPTS      attempts at most (default 1: absent, the reset is one fixed set of draws)
//     bool reset(u)                            builds the state of this attempt and returns whether it is accepted; the state of the
//                                              last attempt is kept, accepted or not
// The row's wave then repeats env_reset_draw + reset until an attempt is accepted or RESET_ATTEMPTS are spent (env_reset_run below):
// lane 0 writes the verdict to one int of the wave's own LDS, every lane reads it behind mw_sync(), so the exit of the loop is
// wave-uniform and the cooperative draws stay under wave-uniform control flow.  The stream is committed once, after the loop.  With
// RESET_ATTEMPTS = 1 there is no loop and no verdict: the code is the fixed reset's.
// Every float64 operation whose rounding the host twin of the environment fixes is an explicit IEEE operation (__dmul_rn, ...), so
// that no contraction can change a bit relative to the elementwise torch / numpy ops of that twin.
// Adding a kind touches this list and nothing else (the third kind, PickPlaceEnvDev, was added by it and found two items it had
// left out: the comments of hp_env_desc and the default script): a struct here; an HP_ENV_* constant in rlarm_hip.h with the
// kind's lines in the params / state_dev comments of hp_env_desc there, and the constant's twin in _lib.py; a unit
// env_<kind>.hip of three lines -- the include of rollout_episodes.h and `const EnvKind env_kind_<kind> = env_kind_entry<Struct>(HP_ENV_...)`,
// which instantiates both kernels for the kind and checks at compile time what a kind must be for them -- and a unit
// demo_<kind>.hip of two, the explicit instantiation of env_launch_demo<Struct> (demo_episodes.h: the scripted-episode kernel, the
// row's third launch), both with their entries in the
// Makefile's EXACT_SRCS; the row's declaration in rollout_episodes.h and its address in the table of env_kind_lookup() (rollout.hip); and
// one Python class pair in device_env.py (the tensor twin, and a native class that names the constant -- and, where the task's
// scripted controller is not the push schedule, its default_demo_script()).  No entry point, dispatch or check names a kind: they
// read the row (env_point_mass.hip, env_push_block.hip and env_pick_place.hip are the models).  A scripted controller is NOT part
// of a kind: the two of demo_episodes.h run on any kind with the bmirobot layout, chosen per call (DemoArgs::controller).
// A gripper-and-block kind (a fourth task of the bmirobot family) derives its struct from GripBlockEnvDev<STRIDE> below and
// writes only what is its own: the constants, its parameters and their lines of load, reset_bounds, the separation test of reset
// in front of place(), the dynamics of step_with behind env_clipped_move, is_success as env_within(blk, goal, threshold), and
// whatever it keeps in array 3 behind the six velocities (load / store / observe call the base's and add those columns).
#pragma once
#include "transition_device.h"
#include <type_traits>

#include "mt19937_wave.h"

// ---- what the kinds share ------------------------------------------------------------------------------------------------------
// |achieved - goal| < threshold over three components: the root (numpy's norm) of tr_sq_distance, (dx dx + dy dy) + dz dz, and
// the comparison.  Every kind's is_success, and the stop rule of demo_action.
__device__ __forceinline__ bool env_within(const double *achieved, const double *goal, double threshold) {
    return __dsqrt_rn(tr_sq_distance(achieved, goal, 3)) < threshold;
}

// The clipped move of every kind: a = clamp(float64(action), -0.5, 0.5); scaled = step_scale * a; moved = clamp(p + scaled, lo, hi);
// v = moved - p; p = moved, per component.  A: float (the policy's action) or double (a scripted controller's).
template <class A>
__device__ __forceinline__ void env_clipped_move(double *__restrict__ p, double *__restrict__ v, const A *__restrict__ action, double step_scale,
                                                 const double *__restrict__ lo, const double *__restrict__ hi) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a = fmin(fmax((double)action[c], -0.5), 0.5);
        const double scaled = __dmul_rn(step_scale, a);
        const double moved = fmin(fmax(__dadd_rn(p[c], scaled), lo[c]), hi[c]);
        v[c] = __dsub_rn(moved, p[c]);
        p[c] = moved;
    }
}

// The core of a gripper-and-block kind: gripper, block, goal and the two velocities; state_dev [0] grip [n][3], [1] blk [n][3],
// [2] goal [n][3], [3] [n][STRIDE] whose first six columns are the gripper's velocity, then the block's (a kind keeps what else it
// has behind them).  The observation's common columns: [0:3] = grip, [6:9] = gvel, [12:15] = blk, [18:21] = blk - grip,
// [21:24] = bvel, zero elsewhere;  ag = blk;  g = goal.  No constructor and no initialiser: the kernels keep the structs in LDS.
template <int STRIDE>
struct GripBlockEnvDev {
    static_assert(STRIDE >= 6, "array 3 starts with the two velocities");
    double grip[3], blk[3], goal[3], gvel[3], bvel[3];

    // the placement half of a rejection reset: block on the table, goal, gripper at its start, velocities zero
    __device__ __forceinline__ void place(double bx, double by, double table_z, double gx, double gy, double gz, double start_x,
                                          double start_y, double start_z) {
        blk[0] = bx; blk[1] = by; blk[2] = table_z;
        goal[0] = gx; goal[1] = gy; goal[2] = gz;
        grip[0] = start_x; grip[1] = start_y; grip[2] = start_z;
#pragma unroll
        for (int c = 0; c < 3; ++c) gvel[c] = bvel[c] = 0.0;
    }
    __device__ __forceinline__ void load(const hp_env_desc &d, long long i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            grip[c] = d.state_dev[0][3 * i + c];
            blk[c] = d.state_dev[1][3 * i + c];
            goal[c] = d.state_dev[2][3 * i + c];
            gvel[c] = d.state_dev[3][STRIDE * i + c];
            bvel[c] = d.state_dev[3][STRIDE * i + 3 + c];
        }
    }
    __device__ __forceinline__ void store(const hp_env_desc &d, long long i) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            d.state_dev[0][3 * i + c] = grip[c];
            d.state_dev[1][3 * i + c] = blk[c];
            d.state_dev[2][3 * i + c] = goal[c];
            d.state_dev[3][STRIDE * i + c] = gvel[c];
            d.state_dev[3][STRIDE * i + 3 + c] = bvel[c];
        }
    }
    template <int OBS>
    __device__ __forceinline__ void observe(double *obs, double *ag, double *g) const {
#pragma unroll
        for (int c = 0; c < OBS; ++c) obs[c] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            obs[c] = grip[c];
            obs[6 + c] = gvel[c];
            obs[12 + c] = blk[c];
            obs[18 + c] = __dsub_rn(blk[c], grip[c]);
            obs[21 + c] = bvel[c];
            ag[c] = blk[c];
            g[c] = goal[c];
        }
    }
};

// device_env.PointMassVecEnv (the tensor twin of synthetic.PointMassGoalEnv), operation for operation:
//     a = clamp(float64(action), -0.5, 0.5);  scaled = step_scale * a[0:3];  new = clamp(pos + scaled, 0, 0.5);  vel = new - pos
//     obs = zeros(27) with [0:3] = pos, [3:6] = vel, [12:15] = pos;  ag = pos;  g = goal
//     is_success = sqrt(dx dx + dy dy + dz dz) < distance_threshold, products, sums (left to right) and root rounded one by one
//     reset: pos = rs.uniform(0, 0.5, 3); goal = rs.uniform(0, 0.5, 3); vel = 0 -- two numpy calls of three values are the twelve
//     words of one draw of six
// params: [0] step_scale, [1] distance_threshold;  state_dev: [0] pos [n][3], [1] vel [n][3], [2] goal [n][3]
struct PointMassEnvDev {
    static constexpr int OBS = 27, GOAL = 3, ACT = 4, RESET_DRAWS = 6, STATE_ARRAYS = 3;
    double pos[3], vel[3], goal[3], step_scale, threshold;

    static __device__ __forceinline__ void reset_bounds(int, double &low, double &range) {
        low = 0.0;
        range = 0.5;   // numpy: high - low
    }
    __device__ __forceinline__ void reset(const double *u) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            pos[c] = u[c];
            goal[c] = u[3 + c];
            vel[c] = 0.0;
        }
    }

    __device__ __forceinline__ void load(const hp_env_desc &d, long long i) {
        step_scale = d.params[0];
        threshold = d.params[1];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            pos[c] = d.state_dev[0][3 * i + c];
            vel[c] = d.state_dev[1][3 * i + c];
            goal[c] = d.state_dev[2][3 * i + c];
        }
    }
    __device__ __forceinline__ void observe(double *obs, double *ag, double *g) const {
#pragma unroll
        for (int c = 0; c < OBS; ++c) obs[c] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            obs[c] = pos[c];
            obs[3 + c] = vel[c];
            obs[12 + c] = pos[c];
            ag[c] = pos[c];
            g[c] = goal[c];
        }
    }
    template <class A>
    __device__ __forceinline__ void step_with(const A *action) {
        const double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.5, 0.5, 0.5};
        env_clipped_move(pos, vel, action, step_scale, lo, hi);
    }
    __device__ __forceinline__ void step(const float *action) { step_with(action); }
    __device__ __forceinline__ void step(const double *action) { step_with(action); }
    __device__ __forceinline__ bool is_success() const { return env_within(pos, goal, threshold); }
    __device__ __forceinline__ void store(const hp_env_desc &d, long long i) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            d.state_dev[0][3 * i + c] = pos[c];
            d.state_dev[1][3 * i + c] = vel[c];
            d.state_dev[2][3 * i + c] = goal[c];
        }
    }
};

// device_env.PushBlockVecEnv (the tensor twin of synthetic.PushBlockGoalEnv), operation for operation: a kinematic planar push.
// The achieved goal is a block (a square of half width r resting on the table) that moves only while the gripper touches it:
//     a = clamp(float64(action), -0.5, 0.5), a[3] ignored;  new = clamp(grip + step_scale * a[0:3], lo, hi);  gvel = new - grip
//     dx = blk.x - grip.x, dy = blk.y - grip.y;  contact = grip.z < z_touch and |dx| < r and |dy| < r
//     contact: px = r - |dx|, py = r - |dy|;  px <= py ? blk.x = grip.x + (dx >= 0 ? r : -r) : blk.y = grip.y + (dy >= 0 ? r : -r),
//              then blk.x, blk.y clamped into the workspace;  bvel = blk_new - blk_old (zero without contact)
//     obs = zeros(27) with [0:3] = grip, [6:9] = gvel, [12:15] = blk, [18:21] = blk - grip, [21:24] = bvel;  ag = blk;  g = goal
//     is_success: the point mass's, between block and goal
//     reset: at most 100 attempts of bx = uniform(0.15, 0.35), by = uniform(0.2, 0.5), gx = uniform(0.0, 0.35), gy = uniform(0.2, 0.5),
//     accepted when sqrt(ddx ddx + ddy ddy) >= min_separation (bmirobot_env_push_F.py:117-132); the last attempt is kept
// No division and no square root inside step: adds, subtracts, multiplies, compares and clamps only.
// params: [0] step_scale, [1] distance_threshold, [2] half_width r, [3] z_touch, [4] min_separation, [5] table_z, [6], [7] gripper
// start x, y;  state_dev: [0] grip [n][3], [1] blk [n][3], [2] goal [n][3], [3] velocities [n][6] (gripper, then block)
struct PushBlockEnvDev : GripBlockEnvDev<6> {
    static constexpr int OBS = 27, GOAL = 3, ACT = 4, RESET_DRAWS = 4, RESET_ATTEMPTS = 100, STATE_ARRAYS = 4;
    // the workspace: x, y of gripper and block; the gripper's z runs from the table to Z_HI and starts at START_Z
    static constexpr double X_LO = 0.0, X_HI = 0.5, Y_LO = 0.0, Y_HI = 0.7, Z_HI = 0.5, START_Z = 0.3;
    double step_scale, threshold, r, z_touch, min_sep, table_z, start_x, start_y;

    static __device__ __forceinline__ void reset_bounds(int k, double &low, double &range) {
        // numpy: low + (high - low) * next_double, the difference in float64 (0.35 - 0.15 is not 0.2)
        constexpr double lo[4] = {0.15, 0.2, 0.0, 0.2}, hi[4] = {0.35, 0.5, 0.35, 0.5};
        low = lo[k];
        range = hi[k] - lo[k];
    }
    __device__ __forceinline__ bool reset(const double *u) {
        const double d = __dsqrt_rn(tr_sq_distance(u, u + 2, 2));   // block (u[0], u[1]) against goal (u[2], u[3])
        place(u[0], u[1], table_z, u[2], u[3], table_z, start_x, start_y, START_Z);
        return d >= min_sep;
    }

    __device__ __forceinline__ void load(const hp_env_desc &d, long long i) {
        step_scale = d.params[0]; threshold = d.params[1]; r = d.params[2]; z_touch = d.params[3];
        min_sep = d.params[4]; table_z = d.params[5]; start_x = d.params[6]; start_y = d.params[7];
        GripBlockEnvDev::load(d, i);
    }
    __device__ __forceinline__ void observe(double *obs, double *ag, double *g) const { GripBlockEnvDev::observe<OBS>(obs, ag, g); }
    template <class A>
    __device__ __forceinline__ void step_with(const A *action) {
        const double lo[3] = {X_LO, Y_LO, table_z}, hi[3] = {X_HI, Y_HI, Z_HI};
        env_clipped_move(grip, gvel, action, step_scale, lo, hi);
        const double dx = __dsub_rn(blk[0], grip[0]), dy = __dsub_rn(blk[1], grip[1]);
        const double adx = fabs(dx), ady = fabs(dy);
        const double ox = blk[0], oy = blk[1];
        if (grip[2] < z_touch && adx < r && ady < r) {
            const double px = __dsub_rn(r, adx), py = __dsub_rn(r, ady);   // how deep the gripper is inside the block, per axis
            if (px <= py) blk[0] = __dadd_rn(grip[0], dx >= 0.0 ? r : -r);  // out along the axis of least penetration
            else blk[1] = __dadd_rn(grip[1], dy >= 0.0 ? r : -r);
            blk[0] = fmin(fmax(blk[0], X_LO), X_HI);
            blk[1] = fmin(fmax(blk[1], Y_LO), Y_HI);
        }
        bvel[0] = __dsub_rn(blk[0], ox);
        bvel[1] = __dsub_rn(blk[1], oy);
        bvel[2] = 0.0;                       // blk.z stays table_z
    }
    __device__ __forceinline__ void step(const float *action) { step_with(action); }
    __device__ __forceinline__ void step(const double *action) { step_with(action); }
    __device__ __forceinline__ bool is_success() const { return env_within(blk, goal, threshold); }
};

// device_env.PickPlaceVecEnv (the tensor twin of synthetic.PickPlaceGoalEnv), operation for operation: a kinematic pick-and-place.
// The achieved goal is a cube of half width r that moves only in a closed hand; the finger pads sit at grip + TOOL:
//     a = clamp(float64(action), -0.5, 0.5), all four;  inside(grip) = |blk - (grip + TOOL)| < r on every axis
//     near = held or inside(grip):  a[3] = -1  (the finger lock of bmirobot_env_pickandplace_v2.py:93-95, behind the clip)
//     f_old = finger;  finger = clamp(finger + finger_scale * a[3], 0, FINGER_MAX)
//     new = clamp(grip + step_scale * a[0:3], lo, hi);  gvel = new - grip;  grip = new
//     held: blk = clamp(blk + gvel, lo, hi);  otherwise inside(new) and f_old > GRASP_WIDTH and finger <= GRASP_WIDTH: held = 1
//     (the block stays where it is in the step of the grasp; the lock keeps a held block's fingers closing: a grasp never opens)
//     bvel = blk_new - blk_old
//     obs = zeros(27) with [0:3] = grip, [6:9] = gvel, [9] = finger, [10] = held, [12:15] = blk, [18:21] = blk - grip,
//     [21:24] = bvel;  ag = blk;  g = goal;  is_success: the push block's
//     reset: at most 100 attempts of bx = uniform(0.15, 0.35), by = uniform(0.2, 0.5), gx = uniform(0.0, 0.35),
//     gy = uniform(0.3, 0.55), gz = uniform(0.3, 0.5), accepted when sqrt(ddx ddx + ddy ddy + ddz ddz) >= min_separation with
//     ddz = table_z - gz (:116-131 without the orientation draws); the last attempt is kept.  Five bounds, all different: five
//     one-value calls of env_reset_draw
// No division and no square root inside step.
// params: [0] step_scale, [1] distance_threshold, [2] half_width r, [3] finger_scale, [4] min_separation, [5] table_z, [6], [7]
// gripper start x, y;  state_dev: [0] grip [n][3], [1] blk [n][3], [2] goal [n][3], [3] [n][8] = gripper velocity, block velocity,
// finger opening, held (0.0 or 1.0)
struct PickPlaceEnvDev : GripBlockEnvDev<8> {
    static constexpr int OBS = 27, GOAL = 3, ACT = 4, RESET_DRAWS = 5, RESET_ATTEMPTS = 100, STATE_ARRAYS = 4;
    // the workspace of gripper and block alike (z from the table to Z_HI); the gripper starts at START_Z
    static constexpr double X_LO = 0.0, X_HI = 0.5, Y_LO = 0.0, Y_HI = 0.7, Z_HI = 0.6, START_Z = 0.3;
    // the finger pads relative to the gripper; the widest opening; the opening at and below which the fingers hold the cube
    static constexpr double TOOL_X = 0.0, TOOL_Y = 0.05, TOOL_Z = -0.05, FINGER_MAX = 0.08, GRASP_WIDTH = 0.04;
    double finger, held;
    double step_scale, threshold, r, finger_scale, min_sep, table_z, start_x, start_y;

    static __device__ __forceinline__ void reset_bounds(int k, double &low, double &range) {
        constexpr double lo[5] = {0.15, 0.2, 0.0, 0.3, 0.3}, hi[5] = {0.35, 0.5, 0.35, 0.55, 0.5};
        low = lo[k];
        range = hi[k] - lo[k];
    }
    __device__ __forceinline__ bool reset(const double *u) {
        const double ddx = __dsub_rn(u[0], u[2]), ddy = __dsub_rn(u[1], u[3]), ddz = __dsub_rn(table_z, u[4]);
        // tr_sq_distance's order, written out: the block's z is table_z, not a draw, so the operands are not two contiguous vectors
        const double d = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(ddx, ddx), __dmul_rn(ddy, ddy)), __dmul_rn(ddz, ddz)));
        place(u[0], u[1], table_z, u[2], u[3], u[4], start_x, start_y, START_Z);
        finger = held = 0.0;
        return d >= min_sep;
    }

    __device__ __forceinline__ void load(const hp_env_desc &d, long long i) {
        step_scale = d.params[0]; threshold = d.params[1]; r = d.params[2]; finger_scale = d.params[3];
        min_sep = d.params[4]; table_z = d.params[5]; start_x = d.params[6]; start_y = d.params[7];
        GripBlockEnvDev::load(d, i);
        finger = d.state_dev[3][8 * i + 6];
        held = d.state_dev[3][8 * i + 7];
    }
    __device__ __forceinline__ void observe(double *obs, double *ag, double *g) const {
        GripBlockEnvDev::observe<OBS>(obs, ag, g);
        obs[9] = finger;
        obs[10] = held;
    }
    // every finger pad coordinate is less than r from the block centre
    __device__ __forceinline__ bool pads_inside() const {
        return fabs(__dsub_rn(blk[0], __dadd_rn(grip[0], TOOL_X))) < r && fabs(__dsub_rn(blk[1], __dadd_rn(grip[1], TOOL_Y))) < r &&
               fabs(__dsub_rn(blk[2], __dadd_rn(grip[2], TOOL_Z))) < r;
    }
    template <class A>
    __device__ __forceinline__ void step_with(const A *action) {
        const double lo[3] = {X_LO, Y_LO, table_z}, hi[3] = {X_HI, Y_HI, Z_HI};
        double a3 = fmin(fmax((double)action[3], -0.5), 0.5);
        if (held != 0.0 || pads_inside()) a3 = -1.0;         // the finger lock, on the state before the move
        const double f_old = finger;
        finger = fmin(fmax(__dadd_rn(finger, __dmul_rn(finger_scale, a3)), 0.0), FINGER_MAX);
        env_clipped_move(grip, gvel, action, step_scale, lo, hi);
        if (held != 0.0) {                                   // carried: the gripper's clipped displacement, clipped again
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double carried = fmin(fmax(__dadd_rn(blk[c], gvel[c]), lo[c]), hi[c]);
                bvel[c] = __dsub_rn(carried, blk[c]);
                blk[c] = carried;
            }
        } else {
            if (pads_inside() && f_old > GRASP_WIDTH && finger <= GRASP_WIDTH) held = 1.0;   // the block moves from the next step on
#pragma unroll
            for (int c = 0; c < 3; ++c) bvel[c] = __dsub_rn(blk[c], blk[c]);
        }
    }
    __device__ __forceinline__ void step(const float *action) { step_with(action); }
    __device__ __forceinline__ void step(const double *action) { step_with(action); }
    __device__ __forceinline__ bool is_success() const { return env_within(blk, goal, threshold); }
    __device__ __forceinline__ void store(const hp_env_desc &d, long long i) const {
        GripBlockEnvDev::store(d, i);
        d.state_dev[3][8 * i + 6] = finger;
        d.state_dev[3][8 * i + 7] = held;
    }
};

// The kernels keep the structs in LDS (EpisodesLds<Env>::env[4]): no constructor runs there, and a base must not change a size
static_assert(std::is_trivially_default_constructible<PointMassEnvDev>::value && sizeof(PointMassEnvDev) == 88, "11 doubles");
static_assert(std::is_trivially_default_constructible<PushBlockEnvDev>::value && sizeof(PushBlockEnvDev) == 184, "15 + 8 doubles");
static_assert(std::is_trivially_default_constructible<PickPlaceEnvDev>::value && sizeof(PickPlaceEnvDev) == 200, "15 + 2 + 8 doubles");

// RESET_ATTEMPTS of a kind, 1 where it declares none
template <class Env, class = void>
struct EnvResetAttempts { static constexpr int value = 1; };
template <class Env>
struct EnvResetAttempts<Env, std::void_t<decltype(Env::RESET_ATTEMPTS)>> { static constexpr int value = Env::RESET_ATTEMPTS; };

// The draws of one reset out of the stream loaded into w, by the row's wave: consecutive draws with the same bounds are one
// mw_draw_uniform call (the point mass: one call of six).  u: RESET_DRAWS doubles of LDS of this wave's own, readable by every
// lane on return.
template <class Env>
__device__ __forceinline__ void env_reset_draw(MwState &w, double *u) {
    static_assert(Env::RESET_DRAWS > 0 && Env::RESET_DRAWS <= MW_THREADS, "one value per lane");
    for (int k = 0; k < Env::RESET_DRAWS;) {
        double low, range;
        Env::reset_bounds(k, low, range);
        int n = 1;
        for (; k + n < Env::RESET_DRAWS; ++n) {
            double l2, r2;
            Env::reset_bounds(k + n, l2, r2);
            if (l2 != low || r2 != range) break;
        }
        mw_draw_uniform(w, low, range, n, [&](int j, double v) { u[k + j] = v; });
        k += n;
    }
    mw_sync();
}

// One whole reset of environment e out of the stream loaded into w, by the row's wave (the caller commits the stream afterwards,
// once): the draws of an attempt, lane 0 builds the state -- and, for a kind with RESET_ATTEMPTS > 1, says through *verdict
// whether the attempt stands; the wave goes round again until one does or the attempts are spent.  e: lane 0's (LDS, or its own
// registers); u: RESET_DRAWS doubles and verdict: one int, both LDS of this wave's own.
template <class Env>
__device__ __forceinline__ void env_reset_run(MwState &w, Env &e, double *u, int *verdict) {
    if constexpr (EnvResetAttempts<Env>::value == 1) {
        env_reset_draw<Env>(w, u);
        if (mw_lane() == 0) e.reset(u);
    } else {
        for (int attempt = 0; attempt < EnvResetAttempts<Env>::value; ++attempt) {
            env_reset_draw<Env>(w, u);
            if (mw_lane() == 0) *verdict = e.reset(u) ? 1 : 0;
            mw_sync();
            const int accepted = __builtin_amdgcn_readfirstlane(*verdict);   // the same int for every lane: a scalar branch
            mw_sync();                       // every lane has read u and the verdict before the next attempt rewrites them
            if (accepted) break;
        }
    }
}
