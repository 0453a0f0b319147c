// env_device.h -- environments the library steps itself: the seam of k_rollout_episodes (rollout.hip).
//
// An environment kind is one struct of __device__ functions over the state of ONE environment; the kernel keeps one instance per
// row of its slab in LDS and calls every function from one lane (lane 0 of the row's wave):
//     static constexpr int OBS, GOAL, ACT     dimensions, compared with the block's on the host before the launch
//     load(desc, i)                            state of environment i out of the arrays of hp_env_desc (and the parameters)
//     observe(obs, ag, g)                      write the current observation row [OBS], achieved goal [GOAL], desired goal [GOAL]
//     step(action_f32)                         advance by one timestep with the float32 action [ACT] the policy side produced
//     is_success()                             the `is_success` flag of the state just reached
//     store(desc, i)                           write the state back (every array: a reset on the device changes the goal too)
// A kind that can be reset on the device (hp_env_reset, the wave loop of k_rollout_episodes) also declares
//     static constexpr int RESET_DRAWS         uniform draws of one reset, taken from the environment's own reset stream
//     reset_bounds(k, low, range)              draw k = random_uniform(low, range) = low + range * next_double, in draw order
//     reset(u)                                 the fresh state out of those RESET_DRAWS values
// and RESET_DRAWS = 0 says the kind has no device reset.  The row's wave draws (env_reset_draw below, mw_draw_uniform) and hands the
// values to lane 0 through LDS.
// Every float64 operation whose rounding the host twin of the environment fixes is an explicit IEEE operation (__dmul_rn, ...), so
// that no contraction can change a bit relative to the elementwise torch / numpy ops of that twin.
// Adding a kind: a struct here, an HP_ENV_* constant in rlarm_hip.h and a case in the dispatches of hp_rollout_episodes / hp_rollout_waves
// and hp_env_reset (rollout.hip).
#pragma once
#include "internal.h"
#include "mt19937_wave.h"

// device_env.PointMassVecEnv (the tensor twin of synthetic.PointMassGoalEnv), operation for operation:
//     a = clamp(float64(action), -0.5, 0.5);  scaled = step_scale * a[0:3];  new = clamp(pos + scaled, 0, 0.5);  vel = new - pos
//     obs = zeros(27) with [0:3] = pos, [3:6] = vel, [12:15] = pos;  ag = pos;  g = goal
//     is_success = sqrt(dx dx + dy dy + dz dz) < distance_threshold, products, sums (left to right) and root rounded one by one
//     reset: pos = rs.uniform(0, 0.5, 3); goal = rs.uniform(0, 0.5, 3); vel = 0 -- two numpy calls of three values are the twelve
//     words of one draw of six
// params: [0] step_scale, [1] distance_threshold;  state_dev: [0] pos [n][3], [1] vel [n][3], [2] goal [n][3]
struct PointMassEnvDev {
    static constexpr int OBS = 27, GOAL = 3, ACT = 4, RESET_DRAWS = 6;
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
    __device__ __forceinline__ void step(const float *action) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double a = fmin(fmax((double)action[c], -0.5), 0.5);
            const double scaled = __dmul_rn(step_scale, a);
            const double moved = fmin(fmax(__dadd_rn(pos[c], scaled), 0.0), 0.5);
            vel[c] = __dsub_rn(moved, pos[c]);
            pos[c] = moved;
        }
    }
    __device__ __forceinline__ bool is_success() const {
        const double dx = __dsub_rn(pos[0], goal[0]), dy = __dsub_rn(pos[1], goal[1]), dz = __dsub_rn(pos[2], goal[2]);
        const double s = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
        return __dsqrt_rn(s) < threshold;
    }
    __device__ __forceinline__ void store(const hp_env_desc &d, long long i) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            d.state_dev[0][3 * i + c] = pos[c];
            d.state_dev[1][3 * i + c] = vel[c];
            d.state_dev[2][3 * i + c] = goal[c];
        }
    }
};

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
