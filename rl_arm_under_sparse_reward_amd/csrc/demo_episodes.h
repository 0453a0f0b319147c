// demo_episodes.h -- demonstration episodes from a scripted controller: the kernel of hp_demo_episodes as a template over an
// environment kind (env_device.h), its argument block, and the two controllers: the push schedule (get_demo_data_push.py:39-61,
// stated on the host as synthetic.scripted_action) and the pick-and-place schedule (get_demo_data_pick.py:54-67,
// synthetic.pick_scripted_action).  Which one runs is a value of the argument block (DemoArgs::controller), the same for every
// workgroup of a launch: a controller is no property of a kind -- either runs on any kind that keeps the bmirobot layout -- so
// the table of kinds has no column for it and a kind's demo unit still holds ONE kernel.
//
// No policy: the mapping is the stand-alone reset kernel's (k_env_reset) grown by a timestep loop.  Workgroup i is ONE wave and
// owns environment i with reset stream i in an LDS ring for the whole launch; for each wave of the round it draws the reset
// (env_reset_run: a rejection loop stays wave-local), then lane 0 -- the environment lives in its registers -- runs T timesteps
// of observe, controller, step through one row of LDS, and the wave's lanes store each row to the block coalesced.  The stream
// is committed once, by mt_commit's rule, and the state written back once.  Nothing crosses a workgroup.
//
// Like the kernels of rollout_episodes.h this one is instantiated by one unit per kind -- demo_point_mass.hip,
// demo_push_block.hip, units of their own so that the units of the rollout kernels compile what they compiled before -- through
// the explicit instantiation of env_launch_demo<Env>, the third launch of the kind's table row (EnvKind, rollout_episodes.h).
#pragma once
#include "env_device.h"

struct DemoArgs {
    double *b_obs, *b_ag, *b_g, *b_act;   // block arrays, already offset to the launch's first episode
    MtState *reset_st;                    // reset stream of environment 0
    float *success, *step_success;        // [rows], [rows][T]
    int rows, T;                          // rows: episodes of the launch = waves of n_envs environments, the last possibly partial
    int n_envs, waves;
    int controller;                       // DEMO_PUSH: demo_action on `s`; DEMO_PICK: demo_action_pick on `p` (the other is zero)
    hp_demo_script s;
    hp_pick_script p;
    hp_env_desc env;
};
enum { DEMO_PUSH = 0, DEMO_PICK = 1 };

// The controller for timestep `step` = 1 .. T out of the observation row (bmirobot layout: gripper [0:3], block [12:15]) and the
// desired goal: act[0:4], float64, unclipped.  One explicit IEEE operation per rounding of the host statement.
__device__ __forceinline__ void demo_action(const hp_demo_script &S, int step, const double *obs, const double *g, double *act) {
    const double *grip = obs, *b = obs + 12;
    if (step <= S.phase_end[0]) {                                   // :43-44 lift and retreat
#pragma unroll
        for (int c = 0; c < 4; ++c) act[c] = S.lift[c];
    } else {
        // :45-58 -- behind the block, push, to the waypoint, behind the block, push
        const int phase = step <= S.phase_end[1] ? 1 : step <= S.phase_end[2] ? 2 : step <= S.phase_end[3] ? 3 : step <= S.phase_end[4] ? 4 : 5;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double d = __dsub_rn(g[c], b[c]);
            if (phase == 3) act[c] = __dsub_rn(S.waypoint[c], grip[c]);
            else if (phase == 1 || phase == 4) act[c] = __dsub_rn(__dadd_rn(__dmul_rn(d, S.behind), b[c]), grip[c]);
            else act[c] = d;
        }
        act[3] = 0.0;
    }
    // :59-61 the stop rule, on top of every phase
    if (env_within(b, g, S.stop_radius)) {
#pragma unroll
        for (int c = 0; c < 4; ++c) act[c] = 0.0;
    }
}

// The pick-and-place controller (get_demo_data_pick.py:54-67, synthetic.pick_scripted_action) for timestep `step` = 1 .. T, out
// of the same two places of the observation row: act[0:4], float64, unclipped.  No stop rule.  The offset is added also where it
// is 0.0, as the host statement adds it.
__device__ __forceinline__ void demo_action_pick(const hp_pick_script &S, int step, const double *obs, const double *g, double *act) {
    const double *grip = obs, *b = obs + 12;
    const int phase = step <= S.phase_end[0] ? 0 : step <= S.phase_end[1] ? 1 : step <= S.phase_end[2] ? 2 : step <= S.phase_end[3] ? 3 :
                      step <= S.phase_end[4] ? 4 : 5;
    if (phase == 0) {                                               // :54-55 lift and retreat
#pragma unroll
        for (int c = 0; c < 4; ++c) act[c] = S.lift[c];
    } else if (phase == 2 || phase == 4) {                          // :59-60 open the fingers, :64-65 close them
        act[0] = act[1] = act[2] = 0.0;
        act[3] = phase == 2 ? S.open : -S.open;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (phase == 5) act[c] = __dsub_rn(g[c], b[c]);        // :66-67 carry the block to the goal
            else act[c] = __dadd_rn(__dsub_rn(b[c], grip[c]), phase == 1 ? S.approach[c] : S.grasp[c]);   // :56-58, :61-63
        }
        act[3] = 0.0;
    }
}

// LDS: the ring (9984 bytes) + the reset's values + one row of OBS + 2 GOAL + ACT doubles (296 bytes): about 10 KB, so the
// workgroups of a CU are bounded by its wave slots, not by LDS.  Environment i takes part in wave w if w * n_envs + i < rows
// (workgroup-uniform: the workgroup is the wave); past that it draws nothing and its state stays what its last episode left.
template <class Env>
__global__ __launch_bounds__(MW_THREADS) void k_demo_episodes(const DemoArgs A) {
    constexpr int OD = Env::OBS, GD = Env::GOAL, AD = Env::ACT, PER = OD + 2 * GD + AD;
    __shared__ uint32_t ring[4][MT_N];
    __shared__ double u[Env::RESET_DRAWS > 0 ? Env::RESET_DRAWS : 1];
    __shared__ double row[PER];              // obs | ag | g | action of the timestep
    __shared__ int verdict;
    if constexpr (Env::RESET_DRAWS > 0) {
        static_assert(OD >= 15 && GD == 3 && AD == 4, "the controller reads the bmirobot layout and writes four components");
        const long long i = blockIdx.x;      // < min(rows, n_envs): every workgroup has an episode in wave 0
        const int lane = mw_lane(), T = A.T;
        MtState *st = A.reset_st + i;
        MwState w(st, ring);
        Env e;
        if (lane == 0) e.load(A.env, i);
        double *ag = row + OD, *g = row + OD + GD, *act = row + OD + 2 * GD;
        for (int wv = 0; wv < A.waves; ++wv) {
            const long long ep = (long long)wv * A.n_envs + i;
            if (ep >= A.rows) break;
            env_reset_run<Env>(w, e, u, &verdict);
            float flag = 0.f;
            for (int t = 0; t < T; ++t) {
                if (lane == 0) {
                    e.observe(row, ag, g);
                    if (A.controller == DEMO_PICK) demo_action_pick(A.p, t + 1, row, g, act);   // workgroup-uniform
                    else demo_action(A.s, t + 1, row, g, act);
                    e.step(act);
                    flag = e.is_success() ? 1.f : 0.f;
                    A.step_success[ep * T + t] = flag;
                }
                mw_sync();
                for (int c = lane; c < PER; c += MW_THREADS) {
                    if (c < OD) A.b_obs[(ep * (T + 1) + t) * OD + c] = row[c];
                    else if (c < OD + GD) A.b_ag[(ep * (T + 1) + t) * GD + (c - OD)] = row[c];
                    else if (c < OD + 2 * GD) A.b_g[(ep * T + t) * GD + (c - OD - GD)] = row[c];
                    else A.b_act[(ep * T + t) * AD + (c - OD - 2 * GD)] = row[c];
                }
                mw_sync();                   // every lane has read the row before lane 0 rewrites it
            }
            if (lane == 0) {
                e.observe(row, ag, g);
                A.success[ep] = flag;
            }
            mw_sync();
            for (int c = lane; c < OD + GD; c += MW_THREADS) {
                if (c < OD) A.b_obs[(ep * (T + 1) + T) * OD + c] = row[c];
                else A.b_ag[(ep * (T + 1) + T) * GD + (c - OD)] = row[c];
            }
            mw_sync();
        }
        w.store(st);
        if (lane == 0) e.store(A.env, i);
    }
}

// one launch of k_demo_episodes<Env> over `blocks` environments; declared in rollout_episodes.h for the kind's table row and
// instantiated explicitly by the kind's demo unit
template <class Env>
hipError_t env_launch_demo(hipStream_t stream, unsigned blocks, const DemoArgs &L) {
    hipLaunchKernelGGL(k_demo_episodes<Env>, dim3(blocks), dim3(MW_THREADS), 0, stream, L);
    return hipGetLastError();
}

// the arguments of the success filter (k_demo_compact, demo_compact.hip) and its one launch, over `episodes` workgroups
struct CompactArgs {
    const double *s_obs, *s_ag, *s_g, *s_act;   // source block arrays, episode 0
    double *d_obs, *d_ag, *d_g, *d_act;         // destination block arrays, episode 0
    const float *success, *s_step;              // [n], [n][T]
    float *d_step;                              // [n_demos][T]
    int n, T, od, gd, ad;
    long long kept, n_demos;
    int *kept_out;
};
hipError_t demo_launch_compact(hipStream_t stream, unsigned episodes, const CompactArgs &A);
