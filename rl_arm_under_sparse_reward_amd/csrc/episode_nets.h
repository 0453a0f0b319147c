// episode_nets.h -- the frame of the four units that run a network over an episode block (episode_q.hip, episode_policy.hip,
// episode_action_grad.hip, episode_bellman.hip; those four include it and nothing else does -- episode_audit.h stays free of the
// slab for episode_stats.hip and episode_returns.hip): the 4-row slab's device functions under one namespace, the row of a flat
// index and the columns of its network input, the argument block every such kernel carries, the refusals every such entry makes
// and the one launch.  So "q is hp_episode_q's bits" holds between the audits because the code is the same code.
#pragma once
#include <cmath>

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wundefined-inline"   // agent_device.h declares the 32-row engine's fragment map, which no code here calls
#include "agent_device.h"
#pragma clang diagnostic pop

// the 4-row slab's device functions (no kernel of slab8.h is compiled in these units).  S8_NRG STAYS DEFINED behind this header:
// code written in the slab height's macros (S8_ROWS, S8_RPW), like the functions of slab8.h, needs it -- critic_action_grad_slab
// (episode_action_grad.hip) is such code -- and no unit that includes this header includes slab8.h at another height
#define S8_DEVICE_ONLY
#define S8_NRG 1
#define S8_NS s8en
#include "slab8.h"
#undef S8_NS
#undef S8_DEVICE_ONLY

#include "episode_audit.h"
#include "policy_call.h"

// ---- device: a row and its columns ---------------------------------------------------------------------------------------------------
// Flat row m = e T + t; workgroup b owns rows 4b .. 4b+3, so a slab may straddle two episodes.  obs and ag have T + 1 rows per
// episode (step t at e (T + 1) + t, the state after it at + 1), g and actions T (step t at m).
struct EpisodeRow {
    long long m, e;
    int t;
};
__device__ __forceinline__ EpisodeRow episode_row(long long m, int T) {
    const long long e = m / T;
    return EpisodeRow{m, e, (int)(m - e * T)};
}

// Column c < od + gd of a state as it enters a network, by the operations a transition meets on its way into an update (s8_gather):
// clip, subtract, divide, clip in float64, one rounding each (tr_net_input).  obs_row: the state's row of P.obs; goal: the row's goal
__device__ __forceinline__ float episode_state_column(const PolicyArgs &P, long long obs_row, const double *goal, int c) {
    if (c < P.od) return tr_net_input(P.obs[obs_row * P.od + c], P.clip_obs, P.onz->mean[c], P.onz->std[c], P.clip_o);
    const int j = c - P.od;
    return tr_net_input(goal[j], P.clip_obs, P.gnz->mean[j], P.gnz->std[j], P.clip_g);
}

// Column c >= od + gd of the critic's input for the recorded action of row m: the action narrowed to float32 and divided by
// max_action in float32 inside [act_off, act_off + act_dim) (s8_gather, k_pack_scaled_actions), 0 in the padding
__device__ __forceinline__ float episode_action_column(const PolicyArgs &P, const double *act, long long m, int act_off, int c) {
    const int j = c - act_off;
    if (j >= 0 && j < P.act_dim) return (float)act[m * P.act_dim + j] / P.max_action;
    return 0.f;
}

// ---- host: the argument block, the refusals, the launch -----------------------------------------------------------------------------
// what every kernel of the four carries, its own pointers behind it
struct EpisodeNetArgs {
    PolicyArgs P;                  // the parameter set, the normalizers, obs / g at the first episode (indexed by the kernels), rows = n T
    NetLayout lc;
    int T, act_off, ca;            // the critic's segment starts at ca = la.total
};

// the rows of a call: a plain entry's arrays, or a block's at its first episode with the block's dimensions
struct EpisodeRows {
    const double *obs, *ag, *g, *act;
    int od, gd, ad;                // -1: a plain entry, which has no dimensions of its own
    int64_t n;
    int32_t T;
};

// What an entry checks of its handles behind its own null check and its HP_SERIALISE.  A plain entry: one context for all
static inline int episode_one_context(const char *entry, const hp_agent *a, const hp_norm *on, const hp_norm *gn) {
    HP_REQUIRE(on->ctx == a->ctx && gn->ctx == a->ctx, HP_ERR_INVALID, "%s: handles belong to different contexts", entry);
    return HP_OK;
}
// a *_block entry: one context for all, then R = the rows of episodes [first, first + n) of the block, refused when they leave it
static inline int episode_block_rows(const char *entry, const hp_rollout *ro, const hp_agent *a, const hp_norm *on, const hp_norm *gn,
                                     int64_t first, int64_t n, EpisodeRows &R) {
    HP_REQUIRE(a->ctx == ro->ctx && on->ctx == ro->ctx && gn->ctx == ro->ctx, HP_ERR_INVALID, "%s: handles belong to different contexts",
               entry);
    RolloutArrays at;
    HP_TRY(episode_block_range(entry, ro, first, n, at));
    R = EpisodeRows{at.b_obs, at.b_ag, at.b_g, at.b_act, ro->od, ro->gd, ro->ad, n, ro->T};
    return HP_OK;
}

// The refusals every entry shares behind the agent's shape, in their order -- the normalizers' sizes against `input` (the word
// the entry's message uses for a->xdim's network), the block's dimensions, n and T (and goal_dim where the entry reads goals
// itself: `goal_dim`, else 1), the launch's bound -- then the fill of the base: everything but the kernel's own pointers
static inline int episode_net_rows(const char *entry, const hp_agent *a, const hp_norm *on, const hp_norm *gn, const char *input,
                                   const SlabNetPtrs &net, const EpisodeRows &R, int32_t goal_dim, double clip_obs, EpisodeNetArgs &A) {
    HP_REQUIRE(on->size + gn->size == a->xdim, HP_ERR_INVALID, "%s: normalizer sizes %d+%d do not match the %s input %d", entry,
               (int)on->size, (int)gn->size, input, a->xdim);
    HP_REQUIRE(R.od < 0 || (R.od == on->size && R.gd == gn->size && R.ad == a->cfg.act_dim), HP_ERR_INVALID,
               "%s: the block has dimensions %d / %d / %d, normalizers and agent have %d / %d / %d", entry, R.od, R.gd, R.ad,
               (int)on->size, (int)gn->size, a->cfg.act_dim);
    HP_TRY(episode_check_shape(entry, R.n, R.T, goal_dim));
    const long long rows = (long long)R.n * R.T;
    HP_REQUIRE(rows < (1LL << 31), HP_ERR_INVALID, "%s: %lld steps are more than one launch holds (2^31)", entry, rows);
    A.P = policy_args(a, net, norm_view(on), norm_view(gn), clip_or_inf(clip_obs), rows);
    A.P.obs = R.obs; A.P.g = R.g;
    A.lc = a->lc; A.T = R.T; A.act_off = a->act_off; A.ca = a->la.total;
    return HP_OK;
}

// the same behind the agent's shape, for an entry that refuses nothing in between (hp_episode_action_grad* does: the missing
// dX-order fragments)
static inline int episode_net_args(const char *entry, const hp_agent *a, const hp_norm *on, const hp_norm *gn, const char *input,
                                   const SlabNetPtrs &net, const EpisodeRows &R, int32_t goal_dim, double clip_obs, EpisodeNetArgs &A) {
    HP_TRY(require_slab_shaped(entry, a, HP_ERR_STATE));
    return episode_net_rows(entry, a, on, gn, input, net, R, goal_dim, clip_obs, A);
}

// the one launch: a 4-row slab per workgroup, one workgroup per CU.  Args::Lds is the type of the kernel's __shared__ block: the
// argument block names it once, for the kernel's declaration and for this bound
template <class Args>
static inline int episode_net_launch(void (*kernel)(const Args), const hp_agent *a, const Args &A) {
    static_assert(sizeof(typename Args::Lds) <= 160 * 1024, "the slab's LDS fits a CU");
    hipLaunchKernelGGL(kernel, dim3((unsigned)(((long long)A.P.rows + 3) / 4)), dim3(S8_THREADS), 0, a->ctx->stream, A);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}
