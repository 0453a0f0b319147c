// episode_audit.h -- the frame the six units of the episode audit share (episode_stats.hip and episode_returns.hip directly; episode_q.hip,
// episode_policy.hip, episode_action_grad.hip and episode_bellman.hip through episode_nets.h, which adds what running a network over a
// block takes): the bound on episodes and steps, the refusals every entry makes of a block's shape, the range check of the
// *_block entries with the block's four arrays behind it, the walk that turns an episode's steps into its columns, and the summary
// of a per-episode table.  No slab here.  The arithmetic of a step: transition_device.h.
#pragma once
#include "transition_device.h"

#define HP_EPISODE_MAX (1 << 24)   // episodes of one call (exclusive) and steps of one episode (inclusive)
static_assert(HP_EPISODE_MAX_GOAL_DIM == NORM_MAX, "a goal is as wide as a normalizer can hold");
constexpr int EPISODE_COLS = 6;    // columns of a per-episode table and of its summary
static_assert(HP_EPISODE_STATS == EPISODE_COLS && HP_EPISODE_SUMMARY == EPISODE_COLS && HP_CRITIC_STATS == EPISODE_COLS &&
              HP_POLICY_STATS == EPISODE_COLS && HP_BELLMAN_STATS == EPISODE_COLS, "one summary loop");

// n_episodes, T, goal_dim, refused in this order under the entry's name (the entries of episode_q.hip and episode_policy.hip
// take no goal_dim of their own -- theirs is the goal normalizer's, or none -- and leave it out)
static inline int episode_check_shape(const char *entry, int64_t n, int32_t T, int32_t gd = 1) {
    HP_REQUIRE(n >= 1 && n < HP_EPISODE_MAX, HP_ERR_INVALID, "%s: n_episodes %lld outside [1, %d)", entry, (long long)n, HP_EPISODE_MAX);
    HP_REQUIRE(T >= 1 && T <= HP_EPISODE_MAX, HP_ERR_INVALID, "%s: T %d outside [1, %d]", entry, (int)T, HP_EPISODE_MAX);
    HP_REQUIRE(gd >= 1 && gd <= HP_EPISODE_MAX_GOAL_DIM, HP_ERR_INVALID, "%s: goal_dim %d outside [1, %d]", entry, (int)gd,
               HP_EPISODE_MAX_GOAL_DIM);
    return HP_OK;
}

// episodes [first, first + n) of a rollout block: refused when they leave it, else the block's arrays at `first`
struct RolloutArrays { const double *b_obs, *b_ag, *b_g, *b_act; };
static inline int episode_block_range(const char *entry, const hp_rollout *ro, int64_t first, int64_t n, RolloutArrays &at) {
    HP_REQUIRE(first >= 0 && n >= 1 && first <= ro->n && n <= ro->n - first, HP_ERR_INVALID, "%s: episodes [%lld, %lld) outside the block of %lld",
               entry, (long long)first, (long long)(first + n), (long long)ro->n);
    rollout_arrays_at(ro, first, at);
    return HP_OK;
}

// The columns of one episode out of its per-step arrays (k_episode_policy_stats, k_episode_signal_stats, k_episode_bellman_stats):
// one wave per episode, T a run-time value walked in chunks of 64 steps as k_episode_returns walks it, here from the first chunk
// up.  The lanes form their steps' terms side by side -- terms(t, s, c): step t's NS float64 terms and NC integer ones, preset to
// 0 -- then the sums over t run wave-uniformly over the chunk in ascending t, step base + i taking its terms out of lane i
// (v_readlane: no LDS, no barrier), one __dadd_rn per column per step.  Float64 sums of values that are not small integers depend
// on that order; the twins (synthetic.episode_policy_stats, episode_signal_stats, episode_bellman_stats) are the same loop.  The
// counts are exact whatever the order.  Every lane returns with the same sums.
template <int NS, int NC, class Terms>
__device__ __forceinline__ void episode_column_walk(int T, double (&sum)[NS], long long (&count)[NC], Terms terms) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NS; ++k) sum[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) count[k] = 0;
    for (int base = 0; base < T; base += 64) {
        const int cnt = T - base < 64 ? T - base : 64;
        double s[NS];
        int c[NC];
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] = 0.0;
#pragma unroll
        for (int k = 0; k < NC; ++k) c[k] = 0;
        if (lane < cnt) terms(base + lane, s, c);
        for (int i = 0; i < cnt; ++i) {
#pragma unroll
            for (int k = 0; k < NS; ++k) sum[k] = __dadd_rn(sum[k], lane_read_d(s[k], i));
#pragma unroll
            for (int k = 0; k < NC; ++k) count[k] += __builtin_amdgcn_readlane(c[k], i);
        }
    }
}

// Summary of a table [n][EPISODE_COLS] into out[EPISODE_COLS]: one wave, and lane 0 walks the rows -- every mean is the left-to-right float64 sum in
// episode order divided by n.  A fixed order on purpose (float64 means of distances depend on it; the host twins in synthetic are
// the same loop), not numpy's pairwise mean.  term(r, k) is what row r adds to column k.
template <class Term>
__device__ __forceinline__ void episode_summary_body(const double *__restrict__ table, long long n, double *__restrict__ out, Term term) {
    if (threadIdx.x != 0) return;
    double sum[EPISODE_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long e = 0; e < n; ++e) {
        const double *r = table + e * EPISODE_COLS;
#pragma unroll
        for (int k = 0; k < EPISODE_COLS; ++k) sum[k] = __dadd_rn(sum[k], term(r, k));
    }
    const double dn = (double)n;
#pragma unroll
    for (int k = 0; k < EPISODE_COLS; ++k) out[k] = __ddiv_rn(sum[k], dn);
}

// the entry of a summary: hp_episode_stats_summary, hp_episode_critic_summary, hp_episode_policy_summary, hp_episode_signal_summary,
// hp_episode_bellman_summary
static inline int episode_summary_launch(const char *entry, hp_ctx *ctx, void (*kernel)(const double *, long long, double *),
                                         const double *table, int64_t n, double *out) {
    HP_REQUIRE(ctx && table && out, HP_ERR_INVALID, "%s: null argument", entry);
    CtxGuard guard(ctx);
    HP_REQUIRE(n >= 1, HP_ERR_INVALID, "%s: n_episodes %lld is not positive", entry, (long long)n);
    hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, ctx->stream, table, (long long)n, out);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}
