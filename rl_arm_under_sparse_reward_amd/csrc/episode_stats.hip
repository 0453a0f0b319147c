// episode_stats.hip -- what an episode block says about its episodes, computed where the block lies (hp_episode_stats,
// hp_episode_stats_block, hp_episode_stats_summary; ddpg_agent.py:280-304 records is_success at every evaluation step and keeps
// the last): return, final and closest goal distance, first successful step, successful steps, final success.
//
// Step t = 0 .. T-1 of an episode compares ag[t + 1] with g[t] (her.py:38, _is_success).  s[t] is the squared distance
// (tr_sq_distance, transition_device.h) and both predicates are taken on s[t] against squared_bound's thresholds, the rule of
// hp_is_success_dev and hp_compute_reward_dev: is_success = s < sq_success, reward = hp_reward(s, sq_reward).  The square root is
// monotone, so min_t d[t] = sqrt(min_t s[t]): an episode takes two square roots, not T.
#include <cmath>

#include "episode_audit.h"

struct EpisodeStatsArgs {
    const double *ag, *g;      // [n][T + 1][gd], [n][T][gd], already offset to the first episode
    double *stats;             // [n][HP_EPISODE_STATS]
    float *step;               // [n][T] or nullptr
    double sq_success, sq_reward;
    int T, gd;
};

// k_episode_stats.  One wave per episode; lane l takes steps l, l + 64, ...  The four reductions across the wave -- a sum of
// rewards that are -1 or -0 (exact integers in float64, started at +0.0 like numpy's add.reduce, so an episode that succeeds at
// every step has return +0.0), a minimum of doubles, a minimum of integers, a sum of integers -- give the same bits in any order, so
// nothing here depends on the mapping: a butterfly over xor 16 .. 1 inside each half of the wave (ds_swizzle), the two halves
// read out of lanes 0 and 32.  That is why the host twin (synthetic.episode_stats) is compared bit for bit, with no tolerance.
// final_distance and final_success belong to step T - 1 alone: the lane that owns it writes them.  Inputs are finite (a NaN
// distance is neither a success nor a minimum here).
__global__ __launch_bounds__(64) void k_episode_stats(const EpisodeStatsArgs A) {
    const int lane = threadIdx.x, T = A.T, gd = A.gd;
    const long long e = blockIdx.x;
    const double *ag = A.ag + e * ((long long)T + 1) * gd, *g = A.g + e * (long long)T * gd;
    double *out = A.stats + e * HP_EPISODE_STATS;
    float *step = A.step ? A.step + e * (long long)T : nullptr;
    double ret = 0.0, smin = INFINITY;
    int first = T, count = 0;
    for (int t = lane; t < T; t += 64) {
        const double s = tr_sq_distance(ag + (long long)(t + 1) * gd, g + (long long)t * gd, gd);
        const bool ok = s < A.sq_success;
        ret = __dadd_rn(ret, (double)hp_reward(s, A.sq_reward));
        smin = s < smin ? s : smin;
        first = (ok && t < first) ? t : first;
        count += ok ? 1 : 0;
        if (step) step[t] = ok ? 1.f : 0.f;
        if (t == T - 1) {
            out[1] = __dsqrt_rn(s);
            out[5] = ok ? 1.0 : 0.0;
        }
    }
#define ES_STAGE(M)                                                              \
    {                                                                            \
        const double r2 = lane_xor_d<M>(ret), m2 = lane_xor_d<M>(smin);          \
        const int f2 = lane_xor_i<M>(first), c2 = lane_xor_i<M>(count);          \
        ret = __dadd_rn(ret, r2); smin = m2 < smin ? m2 : smin;                  \
        first = f2 < first ? f2 : first; count += c2;                            \
    }
    ES_STAGE(16) ES_STAGE(8) ES_STAGE(4) ES_STAGE(2) ES_STAGE(1)
#undef ES_STAGE
    // lanes 0 and 32 hold their halves' results
    const double ret2 = lane_read_d(ret, 32), min2 = lane_read_d(smin, 32);
    const int f_hi = __builtin_amdgcn_readlane(first, 32), c_hi = __builtin_amdgcn_readlane(count, 32);
    if (lane != 0) return;
    ret = __dadd_rn(ret, ret2);
    smin = min2 < smin ? min2 : smin;
    first = f_hi < first ? f_hi : first;
    count += c_hi;
    out[0] = ret;
    out[2] = __dsqrt_rn(smin);
    out[3] = (double)first;
    out[4] = (double)count;
}

// k_episode_stats_summary (episode_summary_body): the means of ret, final_distance, min_distance, first_success, final_success
// and of "the episode had a successful step" (successful_steps > 0), in the order synthetic.episode_stats_summary lists them.
struct StatsSummaryTerm {
    __device__ double operator()(const double *r, int k) const { return k < 4 ? r[k] : k == 4 ? r[5] : (r[4] > 0.0 ? 1.0 : 0.0); }
};
__global__ __launch_bounds__(64) void k_episode_stats_summary(const double *__restrict__ stats, long long n, double *__restrict__ out) {
    episode_summary_body(stats, n, out, StatsSummaryTerm{});
}

static int episode_stats_launch(const char *entry, hipStream_t stream, const double *ag, const double *g, int64_t n, int32_t T,
                                int32_t gd, double thr, double *stats, float *step) {
    HP_TRY(episode_check_shape(entry, n, T, gd));
    EpisodeStatsArgs A;
    A.ag = ag; A.g = g; A.stats = stats; A.step = step;
    A.sq_success = squared_bound(thr, false);
    A.sq_reward = squared_bound(thr, true);
    A.T = T; A.gd = gd;
    hipLaunchKernelGGL(k_episode_stats, dim3((unsigned)n), dim3(64), 0, stream, A);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

int hp_episode_stats(hp_ctx *ctx, const double *ag_dev, const double *g_dev, int64_t n_episodes, int32_t T, int32_t goal_dim,
                     double distance_threshold, double *stats_dev, float *step_success_dev) {
    HP_REQUIRE(ctx && ag_dev && g_dev && stats_dev, HP_ERR_INVALID, "hp_episode_stats: null argument");
    CtxGuard guard(ctx);
    return episode_stats_launch("hp_episode_stats", ctx->stream, ag_dev, g_dev, n_episodes, T, goal_dim, distance_threshold, stats_dev,
                                step_success_dev);
}

int hp_episode_stats_block(hp_rollout *ro, int64_t first_episode, int64_t n_episodes, double distance_threshold, double *stats_dev,
                           float *step_success_dev) {
    HP_REQUIRE(ro && stats_dev, HP_ERR_INVALID, "hp_episode_stats_block: null argument");
    HP_SERIALISE(ro);
    RolloutArrays at;
    HP_TRY(episode_block_range("hp_episode_stats_block", ro, first_episode, n_episodes, at));
    return episode_stats_launch("hp_episode_stats_block", ro->ctx->stream, at.b_ag, at.b_g, n_episodes, ro->T, ro->gd, distance_threshold,
                                stats_dev, step_success_dev);
}

int hp_episode_stats_summary(hp_ctx *ctx, const double *stats_dev, int64_t n_episodes, double *summary_dev) {
    return episode_summary_launch("hp_episode_stats_summary", ctx, k_episode_stats_summary, stats_dev, n_episodes, summary_dev);
}
