// episode_stats.hip -- what an episode block says about its episodes, computed where the block lies (hp_episode_stats,
// hp_episode_stats_block, hp_episode_stats_summary; ddpg_agent.py:280-304 records is_success at every evaluation step and keeps
// the last): return, final and closest goal distance, first successful step, successful steps, final success.
//
// Step t = 0 .. T-1 of an episode compares ag[t + 1] with g[t] (her.py:38, _is_success).  s[t] is the squared distance, products and
// sums rounded one by one and summed left to right over the goal components -- the arithmetic of k_goal_reward (buffer.hip) -- and
// both predicates are taken on s[t] against squared_bound's thresholds, the rule of hp_is_success_dev and hp_compute_reward_dev:
// is_success = s < sq_success, reward = hp_reward(s, sq_reward).  The square root is monotone, so min_t d[t] = sqrt(min_t s[t]):
// an episode takes two square roots, not T.
#include <cmath>

#include "internal.h"

struct EpisodeStatsArgs {
    const double *ag, *g;      // [n][T + 1][gd], [n][T][gd], already offset to the first episode
    double *stats;             // [n][HP_EPISODE_STATS]
    float *step;               // [n][T] or nullptr
    double sq_success, sq_reward;
    int T, gd;
};

// x of lane (i ^ M), M < 32: ds_swizzle in bit-mask mode (the LDS crossbar: no memory, no address register)
template <int M> __device__ __forceinline__ int es_xor_i(int x) { return __builtin_amdgcn_ds_swizzle(x, (M << 10) | 0x1F); }
template <int M> __device__ __forceinline__ double es_xor_d(double x) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)es_xor_i<M>((int)(unsigned)b), hi = (unsigned)es_xor_i<M>((int)(unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

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
        const double *a = ag + (long long)(t + 1) * gd, *b = g + (long long)t * gd;
        double s = 0.0;
        for (int c = 0; c < gd; ++c) {   // numpy add.reduce over < 8 contiguous elements: left to right
            const double d = __dsub_rn(a[c], b[c]);
            const double sq = __dmul_rn(d, d);
            s = (c == 0) ? sq : __dadd_rn(s, sq);
        }
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
        const double r2 = es_xor_d<M>(ret), m2 = es_xor_d<M>(smin);              \
        const int f2 = es_xor_i<M>(first), c2 = es_xor_i<M>(count);              \
        ret = __dadd_rn(ret, r2); smin = m2 < smin ? m2 : smin;                  \
        first = f2 < first ? f2 : first; count += c2;                            \
    }
    ES_STAGE(16) ES_STAGE(8) ES_STAGE(4) ES_STAGE(2) ES_STAGE(1)
#undef ES_STAGE
    // lanes 0 and 32 hold their halves' results
    const long long rb = __double_as_longlong(ret), mb = __double_as_longlong(smin);
    const unsigned r_lo = __builtin_amdgcn_readlane((int)(unsigned)rb, 32), r_hi = __builtin_amdgcn_readlane((int)(unsigned)(rb >> 32), 32);
    const unsigned m_lo = __builtin_amdgcn_readlane((int)(unsigned)mb, 32), m_hi = __builtin_amdgcn_readlane((int)(unsigned)(mb >> 32), 32);
    const int f_hi = __builtin_amdgcn_readlane(first, 32), c_hi = __builtin_amdgcn_readlane(count, 32);
    if (lane != 0) return;
    const double ret2 = __longlong_as_double((long long)(((unsigned long long)r_hi << 32) | r_lo));
    const double min2 = __longlong_as_double((long long)(((unsigned long long)m_hi << 32) | m_lo));
    ret = __dadd_rn(ret, ret2);
    smin = min2 < smin ? min2 : smin;
    first = f_hi < first ? f_hi : first;
    count += c_hi;
    out[0] = ret;
    out[2] = __dsqrt_rn(smin);
    out[3] = (double)first;
    out[4] = (double)count;
}

// k_episode_stats_summary.  One wave, and lane 0 walks the rows: every mean is the left-to-right float64 sum in episode order
// divided by n -- a fixed order on purpose (synthetic.episode_stats_summary is the same loop), not numpy's pairwise mean.
__global__ __launch_bounds__(64) void k_episode_stats_summary(const double *__restrict__ stats, long long n, double *__restrict__ out) {
    if (threadIdx.x != 0) return;
    double sum[HP_EPISODE_SUMMARY] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long e = 0; e < n; ++e) {
        const double *r = stats + e * HP_EPISODE_STATS;
        sum[0] = __dadd_rn(sum[0], r[0]);
        sum[1] = __dadd_rn(sum[1], r[1]);
        sum[2] = __dadd_rn(sum[2], r[2]);
        sum[3] = __dadd_rn(sum[3], r[3]);
        sum[4] = __dadd_rn(sum[4], r[5]);
        sum[5] = __dadd_rn(sum[5], r[4] > 0.0 ? 1.0 : 0.0);
    }
    const double dn = (double)n;
#pragma unroll
    for (int k = 0; k < HP_EPISODE_SUMMARY; ++k) out[k] = __ddiv_rn(sum[k], dn);
}

#define ES_MAX_EPISODES (1 << 24)
static_assert(HP_EPISODE_MAX_GOAL_DIM == NORM_MAX, "a goal is as wide as a normalizer can hold");

static int episode_stats_launch(const char *entry, hipStream_t stream, const double *ag, const double *g, int64_t n, int32_t T,
                                int32_t gd, double thr, double *stats, float *step) {
    HP_REQUIRE(n >= 1 && n < ES_MAX_EPISODES, HP_ERR_INVALID, "%s: n_episodes %lld outside [1, %d)", entry, (long long)n, ES_MAX_EPISODES);
    HP_REQUIRE(T >= 1 && T <= ES_MAX_EPISODES, HP_ERR_INVALID, "%s: T %d outside [1, %d]", entry, (int)T, ES_MAX_EPISODES);
    HP_REQUIRE(gd >= 1 && gd <= HP_EPISODE_MAX_GOAL_DIM, HP_ERR_INVALID, "%s: goal_dim %d outside [1, %d]", entry, (int)gd,
               HP_EPISODE_MAX_GOAL_DIM);
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
    HP_REQUIRE(first_episode >= 0 && n_episodes >= 1 && first_episode <= ro->n && n_episodes <= ro->n - first_episode, HP_ERR_INVALID,
               "hp_episode_stats_block: episodes [%lld, %lld) outside the block of %lld", (long long)first_episode,
               (long long)(first_episode + n_episodes), (long long)ro->n);
    struct { const double *b_obs, *b_ag, *b_g, *b_act; } at;
    rollout_arrays_at(ro, first_episode, at);
    return episode_stats_launch("hp_episode_stats_block", ro->ctx->stream, at.b_ag, at.b_g, n_episodes, ro->T, ro->gd, distance_threshold,
                                stats_dev, step_success_dev);
}

int hp_episode_stats_summary(hp_ctx *ctx, const double *stats_dev, int64_t n_episodes, double *summary_dev) {
    HP_REQUIRE(ctx && stats_dev && summary_dev, HP_ERR_INVALID, "hp_episode_stats_summary: null argument");
    CtxGuard guard(ctx);
    HP_REQUIRE(n_episodes >= 1, HP_ERR_INVALID, "hp_episode_stats_summary: n_episodes %lld is not positive", (long long)n_episodes);
    hipLaunchKernelGGL(k_episode_stats_summary, dim3(1), dim3(64), 0, ctx->stream, stats_dev, (long long)n_episodes, summary_dev);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}
