// episode_returns.hip -- the discounted return every step of an episode block went on to collect, and the critic's Q beside it
// (hp_episode_returns, hp_episode_returns_block, hp_episode_critic_summary; hp_episode_policy_summary, hp_episode_signal_summary and
// hp_episode_bellman_summary are the same kernel).  For
// most of a sparse-reward run the success rate is zero; whether Q(s_t, a_t) (episode_q.hip) tracks G_t, sits on the target
// clip -1 / (1 - gamma) (ddpg_agent.py:259-260) or overestimates is what says that learning is happening.
//
// Step t = 0 .. T-1 of an episode compares ag[t + 1] with g[t]; s[t] is the squared distance (tr_sq_distance,
// transition_device.h) and the reward is compute_reward's in float64 (hp_reward64 there).
//   G_T = +0.0 (tail 0)  or  r[T-1] / (1 - gamma) (tail 1: the last step's reward held for ever, what an infinite-horizon critic is
//   trained towards);   G_t = r[t] + gamma G_{t+1}  for t = T-1 .. 0, every operation rounded on its own.
// The critic columns (HP_CRITIC_STATS) are accumulated in the SAME walk, t = T-1 down to 0, one accumulator per column with Q
// widened to float64: the recursion fixes that order anyway, and a float64 sum of values that are not small integers depends on it
// -- so the host twin (synthetic.episode_returns / episode_critic_stats: plain loops) is compared bit for bit.
#include <cmath>

#include "episode_audit.h"

struct EpisodeReturnsArgs {
    const double *ag, *g;          // [n][T + 1][gd], [n][T][gd], already offset to the first episode
    const float *q;                // [n][T] or nullptr
    double *returns;               // [n][T]
    double *cstats;                // [n][HP_CRITIC_STATS] or nullptr (with q)
    double sq_reward;              // sparse: squared_bound(thr, true); dense: < 0 (hp_reward64's rule)
    double gamma, q_floor;         // q_floor = -1 / (1 - gamma), the target clip (has_floor: gamma < 1)
    int T, gd, tail, has_floor;
};

// k_episode_returns.  One wave per episode.  T is a run-time value (up to 2^24), so the episode is walked in chunks of 64 steps
// from the last chunk down: the lanes form the chunk's 64 rewards side by side (lane l: step base + l; a wave reads one
// contiguous stretch of ag and of g, and 256 contiguous bytes of q), then the recursion -- a dependent chain of one multiply and
// one add per step -- runs wave-uniformly over the chunk, step base + i taking r and Q out of lane i (v_readlane: no LDS, no
// barrier); every lane carries the same G and the same accumulators, lane i keeps G of its own step, and the chunk's returns go
// out as one coalesced store.  Nothing is held per step beyond the chunk: registers only.
__global__ __launch_bounds__(64) void k_episode_returns(const EpisodeReturnsArgs A) {
    const int lane = threadIdx.x, T = A.T, gd = A.gd;
    const long long e = blockIdx.x;
    const double *ag = A.ag + e * ((long long)T + 1) * gd, *g = A.g + e * (long long)T * gd;
    double *ret = A.returns + e * (long long)T;
    const float *q = A.q ? A.q + e * (long long)T : nullptr;
    const double gamma = A.gamma;
    double G = 0.0;
    double sum_q = 0.0, sum_g = 0.0, sum_b = 0.0, sum_a = 0.0, max_a = 0.0;
    int floor_steps = 0;
    bool first = true;
    for (int base = ((T - 1) >> 6) << 6; base >= 0; base -= 64) {
        const int cnt = T - base < 64 ? T - base : 64;
        const int t = base + lane;
        double r = 0.0;
        float qv = 0.f;
        if (lane < cnt) {
            r = hp_reward64(tr_sq_distance(ag + (long long)(t + 1) * gd, g + (long long)t * gd, gd), A.sq_reward);
            if (q) qv = q[t];
        }
        if (first) {
            if (A.tail) G = __ddiv_rn(lane_read_d(r, cnt - 1), __dsub_rn(1.0, gamma));
            first = false;
        }
        double mine = 0.0;
        for (int i = cnt - 1; i >= 0; --i) {
            G = __dadd_rn(lane_read_d(r, i), __dmul_rn(gamma, G));
            mine = (lane == i) ? G : mine;
            if (q) {
                const double qd = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(qv), i));
                const double d = __dsub_rn(qd, G), ad = fabs(d);
                sum_q = __dadd_rn(sum_q, qd);
                sum_g = __dadd_rn(sum_g, G);
                sum_b = __dadd_rn(sum_b, d);
                sum_a = __dadd_rn(sum_a, ad);
                max_a = ad > max_a ? ad : max_a;
                floor_steps += (A.has_floor && qd <= A.q_floor) ? 1 : 0;
            }
        }
        if (lane < cnt) ret[t] = mine;
    }
    if (A.cstats && lane == 0) {
        double *out = A.cstats + e * HP_CRITIC_STATS;
        const double dT = (double)T;
        out[0] = __ddiv_rn(sum_q, dT);
        out[1] = __ddiv_rn(sum_g, dT);
        out[2] = __ddiv_rn(sum_b, dT);
        out[3] = __ddiv_rn(sum_a, dT);
        out[4] = max_a;
        out[5] = (double)floor_steps;
    }
}

// k_episode_column_means (episode_summary_body): the mean of every column of a per-episode table -- the critic's and the policy's
// the actor signal's and the Bellman audit's (synthetic.episode_critic_summary, episode_policy_summary, episode_signal_summary,
// episode_bellman_summary: one loop)
struct ColumnMeanTerm {
    __device__ double operator()(const double *r, int k) const { return r[k]; }
};
__global__ __launch_bounds__(64) void k_episode_column_means(const double *__restrict__ stats, long long n, double *__restrict__ out) {
    episode_summary_body(stats, n, out, ColumnMeanTerm{});
}

static int episode_returns_launch(const char *entry, hipStream_t stream, const double *ag, const double *g, int64_t n, int32_t T,
                                  int32_t gd, double thr, int32_t reward_type, double gamma, int32_t tail, double *returns,
                                  const float *q, double *cstats) {
    HP_TRY(episode_check_shape(entry, n, T, gd));
    HP_REQUIRE(reward_type == 0 || reward_type == 1, HP_ERR_INVALID, "%s: reward_type %d is neither 0 (sparse) nor 1 (dense)", entry,
               (int)reward_type);
    HP_REQUIRE(tail == 0 || tail == 1, HP_ERR_INVALID, "%s: tail %d is neither 0 (zero) nor 1 (persist)", entry, (int)tail);
    HP_REQUIRE(gamma >= 0.0 && gamma <= 1.0, HP_ERR_INVALID, "%s: gamma %g outside [0, 1]", entry, gamma);
    HP_REQUIRE(!(gamma == 1.0 && tail == 1), HP_ERR_INVALID, "%s: gamma 1 with tail 1 (persist) has no finite return", entry);
    HP_REQUIRE((q == nullptr) == (cstats == nullptr), HP_ERR_INVALID, "%s: q_dev and critic_stats_dev come together", entry);
    EpisodeReturnsArgs A;
    A.ag = ag; A.g = g; A.q = q; A.returns = returns; A.cstats = cstats;
    A.sq_reward = reward_type == 0 ? squared_bound(thr, true) : -1.0;
    A.gamma = gamma;
    A.has_floor = gamma < 1.0 ? 1 : 0;
    A.q_floor = A.has_floor ? -(1.0 / (1.0 - gamma)) : 0.0;
    A.T = T; A.gd = gd; A.tail = tail;
    hipLaunchKernelGGL(k_episode_returns, dim3((unsigned)n), dim3(64), 0, stream, A);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

extern "C" {

int hp_episode_returns(hp_ctx *ctx, const double *ag_dev, const double *g_dev, int64_t n_episodes, int32_t T, int32_t goal_dim,
                       double distance_threshold, int32_t reward_type, double gamma, int32_t tail, double *returns_dev,
                       const float *q_dev, double *critic_stats_dev) {
    HP_REQUIRE(ctx && ag_dev && g_dev && returns_dev, HP_ERR_INVALID, "hp_episode_returns: null argument");
    CtxGuard guard(ctx);
    return episode_returns_launch("hp_episode_returns", ctx->stream, ag_dev, g_dev, n_episodes, T, goal_dim, distance_threshold,
                                  reward_type, gamma, tail, returns_dev, q_dev, critic_stats_dev);
}

int hp_episode_returns_block(hp_rollout *ro, int64_t first_episode, int64_t n_episodes, double distance_threshold, int32_t reward_type,
                             double gamma, int32_t tail, double *returns_dev, const float *q_dev, double *critic_stats_dev) {
    HP_REQUIRE(ro && returns_dev, HP_ERR_INVALID, "hp_episode_returns_block: null argument");
    HP_SERIALISE(ro);
    RolloutArrays at;
    HP_TRY(episode_block_range("hp_episode_returns_block", ro, first_episode, n_episodes, at));
    return episode_returns_launch("hp_episode_returns_block", ro->ctx->stream, at.b_ag, at.b_g, n_episodes, ro->T, ro->gd,
                                  distance_threshold, reward_type, gamma, tail, returns_dev, q_dev, critic_stats_dev);
}

int hp_episode_critic_summary(hp_ctx *ctx, const double *critic_stats_dev, int64_t n_episodes, double *summary_dev) {
    return episode_summary_launch("hp_episode_critic_summary", ctx, k_episode_column_means, critic_stats_dev, n_episodes, summary_dev);
}

int hp_episode_policy_summary(hp_ctx *ctx, const double *policy_stats_dev, int64_t n_episodes, double *summary_dev) {
    return episode_summary_launch("hp_episode_policy_summary", ctx, k_episode_column_means, policy_stats_dev, n_episodes, summary_dev);
}

int hp_episode_signal_summary(hp_ctx *ctx, const double *signal_stats_dev, int64_t n_episodes, double *summary_dev) {
    return episode_summary_launch("hp_episode_signal_summary", ctx, k_episode_column_means, signal_stats_dev, n_episodes, summary_dev);
}

int hp_episode_bellman_summary(hp_ctx *ctx, const double *bellman_stats_dev, int64_t n_episodes, double *summary_dev) {
    return episode_summary_launch("hp_episode_bellman_summary", ctx, k_episode_column_means, bellman_stats_dev, n_episodes, summary_dev);
}

}  // extern "C"
