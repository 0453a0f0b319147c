// episode_bellman.hip -- the quantity the critic is trained on, for every step of an episode block, computed where the block lies
// (hp_episode_bellman, hp_episode_bellman_block): the residual of ddpg_agent.py:249-263,
//   y_t = clamp(r_t + gamma Q'(s_{t+1}, pi'(s_{t+1})), -1 / (1 - gamma), 0),   delta_t = y_t - Q(s_t, a_t),
// for t = 0 .. T-1 of every episode in ONE launch, and the columns that summarise it (hp_episode_bellman_stats; their means,
// hp_episode_bellman_summary, are episode_returns.hip's k_episode_column_means).  The critic audit sets Q beside the return of the
// recorded episode, which belongs to the exploring policy; this sets Q beside the target the update itself bootstraps from -- and
// under a goal the episode went on to achieve (HP_GOAL_FINAL), where hindsight teaches the critic first.
//
// k_episode_bellman runs in the frame of k_episode_policy (episode_policy.hip): flat row m = e T + t, workgroup b owns rows
// 4b .. 4b+3, obs and ag have T + 1 rows per episode, g and actions T, one PolicyLds.  Three network passes per slab with one barrier
// between consecutive ones -- the entry condition of s8_critic_slab: the previous trunk has drained its weight ring and nothing
// reads the LDS any more:
//   1. the TARGET actor (s8_policy_slab) on the next-state rows, obs[e (T + 1) + t + 1] | G(e, t); its emit puts
//      u = (max_action * th) / max_action at act_off, the expression and the place of the actor-side chain; pi' is not stored;
//   2. the TARGET critic (s8_critic_slab) on the same rows, the normalised columns kept as k_episode_policy keeps them: q_next[m].
//      Its emit is one lane per row, and that lane forms the row's reward and target: r = hp_reward of the squared distance between
//      ag[e (T + 1) + t + 1] and G(e, t), y by the two float32 operations of s8_head_bwd_inplace_td (slab8.h) with the agent's own
//      gamma and clip_ret -- so y is an update's target for that row;
//   3. the ONLINE critic on the rows of s_t: obs[e (T + 1) + t] normalised anew, the goal columns kept from pass 1 (the same
//      tr_net_input of the same values, so hp_episode_q's bits), the action (float)act / max_action as k_episode_q forms it: q[m].
// G(e, t) is g[m] (HP_GOAL_DESIRED: the update's rule for g_next = g, ddpg_agent.py:231) or the episode's last achieved goal
// ag[e (T + 1) + T] for every t (HP_GOAL_FINAL: the relabel under which every episode ends in success).
//
// Rows past n T in the last slab take part in every barrier, read nothing (the slabs call the input functions for rows that exist)
// and store nothing.  Which weights: the four buffers episode_q.hip's header names, on the context's stream behind whatever wrote them.
#include "episode_nets.h"

struct EpisodeBellmanArgs : EpisodeNetArgs {   // P.net: the target parameter set
    using Lds = s8en::PolicyLds;
    SlabNetPtrs online;            // the online parameter set
    const double *ag, *act;        // [n][T + 1][gd], [n][T][ad], already offset to the first episode
    float *q, *q_next, *r, *y;     // [n][T] each
    double sq_threshold;           // sparse: squared_bound(thr, true); dense: < 0 (hp_reward's rule)
    float gamma, clip_ret;         // what the agent hands its update kernels
    int goal_mode;
};

__global__ __launch_bounds__(S8_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_episode_bellman(const EpisodeBellmanArgs A) {
    __shared__ EpisodeBellmanArgs::Lds L;
    const long long row0 = (long long)blockIdx.x * 4;
    const PolicyArgs &P = A.P;
    const int T = A.T, gd = P.gd;
    // the goal of a row: the block's own at t, or the episode's last achieved one
    auto goal_of = [&](const EpisodeRow &w) -> const double * {
        return A.goal_mode == HP_GOAL_FINAL ? A.ag + (w.e * (T + 1) + T) * gd : P.g + w.m * gd;
    };
    s8en::s8_policy_slab(P, L, (size_t)row0,
        [&](int r, int c) -> float {
            const EpisodeRow w = episode_row(row0 + r, T);
            return episode_state_column(P, w.e * (T + 1) + w.t + 1, goal_of(w), c);
        },
        [&](int r, int j, float a) { L.xin[r * S8_LDX + A.act_off + j] = a / P.max_action; });   // a = max_action * th: the actor-side chain's u
    s8en::s8_sync();
    s8en::s8_critic_slab(P.net, A.lc, A.ca, P.H, (long long)P.rows, L, (size_t)row0,
        [&](int r, int c) -> float { return L.xin[r * S8_LDX + c]; },
        [&](int r, float qn) {
            const EpisodeRow w = episode_row(row0 + r, T);
            const float rw = hp_reward(tr_sq_distance(A.ag + (w.e * (T + 1) + w.t + 1) * gd, goal_of(w), gd), A.sq_threshold);
            float y = rw + A.gamma * qn;
            y = fminf(fmaxf(y, -A.clip_ret), 0.f);
            A.q_next[w.m] = qn; A.r[w.m] = rw; A.y[w.m] = y;
        });
    s8en::s8_sync();
    s8en::s8_critic_slab(A.online, A.lc, A.ca, P.H, (long long)P.rows, L, (size_t)row0,
        [&](int r, int c) -> float {
            const EpisodeRow w = episode_row(row0 + r, T);
            if (c < P.od) return episode_state_column(P, w.e * (T + 1) + w.t, nullptr, c);
            if (c < P.od + gd) return L.xin[r * S8_LDX + c];      // kept: this thread is about to store the word it reads
            return episode_action_column(P, A.act, w.m, A.act_off, c);   // k_episode_q's
        },
        [&](int r, float q) { A.q[row0 + r] = q; });
}

// everything behind the entry's own checks (null arguments, contexts, the block's range): the remaining refusals in
// hp_episode_policy's order -- the goal mode and the reward kind behind the row count -- then the one launch
static int episode_bellman_launch(const char *entry, hp_agent *a, hp_norm *on, hp_norm *gn, int32_t goal_mode, const EpisodeRows &R,
                                  double thr, int32_t reward_type, double clip_obs, float *q, float *q_next, float *r, float *y) {
    EpisodeBellmanArgs A = {};
    HP_TRY(episode_net_args(entry, a, on, gn, "network", slab_net(a, true), R, (int32_t)gn->size, clip_obs, A));
    HP_REQUIRE(goal_mode == HP_GOAL_DESIRED || goal_mode == HP_GOAL_FINAL, HP_ERR_INVALID,
               "%s: goal_mode %d is neither 0 (the desired goal) nor 1 (the episode's final achieved goal)", entry, (int)goal_mode);
    HP_REQUIRE(reward_type == 0 || reward_type == 1, HP_ERR_INVALID, "%s: reward_type %d is neither 0 (sparse) nor 1 (dense)", entry,
               (int)reward_type);
    A.online = slab_net(a, false);
    A.ag = R.ag; A.act = R.act;
    A.q = q; A.q_next = q_next; A.r = r; A.y = y;
    A.goal_mode = goal_mode;
    A.sq_threshold = reward_type == 0 ? squared_bound(thr, true) : -1.0;
    A.gamma = (float)a->cfg.gamma;                                   // agent_engines.hip, agent_layers.hip: the update kernels' two
    A.clip_ret = (float)(1.0 / (1.0 - a->cfg.gamma));
    return episode_net_launch(k_episode_bellman, a, A);
}

// ---- the columns (HP_BELLMAN_STATS) -------------------------------------------------------------------------------------------------
struct BellmanStatsArgs {
    const float *q, *q_next, *r, *y;   // [n][T] each
    double *stats;                     // [n][HP_BELLMAN_STATS]
    float gamma;
    int T;
};

// k_episode_bellman_stats: episode_column_walk (episode_audit.h) over five sums and one count.  Per step
// d = (double)y - (double)q; a step counts as clipped when r + gamma * q_next, the float32 expression of the target, is not y.
__global__ __launch_bounds__(64) void k_episode_bellman_stats(const BellmanStatsArgs A) {
    const int T = A.T;
    const long long e = blockIdx.x;
    const float *q = A.q + e * (long long)T, *q_next = A.q_next + e * (long long)T, *r = A.r + e * (long long)T, *y = A.y + e * (long long)T;
    double sum[5];                 // d, |d|, d^2, y, r
    long long count[1];            // clipped
    episode_column_walk(T, sum, count, [&](int t, double (&s)[5], int (&c)[1]) {
        const float yv = y[t], rv = r[t];
        const double d = __dsub_rn((double)yv, (double)q[t]);
        s[0] = d;
        s[1] = fabs(d);
        s[2] = __dmul_rn(d, d);
        s[3] = (double)yv;
        s[4] = (double)rv;
        const float raw = rv + A.gamma * q_next[t];
        c[0] = raw != yv ? 1 : 0;
    });
    if (threadIdx.x == 0) {
        double *out = A.stats + e * HP_BELLMAN_STATS;
        const double dT = (double)T;
        out[0] = __ddiv_rn(sum[0], dT);
        out[1] = __ddiv_rn(sum[1], dT);
        out[2] = __ddiv_rn(sum[2], dT);
        out[3] = __ddiv_rn(sum[3], dT);
        out[4] = __ddiv_rn((double)count[0], dT);
        out[5] = __ddiv_rn(sum[4], dT);
    }
}

extern "C" {

int hp_episode_bellman(hp_agent *a, hp_norm *on, hp_norm *gn, int32_t goal_mode, const double *obs_dev, const double *ag_dev,
                       const double *g_dev, const double *actions_dev, int64_t n_episodes, int32_t T, double distance_threshold,
                       int32_t reward_type, double clip_obs, float *q_dev, float *q_next_dev, float *r_dev, float *y_dev) {
    HP_REQUIRE(a && on && gn && obs_dev && ag_dev && g_dev && actions_dev && q_dev && q_next_dev && r_dev && y_dev, HP_ERR_INVALID,
               "hp_episode_bellman: null argument");
    HP_SERIALISE(a);
    HP_TRY(episode_one_context("hp_episode_bellman", a, on, gn));
    return episode_bellman_launch("hp_episode_bellman", a, on, gn, goal_mode,
                                  EpisodeRows{obs_dev, ag_dev, g_dev, actions_dev, -1, -1, -1, n_episodes, T}, distance_threshold, reward_type,
                                  clip_obs, q_dev, q_next_dev, r_dev, y_dev);
}

int hp_episode_bellman_block(hp_rollout *ro, hp_agent *a, hp_norm *on, hp_norm *gn, int32_t goal_mode, int64_t first_episode,
                             int64_t n_episodes, double distance_threshold, int32_t reward_type, double clip_obs, float *q_dev,
                             float *q_next_dev, float *r_dev, float *y_dev) {
    HP_REQUIRE(ro && a && on && gn && q_dev && q_next_dev && r_dev && y_dev, HP_ERR_INVALID, "hp_episode_bellman_block: null argument");
    HP_SERIALISE(ro);
    EpisodeRows rows;
    HP_TRY(episode_block_rows("hp_episode_bellman_block", ro, a, on, gn, first_episode, n_episodes, rows));
    return episode_bellman_launch("hp_episode_bellman_block", a, on, gn, goal_mode, rows, distance_threshold, reward_type, clip_obs, q_dev,
                                  q_next_dev, r_dev, y_dev);
}

int hp_episode_bellman_stats(hp_ctx *ctx, const float *q_dev, const float *q_next_dev, const float *r_dev, const float *y_dev,
                             int64_t n_episodes, int32_t T, double gamma, double *stats_dev) {
    HP_REQUIRE(ctx && q_dev && q_next_dev && r_dev && y_dev && stats_dev, HP_ERR_INVALID, "hp_episode_bellman_stats: null argument");
    CtxGuard guard(ctx);
    HP_TRY(episode_check_shape("hp_episode_bellman_stats", n_episodes, T));
    HP_REQUIRE(gamma >= 0.0 && gamma <= 1.0, HP_ERR_INVALID, "hp_episode_bellman_stats: gamma %g outside [0, 1]", gamma);
    BellmanStatsArgs A;
    A.q = q_dev; A.q_next = q_next_dev; A.r = r_dev; A.y = y_dev; A.stats = stats_dev;
    A.gamma = (float)gamma;        // the agent's own: float32, narrowed as the update launches narrow it
    A.T = T;
    hipLaunchKernelGGL(k_episode_bellman_stats, dim3((unsigned)n_episodes), dim3(64), 0, ctx->stream, A);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

}  // extern "C"
