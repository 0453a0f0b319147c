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
#include <cmath>

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wundefined-inline"   // agent_device.h declares the 32-row engine's fragment map, which no code here calls
#include "agent_device.h"
#pragma clang diagnostic pop

// the 4-row slab's device functions (no kernel of slab8.h is compiled here)
#define S8_DEVICE_ONLY
#define S8_NRG 1
#define S8_NS s8eb
#include "slab8.h"
#undef S8_NRG
#undef S8_NS
#undef S8_DEVICE_ONLY

#include "episode_audit.h"
#include "policy_call.h"

struct EpisodeBellmanArgs {
    PolicyArgs P;                  // the target actor: obs / g at the first episode (indexed here, not by s8_policy_slab), rows = n T
    SlabNetPtrs online;            // the online parameter set (P.net: the target one)
    const double *ag, *act;        // [n][T + 1][gd], [n][T][ad], already offset to the first episode
    float *q, *q_next, *r, *y;     // [n][T] each
    NetLayout lc;
    double sq_threshold;           // sparse: squared_bound(thr, true); dense: < 0 (hp_reward's rule)
    float gamma, clip_ret;         // what the agent hands its update kernels
    int T, act_off, ca, goal_mode; // the critic's segment starts at ca = la.total
};

__global__ __launch_bounds__(S8_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_episode_bellman(const EpisodeBellmanArgs A) {
    __shared__ s8eb::PolicyLds L;
    const long long row0 = (long long)blockIdx.x * 4;
    const PolicyArgs &P = A.P;
    const int T = A.T, gd = P.gd;
    // the goal of row m = e T + t: the block's own at t, or the episode's last achieved one
    auto goal_of = [&](long long m, long long e) -> const double * {
        return A.goal_mode == HP_GOAL_FINAL ? A.ag + (e * (T + 1) + T) * gd : P.g + m * gd;
    };
    s8eb::s8_policy_slab(P, L, (size_t)row0,
        [&](int r, int c) -> float {
            const long long m = row0 + r, e = m / T;
            const int t = (int)(m - e * T);
            if (c < P.od) return tr_net_input(P.obs[(e * (T + 1) + t + 1) * P.od + c], P.clip_obs, P.onz->mean[c], P.onz->std[c], P.clip_o);
            const int j = c - P.od;
            return tr_net_input(goal_of(m, e)[j], P.clip_obs, P.gnz->mean[j], P.gnz->std[j], P.clip_g);
        },
        [&](int r, int j, float a) { L.xin[r * S8_LDX + A.act_off + j] = a / P.max_action; });   // a = max_action * th: the actor-side chain's u
    s8eb::s8_sync();
    s8eb::s8_critic_slab(P.net, A.lc, A.ca, P.H, (long long)P.rows, L, (size_t)row0,
        [&](int r, int c) -> float { return L.xin[r * S8_LDX + c]; },
        [&](int r, float qn) {
            const long long m = row0 + r, e = m / T;
            const int t = (int)(m - e * T);
            const float rw = hp_reward(tr_sq_distance(A.ag + (e * (T + 1) + t + 1) * gd, goal_of(m, e), gd), A.sq_threshold);
            float y = rw + A.gamma * qn;
            y = fminf(fmaxf(y, -A.clip_ret), 0.f);
            A.q_next[m] = qn; A.r[m] = rw; A.y[m] = y;
        });
    s8eb::s8_sync();
    s8eb::s8_critic_slab(A.online, A.lc, A.ca, P.H, (long long)P.rows, L, (size_t)row0,
        [&](int r, int c) -> float {
            const long long m = row0 + r, e = m / T;
            const int t = (int)(m - e * T);
            if (c < P.od) return tr_net_input(P.obs[(e * (T + 1) + t) * P.od + c], P.clip_obs, P.onz->mean[c], P.onz->std[c], P.clip_o);
            if (c < P.od + gd) return L.xin[r * S8_LDX + c];      // kept: this thread is about to store the word it reads
            const int j = c - A.act_off;
            if (j >= 0 && j < P.act_dim) return (float)A.act[m * P.act_dim + j] / P.max_action;   // s8_gather, k_episode_q
            return 0.f;
        },
        [&](int r, float q) { A.q[row0 + r] = q; });
}

// everything behind the entry's own checks (null arguments, contexts, the block's range): the remaining refusals in
// hp_episode_policy's order -- the goal mode and the reward kind behind the row count -- then the one launch
static int episode_bellman_launch(const char *entry, hp_agent *a, hp_norm *on, hp_norm *gn, int32_t goal_mode, const double *obs,
                                  const double *ag, const double *g, const double *act, int block_od, int block_gd, int block_ad,
                                  int64_t n, int32_t T, double thr, int32_t reward_type, double clip_obs, float *q, float *q_next,
                                  float *r, float *y) {
    HP_TRY(require_slab_shaped(entry, a, HP_ERR_STATE));
    HP_REQUIRE(on->size + gn->size == a->xdim, HP_ERR_INVALID, "%s: normalizer sizes %d+%d do not match the network input %d", entry,
               (int)on->size, (int)gn->size, a->xdim);
    HP_REQUIRE(block_od < 0 || (block_od == on->size && block_gd == gn->size && block_ad == a->cfg.act_dim), HP_ERR_INVALID,
               "%s: the block has dimensions %d / %d / %d, normalizers and agent have %d / %d / %d", entry, block_od, block_gd, block_ad,
               (int)on->size, (int)gn->size, a->cfg.act_dim);
    HP_TRY(episode_check_shape(entry, n, T, (int32_t)gn->size));
    const long long rows = (long long)n * T;
    HP_REQUIRE(rows < (1LL << 31), HP_ERR_INVALID, "%s: %lld steps are more than one launch holds (2^31)", entry, rows);
    HP_REQUIRE(goal_mode == HP_GOAL_DESIRED || goal_mode == HP_GOAL_FINAL, HP_ERR_INVALID,
               "%s: goal_mode %d is neither 0 (the desired goal) nor 1 (the episode's final achieved goal)", entry, (int)goal_mode);
    HP_REQUIRE(reward_type == 0 || reward_type == 1, HP_ERR_INVALID, "%s: reward_type %d is neither 0 (sparse) nor 1 (dense)", entry,
               (int)reward_type);
    static_assert(sizeof(s8eb::PolicyLds) <= 160 * 1024, "the policy slab's LDS fits a CU");
    EpisodeBellmanArgs A;
    memset(&A, 0, sizeof(A));
    A.P = policy_args(a, slab_net(a, true), norm_view(on), norm_view(gn), clip_or_inf(clip_obs), rows);
    A.P.obs = obs; A.P.g = g;
    A.online = slab_net(a, false);
    A.ag = ag; A.act = act;
    A.q = q; A.q_next = q_next; A.r = r; A.y = y;
    A.lc = a->lc; A.T = T; A.act_off = a->act_off; A.ca = a->la.total; A.goal_mode = goal_mode;
    A.sq_threshold = reward_type == 0 ? squared_bound(thr, true) : -1.0;
    A.gamma = (float)a->cfg.gamma;                                   // agent_engines.hip, agent_layers.hip: the update kernels' two
    A.clip_ret = (float)(1.0 / (1.0 - a->cfg.gamma));
    hipLaunchKernelGGL(k_episode_bellman, dim3((unsigned)((rows + 3) / 4)), dim3(S8_THREADS), 0, a->ctx->stream, A);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

// ---- the columns (HP_BELLMAN_STATS) -------------------------------------------------------------------------------------------------
struct BellmanStatsArgs {
    const float *q, *q_next, *r, *y;   // [n][T] each
    double *stats;                     // [n][HP_BELLMAN_STATS]
    float gamma;
    int T;
};

// k_episode_bellman_stats.  One wave per episode, T walked in chunks of 64 steps from the first chunk up, as k_episode_policy_stats
// walks it: the lanes form their steps' terms side by side, then the sums over t run wave-uniformly in ascending t, step base + i
// taking its terms out of lane i (v_readlane).  The twin (synthetic.episode_bellman_stats) is the same loop.  Per step
// d = (double)y - (double)q; a step counts as clipped when r + gamma * q_next, the float32 expression of the target, is not y.
__global__ __launch_bounds__(64) void k_episode_bellman_stats(const BellmanStatsArgs A) {
    const int lane = threadIdx.x, T = A.T;
    const long long e = blockIdx.x;
    const float *q = A.q + e * (long long)T, *q_next = A.q_next + e * (long long)T, *r = A.r + e * (long long)T, *y = A.y + e * (long long)T;
    double sum_d = 0.0, sum_abs = 0.0, sum_sq = 0.0, sum_y = 0.0, sum_r = 0.0;
    long long clipped = 0;
    for (int base = 0; base < T; base += 64) {
        const int cnt = T - base < 64 ? T - base : 64;
        const int t = base + lane;
        double d = 0.0, ab = 0.0, sq = 0.0, yd = 0.0, rd = 0.0;
        int clip = 0;
        if (lane < cnt) {
            const float yv = y[t], rv = r[t];
            yd = (double)yv;
            rd = (double)rv;
            d = __dsub_rn(yd, (double)q[t]);
            ab = fabs(d);
            sq = __dmul_rn(d, d);
            const float raw = rv + A.gamma * q_next[t];
            clip = raw != yv ? 1 : 0;
        }
        for (int i = 0; i < cnt; ++i) {
            sum_d = __dadd_rn(sum_d, lane_read_d(d, i));
            sum_abs = __dadd_rn(sum_abs, lane_read_d(ab, i));
            sum_sq = __dadd_rn(sum_sq, lane_read_d(sq, i));
            sum_y = __dadd_rn(sum_y, lane_read_d(yd, i));
            sum_r = __dadd_rn(sum_r, lane_read_d(rd, i));
            clipped += __builtin_amdgcn_readlane(clip, i);
        }
    }
    if (lane == 0) {
        double *out = A.stats + e * HP_BELLMAN_STATS;
        const double dT = (double)T;
        out[0] = __ddiv_rn(sum_d, dT);
        out[1] = __ddiv_rn(sum_abs, dT);
        out[2] = __ddiv_rn(sum_sq, dT);
        out[3] = __ddiv_rn(sum_y, dT);
        out[4] = __ddiv_rn((double)clipped, dT);
        out[5] = __ddiv_rn(sum_r, dT);
    }
}

extern "C" {

int hp_episode_bellman(hp_agent *a, hp_norm *on, hp_norm *gn, int32_t goal_mode, const double *obs_dev, const double *ag_dev,
                       const double *g_dev, const double *actions_dev, int64_t n_episodes, int32_t T, double distance_threshold,
                       int32_t reward_type, double clip_obs, float *q_dev, float *q_next_dev, float *r_dev, float *y_dev) {
    HP_REQUIRE(a && on && gn && obs_dev && ag_dev && g_dev && actions_dev && q_dev && q_next_dev && r_dev && y_dev, HP_ERR_INVALID,
               "hp_episode_bellman: null argument");
    HP_SERIALISE(a);
    HP_REQUIRE(on->ctx == a->ctx && gn->ctx == a->ctx, HP_ERR_INVALID, "hp_episode_bellman: handles belong to different contexts");
    return episode_bellman_launch("hp_episode_bellman", a, on, gn, goal_mode, obs_dev, ag_dev, g_dev, actions_dev, -1, -1, -1, n_episodes, T,
                                  distance_threshold, reward_type, clip_obs, q_dev, q_next_dev, r_dev, y_dev);
}

int hp_episode_bellman_block(hp_rollout *ro, hp_agent *a, hp_norm *on, hp_norm *gn, int32_t goal_mode, int64_t first_episode,
                             int64_t n_episodes, double distance_threshold, int32_t reward_type, double clip_obs, float *q_dev,
                             float *q_next_dev, float *r_dev, float *y_dev) {
    HP_REQUIRE(ro && a && on && gn && q_dev && q_next_dev && r_dev && y_dev, HP_ERR_INVALID, "hp_episode_bellman_block: null argument");
    HP_SERIALISE(ro);
    HP_REQUIRE(a->ctx == ro->ctx && on->ctx == ro->ctx && gn->ctx == ro->ctx, HP_ERR_INVALID,
               "hp_episode_bellman_block: handles belong to different contexts");
    RolloutArrays at;
    HP_TRY(episode_block_range("hp_episode_bellman_block", ro, first_episode, n_episodes, at));
    return episode_bellman_launch("hp_episode_bellman_block", a, on, gn, goal_mode, at.b_obs, at.b_ag, at.b_g, at.b_act, ro->od, ro->gd,
                                  ro->ad, n_episodes, ro->T, distance_threshold, reward_type, clip_obs, q_dev, q_next_dev, r_dev, y_dev);
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
