// episode_policy.hip -- what the actor's objective sees of an episode block, computed where the block lies (hp_episode_policy,
// hp_episode_policy_block): pi(s_t) and Q(s_t, pi(s_t)) for t = 0 .. T-1 of every episode in ONE launch, and the columns that set
// them beside the recorded actions and hp_episode_q's Q(s_t, a_t) (hp_episode_policy_stats, hp_episode_policy_stats_block; their
// means, hp_episode_policy_summary, are episode_returns.hip's k_episode_column_means): whether the critic ranks a
// demonstration's action above the policy's (the Q-filter), how far the
// recorded actions lie from the policy (what exploration or a script adds), and whether the actor saturates its tanh -- the two terms
// of the actor loss, -Q(s, pi(s)) and (pi / max_action)^2 (ddpg_agent.py:265-267), on real episodes.
//
// k_episode_policy is the forward half of the actor-side chain of an update (slab8_actor_side.inc) inside the frame of k_episode_q
// (episode_q.hip): flat row m = e T + t, workgroup b owns rows 4b .. 4b+3, obs has T + 1 rows per episode and g T, one PolicyLds.
// s8_policy_slab runs on the slab with the inputs of s8_gather (tr_net_input: clip, subtract, divide, clip in float64, one rounding
// each); its emit writes pi[m][j] and puts u_j = (max_action * th_j) / max_action, float32, at act_off of the row's input in the
// LDS -- the expression and the place of the actor-side chain.  One barrier, which is the entry condition of s8_critic_slab (the
// actor's trunk has drained its weight ring, nothing reads the LDS any more), and s8_critic_slab runs on the same four rows.
//
// The normalised obs | g columns are KEPT, not recomputed: the actor's trunk reads the input rows and leaves them alone, the
// critic's input has the same columns at the same places (its own begin at act_off >= od + gd, and s8_policy_slab zeroed what lies
// between), so the critic's input function hands every thread back the word it is about to store.  The float64 divisions of
// tr_net_input -- what a gather is bound by -- are done once per row, as in an update.
//
// Which weights: the four buffers episode_q.hip's header names (a->fragF / a->params, a->fragFT / a->targets), the actor's segment at
// 0 and the critic's at la.total, on the context's stream behind whatever wrote them.  target: both target networks together.
#include "episode_nets.h"

struct EpisodePolicyArgs : EpisodeNetArgs {   // P.net: the actor's and the critic's parameter set
    using Lds = s8en::PolicyLds;
    float *pi, *q_pi;              // [n][T][ad], [n][T]
};

__global__ __launch_bounds__(S8_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_episode_policy(const EpisodePolicyArgs A) {
    __shared__ EpisodePolicyArgs::Lds L;
    const long long row0 = (long long)blockIdx.x * 4;
    const PolicyArgs &P = A.P;
    s8en::s8_policy_slab(P, L, (size_t)row0,
        [&](int r, int c) -> float {
            const EpisodeRow w = episode_row(row0 + r, A.T);
            return episode_state_column(P, w.e * (A.T + 1) + w.t, P.g + w.m * P.gd, c);
        },
        [&](int r, int j, float a) {
            A.pi[(row0 + r) * P.act_dim + j] = a;
            L.xin[r * S8_LDX + A.act_off + j] = a / P.max_action;   // a = max_action * th: the actor-side chain's u
        });
    s8en::s8_sync();
    s8en::s8_critic_slab(P.net, A.lc, A.ca, P.H, (long long)P.rows, L, (size_t)row0,
        [&](int r, int c) -> float { return L.xin[r * S8_LDX + c]; },
        [&](int r, float q) { A.q_pi[row0 + r] = q; });
}

// everything behind the entry's own checks (null arguments, contexts, the block's range): the remaining refusals in hp_episode_q's
// order, then the one launch
static int episode_policy_launch(const char *entry, hp_agent *a, hp_norm *on, hp_norm *gn, int32_t target, const EpisodeRows &R,
                                 double clip_obs, float *pi, float *q_pi) {
    HP_REQUIRE(target == 0 || target == 1, HP_ERR_INVALID, "%s: target %d is neither 0 (online) nor 1 (target networks)", entry, (int)target);
    EpisodePolicyArgs A = {};
    HP_TRY(episode_net_args(entry, a, on, gn, "network", slab_net(a, target != 0), R, 1, clip_obs, A));
    A.pi = pi; A.q_pi = q_pi;
    return episode_net_launch(k_episode_policy, a, A);
}

// ---- the columns (HP_POLICY_STATS) --------------------------------------------------------------------------------------------------
struct PolicyStatsArgs {
    const float *pi, *q_pi, *q;    // [n][T][ad], [n][T], [n][T] or nullptr
    const double *act;             // [n][T][ad], already offset to the first episode
    double *stats;                 // [n][HP_POLICY_STATS]
    double max_action, sat_bound;  // (double)(float)max_action; sat * max_action
    int T, ad;
};

// k_episode_policy_stats: episode_column_walk (episode_audit.h) over four sums and two counts; a step's inner sums over j ascending
__global__ __launch_bounds__(64) void k_episode_policy_stats(const PolicyStatsArgs A) {
    const int T = A.T, ad = A.ad;
    const long long e = blockIdx.x;
    const float *pi = A.pi + e * (long long)T * ad, *q_pi = A.q_pi + e * (long long)T;
    const float *q = A.q ? A.q + e * (long long)T : nullptr;
    const double *act = A.act + e * (long long)T * ad;
    double sum[4];                 // q_pi, q - q_pi, the action gap, the regulariser
    long long count[2];            // filtered, saturated
    episode_column_walk(T, sum, count, [&](int t, double (&s)[4], int (&c)[2]) {
        const float qp = q_pi[t];
        s[0] = (double)qp;
        if (q) {
            const float qv = q[t];
            s[1] = __dsub_rn(s[0], (double)qv);
            c[0] = qv > qp ? 1 : 0;
        }
        double dd = 0.0, vv = 0.0;
        for (int j = 0; j < ad; ++j) {
            const double p = (double)pi[(long long)t * ad + j];
            const double d = __dsub_rn(act[(long long)t * ad + j], p);
            const double v = __ddiv_rn(p, A.max_action);
            dd = __dadd_rn(dd, __dmul_rn(d, d));
            vv = __dadd_rn(vv, __dmul_rn(v, v));
            c[1] += fabs(p) >= A.sat_bound ? 1 : 0;
        }
        s[2] = __dsqrt_rn(dd);
        s[3] = __ddiv_rn(vv, (double)ad);
    });
    if (threadIdx.x == 0) {
        double *out = A.stats + e * HP_POLICY_STATS;
        const double dT = (double)T, none = __longlong_as_double(0x7ff8000000000000LL);
        out[0] = __ddiv_rn(sum[0], dT);
        out[1] = q ? __ddiv_rn(sum[1], dT) : none;
        out[2] = q ? __ddiv_rn((double)count[0], dT) : none;
        out[3] = __ddiv_rn(__ddiv_rn(sum[2], A.max_action), dT);
        out[4] = __ddiv_rn((double)count[1], (double)((long long)T * ad));
        out[5] = __ddiv_rn(sum[3], dT);
    }
}

static int policy_stats_launch(const char *entry, hipStream_t stream, const float *pi, const float *q_pi, const double *act,
                               const float *q, int64_t n, int32_t T, int32_t ad, double max_action, double sat, double *stats) {
    HP_TRY(episode_check_shape(entry, n, T));
    HP_REQUIRE(ad >= 1 && ad <= HP_POLICY_MAX_ACT_DIM, HP_ERR_INVALID, "%s: act_dim %d outside [1, %d]", entry, (int)ad,
               HP_POLICY_MAX_ACT_DIM);
    HP_REQUIRE(max_action > 0.0 && std::isfinite(max_action), HP_ERR_INVALID, "%s: max_action %g is not a positive number", entry, max_action);
    HP_REQUIRE(sat >= 0.0 && sat <= 1.0, HP_ERR_INVALID, "%s: sat %g outside [0, 1]", entry, sat);
    PolicyStatsArgs A;
    A.pi = pi; A.q_pi = q_pi; A.q = q; A.act = act; A.stats = stats;
    A.max_action = (double)(float)max_action;       // the networks' own: float32
    A.sat_bound = sat * A.max_action;
    A.T = T; A.ad = ad;
    hipLaunchKernelGGL(k_episode_policy_stats, dim3((unsigned)n), dim3(64), 0, stream, A);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

extern "C" {

int hp_episode_policy(hp_agent *a, hp_norm *on, hp_norm *gn, int32_t target, const double *obs_dev, const double *g_dev,
                      int64_t n_episodes, int32_t T, double clip_obs, float *pi_dev, float *q_pi_dev) {
    HP_REQUIRE(a && on && gn && obs_dev && g_dev && pi_dev && q_pi_dev, HP_ERR_INVALID, "hp_episode_policy: null argument");
    HP_SERIALISE(a);
    HP_TRY(episode_one_context("hp_episode_policy", a, on, gn));
    return episode_policy_launch("hp_episode_policy", a, on, gn, target, EpisodeRows{obs_dev, nullptr, g_dev, nullptr, -1, -1, -1, n_episodes, T},
                                 clip_obs, pi_dev, q_pi_dev);
}

int hp_episode_policy_block(hp_rollout *ro, hp_agent *a, hp_norm *on, hp_norm *gn, int32_t target, int64_t first_episode,
                            int64_t n_episodes, double clip_obs, float *pi_dev, float *q_pi_dev) {
    HP_REQUIRE(ro && a && on && gn && pi_dev && q_pi_dev, HP_ERR_INVALID, "hp_episode_policy_block: null argument");
    HP_SERIALISE(ro);
    EpisodeRows rows;
    HP_TRY(episode_block_rows("hp_episode_policy_block", ro, a, on, gn, first_episode, n_episodes, rows));
    return episode_policy_launch("hp_episode_policy_block", a, on, gn, target, rows, clip_obs, pi_dev, q_pi_dev);
}

int hp_episode_policy_stats(hp_ctx *ctx, const float *pi_dev, const float *q_pi_dev, const double *actions_dev, const float *q_dev,
                            int64_t n_episodes, int32_t T, int32_t act_dim, double max_action, double sat, double *stats_dev) {
    HP_REQUIRE(ctx && pi_dev && q_pi_dev && actions_dev && stats_dev, HP_ERR_INVALID, "hp_episode_policy_stats: null argument");
    CtxGuard guard(ctx);
    return policy_stats_launch("hp_episode_policy_stats", ctx->stream, pi_dev, q_pi_dev, actions_dev, q_dev, n_episodes, T, act_dim,
                               max_action, sat, stats_dev);
}

int hp_episode_policy_stats_block(hp_rollout *ro, const float *pi_dev, const float *q_pi_dev, const float *q_dev, int64_t first_episode,
                                  int64_t n_episodes, double max_action, double sat, double *stats_dev) {
    HP_REQUIRE(ro && pi_dev && q_pi_dev && stats_dev, HP_ERR_INVALID, "hp_episode_policy_stats_block: null argument");
    HP_SERIALISE(ro);
    RolloutArrays at;
    HP_TRY(episode_block_range("hp_episode_policy_stats_block", ro, first_episode, n_episodes, at));
    return policy_stats_launch("hp_episode_policy_stats_block", ro->ctx->stream, pi_dev, q_pi_dev, at.b_act, q_dev, n_episodes, ro->T,
                               ro->ad, max_action, sat, stats_dev);
}

}  // extern "C"
