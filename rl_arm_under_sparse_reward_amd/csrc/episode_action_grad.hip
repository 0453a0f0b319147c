// episode_action_grad.hip -- the quantity that moves the actor, for every step of an episode block, computed where the block lies
// (hp_episode_action_grad, hp_episode_action_grad_block): dQ/du at u = pi(s_t) / max_action (at = 0) or at the recorded
// u = a_t / max_action (at = 1) for t = 0 .. T-1 of every episode in ONE launch, and the columns that set it beside the regulariser
// and the recorded actions (hp_episode_signal_stats, hp_episode_signal_stats_block; their means, hp_episode_signal_summary, are
// episode_returns.hip's k_episode_column_means).  A sample's actor update is dQ/da at a = pi(s), minus the action_l2 pull, through
// tanh' (ddpg_agent.py:265-267 through models.py:28-44): where the critic is flat in the action the actor learns nothing, or only
// shrinks towards zero, and a demonstration helps only where the gradient at pi(s) points towards the demonstrated action.
//
// k_episode_action_grad is the actor-side chain of an update (slab8_actor_side.inc) up to the action columns of the critic's input
// gradient, inside the frame of k_episode_policy (episode_policy.hip): flat row m = e T + t, workgroup b owns rows 4b .. 4b+3.
//   at = 0: s8_policy_slab exactly as k_episode_policy runs it (pi emitted, u = (max_action th) / max_action at act_off), one barrier;
//   at = 1: the rows of k_episode_q (episode_q.hip), the action columns the recorded act / max_action in float32; no actor.
// Then the critic's forward WITH the ReLU masks of h1 and h2 (s8_trunk writes them behind the same arithmetic: the forward values
// are bit for bit hp_episode_policy's / hp_episode_q's), Q emitted; s8_head_bwd_inplace_rows with the seed dQ/dq = 1 for every
// live row (an update seeds -1 / B); the two masked wide dX layers over the critic's dX-order fragments, the weight ring running
// on from the forward fragments without draining; s8_rowdots against the action columns of the critic's first layer.  Lane j of a
// row's wave stores dq_du[m][j].  What is stored is the derivative with respect to the critic's action INPUT u = a / max_action;
// dQ/da = dq_du / max_action and is not stored.
//
// Which weights: the online set's three buffers (a->fragF, a->fragD, a->params; episode_q.hip's header), the critic's segment at
// la.total.  The target networks keep no dX-order fragments (slab_net, policy_call.h: fragFT and targets alone -- no update ever
// differentiates through them), and this audit builds no second set: target = 1 is refused with HP_ERR_STATE.
#include "episode_nets.h"   // S8_NRG stays defined behind it: critic_action_grad_slab below is written in the slab height's macros

static_assert(HP_SIGNAL_STATS == EPISODE_COLS, "one summary loop");

struct ActionGradLds {
    s8en::PolicyLds P;
    s8en::s8_mask_t msk[2][256];                       // ReLU masks of the critic's h1, h2
    float w1t[4 * 256] __attribute__((aligned(16)));   // the action columns of the critic's first layer, [column][unit]
};

struct ActionGradArgs : EpisodeNetArgs {   // P.net: the online parameter set
    using Lds = ActionGradLds;
    const double *act;             // [n][T][ad] (at = 1)
    float *pi, *q, *dq_du;         // [n][T][ad] (at = 0), [n][T], [n][T][ad]
    int at;
};

// s8_critic_slab (slab8.h) with the masks kept and the chain's backward steps behind it.  net.wd must exist.  input / emit_q as
// there; emit_g(r, j, v) is called by lane j < ad of wave r with d Q / d u_j of row r.
template <class Input, class EmitQ, class EmitG>
__device__ __forceinline__ void critic_action_grad_slab(const SlabNetPtrs &net, const NetLayout &lc, int ca, int H, int act_off, int ad,
                                                        long long rows, ActionGradLds &L, size_t row0, Input input, EmitQ emit_q,
                                                        EmitG emit_g) {
    using namespace s8en;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float *wf = net.wf + ca, *wd = net.wd + ca, *canon = net.canon + ca;
    float *xin = L.P.xin, *bufA = L.P.bufA, *bufB = L.P.bufB, *pbuf = L.P.pbuf;
    RingSlot *ring = L.P.wring[wave];
    int rbase = 0;
    float4 wbc[6], wq[4];
    float w1n[4];
    s8_small_prefetch(wf + lc.w1, lc.K1, wbc);
    wq[0] = *reinterpret_cast<const float4 *>(canon + lc.w4 + 4 * lane);
    const float bq = canon[lc.b4];
    const float w4c = canon[lc.w4 + (tid & 255)];
    {
        const float *w1 = canon + lc.w1 + (size_t)(tid & 255) * lc.K1 + act_off;
#pragma unroll
        for (int j = 0; j < 4; ++j) w1n[j] = w1[j < ad ? j : ad - 1];
    }
    for (int idx = tid; idx < S8_ROWS * S8_LDX; idx += S8_THREADS) {
        const int r = idx / S8_LDX, c = idx - r * S8_LDX;
        const size_t m = row0 + r;
        float v = 0.f;
        if ((long long)m < rows) v = input(r, c);
        xin[idx] = v;
    }
    s8_ring_prologue(ring, rbase, wf + lc.w2);
    s8_sync();
    s8_trunk(xin, lc, wbc, wf, canon, H, bufA, bufB, pbuf, nullptr, nullptr, nullptr, row0, ring, rbase, wd + lc.w3, nullptr, 0,
             L.msk[0], L.msk[1]);
#pragma unroll
    for (int i = 0; i < S8_RPW; ++i) {
        const int rr = wave + S8_WAVES * i;
        const float q = s8_rowdots(bufA, S8_LD, rr < S8_ROWS ? rr : 0, 1, wq);
        if (lane == 0 && rr < S8_ROWS && (long long)(row0 + rr) < rows) emit_q(rr, q + bq);
    }
    if (tid < 256) {
#pragma unroll
        for (int j = 0; j < 4; ++j) L.w1t[j * 256 + tid] = w1n[j];
    }
    s8_sync();
    s8_head_bwd_inplace_rows(1.0f, (int)row0, (int)rows, w4c, bufA);   // bufA holds h3; dQ / dq = 1 for a live row
    s8_sync();
    s8_big_layer(bufA, S8_LD, ring, rbase, wd + lc.w3, wd + lc.w2, SE_MASK, nullptr, 0, pbuf, bufB, S8_LD, L.msk[1]);
    s8_sync();
    s8_big_layer(bufB, S8_LD, ring, rbase, wd + lc.w2, nullptr, SE_MASK, nullptr, 0, pbuf, bufA, S8_LD, L.msk[0]);
    s8_sync();
    float4 w1g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w1g[j] = *reinterpret_cast<const float4 *>(L.w1t + j * 256 + 4 * lane);
#pragma unroll
    for (int i = 0; i < S8_RPW; ++i) {
        const int rr = wave + S8_WAVES * i;
        const float sj = s8_rowdots(bufA, S8_LD, rr < S8_ROWS ? rr : 0, ad, w1g);
        if (lane < ad && rr < S8_ROWS && (long long)(row0 + rr) < rows) emit_g(rr, lane, sj);
    }
}

__global__ __launch_bounds__(S8_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_episode_action_grad(const ActionGradArgs A) {
    __shared__ ActionGradArgs::Lds L;
    const long long row0 = (long long)blockIdx.x * 4;
    const PolicyArgs &P = A.P;
    auto net_input = [&](int r, int c) -> float {
        const EpisodeRow w = episode_row(row0 + r, A.T);
        return episode_state_column(P, w.e * (A.T + 1) + w.t, P.g + w.m * P.gd, c);
    };
    if (A.at == 0) {
        s8en::s8_policy_slab(P, L.P, (size_t)row0, net_input,
            [&](int r, int j, float a) {
                A.pi[(row0 + r) * P.act_dim + j] = a;
                L.P.xin[r * S8_LDX + A.act_off + j] = a / P.max_action;   // a = max_action * th: the actor-side chain's u
            });
        s8en::s8_sync();
    }
    critic_action_grad_slab(P.net, A.lc, A.ca, P.H, A.act_off, P.act_dim, (long long)P.rows, L, (size_t)row0,
        [&](int r, int c) -> float {
            if (A.at == 0) return L.P.xin[r * S8_LDX + c];               // kept, as in k_episode_policy
            if (c < P.od + P.gd) return net_input(r, c);
            return episode_action_column(P, A.act, row0 + r, A.act_off, c);   // k_episode_q's
        },
        [&](int r, float q) { A.q[row0 + r] = q; },
        [&](int r, int j, float v) { A.dq_du[(row0 + r) * P.act_dim + j] = v; });
}

// everything behind the entry's own checks (null arguments, contexts, the block's range): the remaining refusals in
// hp_episode_policy's order -- `at` and what it needs behind `target`, the missing target fragments behind the agent's shape --
// then the one launch
static int action_grad_launch(const char *entry, hp_agent *a, hp_norm *on, hp_norm *gn, int32_t target, int32_t at, const EpisodeRows &R,
                              double clip_obs, float *pi, float *q, float *dq_du) {
    HP_REQUIRE(target == 0 || target == 1, HP_ERR_INVALID, "%s: target %d is neither 0 (online) nor 1 (target networks)", entry, (int)target);
    HP_REQUIRE(at == 0 || at == 1, HP_ERR_INVALID, "%s: at %d is neither 0 (the policy's action) nor 1 (the recorded action)", entry, (int)at);
    HP_REQUIRE(at == 0 || R.act, HP_ERR_INVALID, "%s: at 1 (the recorded action) needs actions_dev", entry);
    HP_REQUIRE(at == 1 || pi, HP_ERR_INVALID, "%s: at 0 (the policy's action) needs pi_dev", entry);
    HP_TRY(require_slab_shaped(entry, a, HP_ERR_STATE));
    const SlabNetPtrs net = slab_net(a, target != 0);
    HP_REQUIRE(net.wd, HP_ERR_STATE, "%s: the target networks keep no dX-order fragments (no update differentiates through them): target 1 is not available",
               entry);
    ActionGradArgs A = {};
    HP_TRY(episode_net_rows(entry, a, on, gn, "network", net, R, 1, clip_obs, A));
    A.act = R.act; A.pi = pi; A.q = q; A.dq_du = dq_du; A.at = at;
    return episode_net_launch(k_episode_action_grad, a, A);
}

// ---- the columns (HP_SIGNAL_STATS) --------------------------------------------------------------------------------------------------
struct SignalStatsArgs {
    const float *pi, *dq_du;       // [n][T][ad], [n][T][ad]
    const double *act;             // [n][T][ad], already offset to the first episode
    double *stats;                 // [n][HP_SIGNAL_STATS]
    double max_action, action_l2, flat;   // (double)(float)max_action
    int T, ad;
};

// k_episode_signal_stats: episode_column_walk (episode_audit.h) over four sums and two counts; a step's inner sums over j ascending.
// Per step, with M = max_action, lambda = action_l2: g_j = dq_du_j, v_j = pi_j / M, d_j = (act_j - pi_j) / M.
__global__ __launch_bounds__(64) void k_episode_signal_stats(const SignalStatsArgs A) {
    const int T = A.T, ad = A.ad;
    const long long e = blockIdx.x;
    const float *pi = A.pi + e * (long long)T * ad, *dq = A.dq_du + e * (long long)T * ad;
    const double *act = A.act + e * (long long)T * ad;
    const double dad = (double)ad, lam2 = __dmul_rn(A.action_l2, 2.0), reg_scale = __dmul_rn(A.action_l2, __ddiv_rn(2.0, dad));
    double sum[4];                 // |g|, the cosine, g . d, the trunk's signal
    long long count[2];            // flat, regulariser above the gradient
    episode_column_walk(T, sum, count, [&](int t, double (&s)[4], int (&c)[2]) {
        double gg = 0.0, vv = 0.0, dd = 0.0, ss = 0.0, dot = 0.0;
        for (int j = 0; j < ad; ++j) {
            const double p = (double)pi[(long long)t * ad + j];
            const double gj = (double)dq[(long long)t * ad + j];
            const double v = __ddiv_rn(p, A.max_action);
            const double d = __ddiv_rn(__dsub_rn(act[(long long)t * ad + j], p), A.max_action);
            gg = __dadd_rn(gg, __dmul_rn(gj, gj));
            vv = __dadd_rn(vv, __dmul_rn(v, v));
            dd = __dadd_rn(dd, __dmul_rn(d, d));
            dot = __dadd_rn(dot, __dmul_rn(gj, d));
            const double sj = __dmul_rn(__dsub_rn(gj, __ddiv_rn(__dmul_rn(lam2, v), dad)), __dsub_rn(1.0, __dmul_rn(v, v)));
            ss = __dadd_rn(ss, __dmul_rn(sj, sj));
        }
        const double gn = __dsqrt_rn(gg), vn = __dsqrt_rn(vv), den = __dmul_rn(gn, __dsqrt_rn(dd));
        c[0] = gn < A.flat ? 1 : 0;
        c[1] = __dmul_rn(reg_scale, vn) > gn ? 1 : 0;
        s[0] = gn;
        s[1] = den > 0.0 ? __ddiv_rn(dot, den) : 0.0;       // a step counts 0 when either norm is 0
        s[2] = dot;
        s[3] = __dsqrt_rn(ss);
    });
    if (threadIdx.x == 0) {
        double *out = A.stats + e * HP_SIGNAL_STATS;
        const double dT = (double)T;
        out[0] = __ddiv_rn(sum[0], dT);
        out[1] = __ddiv_rn((double)count[0], dT);
        out[2] = __ddiv_rn((double)count[1], dT);
        out[3] = __ddiv_rn(sum[1], dT);
        out[4] = __ddiv_rn(sum[2], dT);
        out[5] = __ddiv_rn(sum[3], dT);
    }
}

static int signal_stats_launch(const char *entry, hipStream_t stream, const float *pi, const float *dq_du, const double *act, int64_t n,
                               int32_t T, int32_t ad, double max_action, double action_l2, double flat, double *stats) {
    HP_TRY(episode_check_shape(entry, n, T));
    HP_REQUIRE(ad >= 1 && ad <= HP_POLICY_MAX_ACT_DIM, HP_ERR_INVALID, "%s: act_dim %d outside [1, %d]", entry, (int)ad,
               HP_POLICY_MAX_ACT_DIM);
    HP_REQUIRE(max_action > 0.0 && std::isfinite(max_action), HP_ERR_INVALID, "%s: max_action %g is not a positive number", entry, max_action);
    HP_REQUIRE(action_l2 >= 0.0 && std::isfinite(action_l2), HP_ERR_INVALID, "%s: action_l2 %g is not a finite number >= 0", entry, action_l2);
    HP_REQUIRE(flat >= 0.0 && std::isfinite(flat), HP_ERR_INVALID, "%s: flat %g is not a finite number >= 0", entry, flat);
    SignalStatsArgs A;
    A.pi = pi; A.dq_du = dq_du; A.act = act; A.stats = stats;
    A.max_action = (double)(float)max_action;       // the networks' own: float32
    A.action_l2 = action_l2; A.flat = flat;
    A.T = T; A.ad = ad;
    hipLaunchKernelGGL(k_episode_signal_stats, dim3((unsigned)n), dim3(64), 0, stream, A);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

extern "C" {

int hp_episode_action_grad(hp_agent *a, hp_norm *on, hp_norm *gn, int32_t target, int32_t at, const double *obs_dev, const double *g_dev,
                           const double *actions_dev, int64_t n_episodes, int32_t T, double clip_obs, float *pi_dev, float *q_dev,
                           float *dq_du_dev) {
    HP_REQUIRE(a && on && gn && obs_dev && g_dev && q_dev && dq_du_dev, HP_ERR_INVALID, "hp_episode_action_grad: null argument");
    HP_SERIALISE(a);
    HP_TRY(episode_one_context("hp_episode_action_grad", a, on, gn));
    return action_grad_launch("hp_episode_action_grad", a, on, gn, target, at,
                              EpisodeRows{obs_dev, nullptr, g_dev, actions_dev, -1, -1, -1, n_episodes, T}, clip_obs, pi_dev, q_dev, dq_du_dev);
}

int hp_episode_action_grad_block(hp_rollout *ro, hp_agent *a, hp_norm *on, hp_norm *gn, int32_t target, int32_t at, int64_t first_episode,
                                 int64_t n_episodes, double clip_obs, float *pi_dev, float *q_dev, float *dq_du_dev) {
    HP_REQUIRE(ro && a && on && gn && q_dev && dq_du_dev, HP_ERR_INVALID, "hp_episode_action_grad_block: null argument");
    HP_SERIALISE(ro);
    EpisodeRows rows;
    HP_TRY(episode_block_rows("hp_episode_action_grad_block", ro, a, on, gn, first_episode, n_episodes, rows));
    return action_grad_launch("hp_episode_action_grad_block", a, on, gn, target, at, rows, clip_obs, pi_dev, q_dev, dq_du_dev);
}

int hp_episode_signal_stats(hp_ctx *ctx, const float *pi_dev, const float *dq_du_dev, const double *actions_dev, int64_t n_episodes,
                            int32_t T, int32_t act_dim, double max_action, double action_l2, double flat, double *stats_dev) {
    HP_REQUIRE(ctx && pi_dev && dq_du_dev && actions_dev && stats_dev, HP_ERR_INVALID, "hp_episode_signal_stats: null argument");
    CtxGuard guard(ctx);
    return signal_stats_launch("hp_episode_signal_stats", ctx->stream, pi_dev, dq_du_dev, actions_dev, n_episodes, T, act_dim, max_action,
                               action_l2, flat, stats_dev);
}

int hp_episode_signal_stats_block(hp_rollout *ro, const float *pi_dev, const float *dq_du_dev, int64_t first_episode, int64_t n_episodes,
                                  double max_action, double action_l2, double flat, double *stats_dev) {
    HP_REQUIRE(ro && pi_dev && dq_du_dev && stats_dev, HP_ERR_INVALID, "hp_episode_signal_stats_block: null argument");
    HP_SERIALISE(ro);
    RolloutArrays arr;
    HP_TRY(episode_block_range("hp_episode_signal_stats_block", ro, first_episode, n_episodes, arr));
    return signal_stats_launch("hp_episode_signal_stats_block", ro->ctx->stream, pi_dev, dq_du_dev, arr.b_act, n_episodes, ro->T, ro->ad,
                               max_action, action_l2, flat, stats_dev);
}

}  // extern "C"
