// episode_q.hip -- what the critic believes of every step of an episode block, computed where the block lies (hp_episode_q,
// hp_episode_q_block): Q(s_t, a_t) for t = 0 .. T-1 of every episode in ONE launch, out of the float64 rows the rollouts wrote, the
// normalizers' device statistics and the critic's forward-order weight fragments -- no upload, no download, no stream wait
// (hp_agent_critic_forward, the only other critic forward behind the ABI, takes host rows the caller has already clipped,
// normalised and scaled, and costs two uploads, seven launches, a download and a wait).
//
// The kernel is the critic half of the chain kernels (slab8.h, s8_critic_slab: the target critic's forward of fb_slab8_body with
// the network as an argument) inside the frame of the policy launch (k_policy_slab8): a 4-row slab per workgroup, the policy slab's
// LDS, one workgroup per CU.  Flat row m = e T + t; workgroup b owns rows 4b .. 4b+3, so a slab may straddle two episodes; obs has
// T + 1 rows per episode, g and actions T.  A row's input is built by the operations a transition meets on its way into an update
// (s8_gather): clip, subtract, divide, clip in float64 one rounding each (tr_net_input), the action narrowed to float32 and
// divided by max_action in float32 -- so a recorded transition enters the critic here exactly as it enters an update.
//
// Which weights.  Every launch form of an update sequence (one chain launch, the split launch with its tile launches, the
// layer-per-launch engine's Adam pass) writes the optimizer step through AdamFuse into ONE set of buffers: a->params (canonical)
// and a->fragF (forward fragments), and the polyak step into a->targets / a->fragFT (adam_fuse / adam_block in agent_engines.hip are
// the one place that writes them, slab_net in policy_call.h the one that reads them here; hp_agent_set_params / hp_agent_soft_update / hp_state_restore go through k_relayout / k_polyak_frag
// onto the same buffers).  There is no second copy to go stale: this launch reads those four, the critic's segment at la.total, on the
// context's stream behind whatever wrote them.
#include <cmath>

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wundefined-inline"   // agent_device.h declares the 32-row engine's fragment map, which no code here calls
#include "agent_device.h"
#pragma clang diagnostic pop

// the 4-row slab's device functions (no kernel of slab8.h is compiled here)
#define S8_DEVICE_ONLY
#define S8_NRG 1
#define S8_NS s8eq
#include "slab8.h"
#undef S8_NRG
#undef S8_NS
#undef S8_DEVICE_ONLY

#include "episode_audit.h"
#include "policy_call.h"

// (od / gd / onz / gnz / clip_obs / clip_o / clip_g keep PolicyArgs' names: set_norm_inputs, policy_call.h, fills them by name)
struct EpisodeQArgs {
    const double *obs, *g, *act;   // [n][T + 1][od], [n][T][gd], [n][T][ad], already offset to the first episode
    float *q;                      // [n][T]
    long long rows;                // n T
    int T, od, gd, ad, act_off;
    const NormDev *onz, *gnz;
    double clip_obs, clip_o, clip_g;
    SlabNetPtrs net;               // forward fragments + canonical arena of the parameter set to evaluate
    NetLayout lc;
    int ca, H;                     // the critic's segment starts at ca = la.total
    float max_action;
};

__global__ __launch_bounds__(S8_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_episode_q(const EpisodeQArgs A) {
    __shared__ s8eq::PolicyLds L;
    const long long row0 = (long long)blockIdx.x * 4;
    s8eq::s8_critic_slab(A.net, A.lc, A.ca, A.H, A.rows, L, (size_t)row0,
        [&](int r, int c) -> float {
            const long long m = row0 + r, e = m / A.T;
            const int t = (int)(m - e * A.T);
            if (c < A.od)
                return tr_net_input(A.obs[(e * (A.T + 1) + t) * A.od + c], A.clip_obs, A.onz->mean[c], A.onz->std[c], A.clip_o);
            if (c < A.od + A.gd) {
                const int j = c - A.od;
                return tr_net_input(A.g[m * A.gd + j], A.clip_obs, A.gnz->mean[j], A.gnz->std[j], A.clip_g);
            }
            const int j = c - A.act_off;
            if (j >= 0 && j < A.ad) return (float)A.act[m * A.ad + j] / A.max_action;   // s8_gather, k_pack_scaled_actions
            return 0.f;
        },
        [&](int r, float q) { A.q[row0 + r] = q; });
}

// everything behind the entry's own checks (null arguments, contexts, the block's range): the remaining refusals in the order the
// header lists them, then the one launch
static int episode_q_launch(const char *entry, hp_agent *a, hp_norm *on, hp_norm *gn, int32_t net, const double *obs,
                            const double *g, const double *act, int block_od, int block_gd, int block_ad, int64_t n, int32_t T,
                            double clip_obs, float *q) {
    HP_REQUIRE(net == HP_NET_CRITIC || net == HP_NET_CRITIC_TARGET, HP_ERR_INVALID, "%s: net must be a critic", entry);
    HP_TRY(require_slab_shaped(entry, a, HP_ERR_STATE));
    HP_REQUIRE(on->size + gn->size == a->xdim, HP_ERR_INVALID, "%s: normalizer sizes %d+%d do not match the critic input %d", entry,
               (int)on->size, (int)gn->size, a->xdim);
    HP_REQUIRE(block_od < 0 || (block_od == on->size && block_gd == gn->size && block_ad == a->cfg.act_dim), HP_ERR_INVALID,
               "%s: the block has dimensions %d / %d / %d, normalizers and agent have %d / %d / %d", entry, block_od, block_gd, block_ad,
               (int)on->size, (int)gn->size, a->cfg.act_dim);
    HP_TRY(episode_check_shape(entry, n, T));
    const long long rows = (long long)n * T;
    HP_REQUIRE(rows < (1LL << 31), HP_ERR_INVALID, "%s: %lld steps are more than one launch holds (2^31)", entry, rows);
    static_assert(sizeof(s8eq::PolicyLds) <= 160 * 1024, "the policy slab's LDS fits a CU");
    EpisodeQArgs A;
    memset(&A, 0, sizeof(A));
    A.obs = obs; A.g = g; A.act = act; A.q = q;
    A.rows = rows; A.T = T;
    set_norm_inputs(A, norm_view(on), norm_view(gn), clip_or_inf(clip_obs));   // the normalizer half, as PolicyArgs names it
    A.ad = a->cfg.act_dim; A.act_off = a->act_off;
    A.net = slab_net(a, net != HP_NET_CRITIC);
    A.lc = a->lc; A.ca = a->la.total; A.H = a->H;
    A.max_action = (float)a->cfg.max_action;
    hipLaunchKernelGGL(k_episode_q, dim3((unsigned)((rows + 3) / 4)), dim3(S8_THREADS), 0, a->ctx->stream, A);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

extern "C" {

int hp_episode_q(hp_agent *a, hp_norm *on, hp_norm *gn, int32_t net, const double *obs_dev, const double *g_dev,
                 const double *actions_dev, int64_t n_episodes, int32_t T, double clip_obs, float *q_dev) {
    HP_REQUIRE(a && on && gn && obs_dev && g_dev && actions_dev && q_dev, HP_ERR_INVALID, "hp_episode_q: null argument");
    HP_SERIALISE(a);
    HP_REQUIRE(on->ctx == a->ctx && gn->ctx == a->ctx, HP_ERR_INVALID, "hp_episode_q: handles belong to different contexts");
    return episode_q_launch("hp_episode_q", a, on, gn, net, obs_dev, g_dev, actions_dev, -1, -1, -1, n_episodes, T, clip_obs, q_dev);
}

int hp_episode_q_block(hp_rollout *ro, hp_agent *a, hp_norm *on, hp_norm *gn, int32_t net, int64_t first_episode, int64_t n_episodes,
                       double clip_obs, float *q_dev) {
    HP_REQUIRE(ro && a && on && gn && q_dev, HP_ERR_INVALID, "hp_episode_q_block: null argument");
    HP_SERIALISE(ro);
    HP_REQUIRE(a->ctx == ro->ctx && on->ctx == ro->ctx && gn->ctx == ro->ctx, HP_ERR_INVALID,
               "hp_episode_q_block: handles belong to different contexts");
    RolloutArrays at;
    HP_TRY(episode_block_range("hp_episode_q_block", ro, first_episode, n_episodes, at));
    return episode_q_launch("hp_episode_q_block", a, on, gn, net, at.b_obs, at.b_g, at.b_act, ro->od, ro->gd, ro->ad, n_episodes, ro->T,
                            clip_obs, q_dev);
}

}  // extern "C"
