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
#include "episode_nets.h"

struct EpisodeQArgs : EpisodeNetArgs {   // P.net: the critic's parameter set (the actor's layout P.la goes unread)
    using Lds = s8en::PolicyLds;
    const double *act;             // [n][T][ad], already offset to the first episode
    float *q;                      // [n][T]
};

__global__ __launch_bounds__(S8_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_episode_q(const EpisodeQArgs A) {
    __shared__ EpisodeQArgs::Lds L;
    const long long row0 = (long long)blockIdx.x * 4;
    const PolicyArgs &P = A.P;
    s8en::s8_critic_slab(P.net, A.lc, A.ca, P.H, (long long)P.rows, L, (size_t)row0,
        [&](int r, int c) -> float {
            const EpisodeRow w = episode_row(row0 + r, A.T);
            if (c < P.od + P.gd) return episode_state_column(P, w.e * (A.T + 1) + w.t, P.g + w.m * P.gd, c);
            return episode_action_column(P, A.act, w.m, A.act_off, c);
        },
        [&](int r, float q) { A.q[row0 + r] = q; });
}

// everything behind the entry's own checks (null arguments, contexts, the block's range): the remaining refusals in the order the
// header lists them, then the one launch
static int episode_q_launch(const char *entry, hp_agent *a, hp_norm *on, hp_norm *gn, int32_t net, const EpisodeRows &R, double clip_obs,
                            float *q) {
    HP_REQUIRE(net == HP_NET_CRITIC || net == HP_NET_CRITIC_TARGET, HP_ERR_INVALID, "%s: net must be a critic", entry);
    EpisodeQArgs A = {};
    HP_TRY(episode_net_args(entry, a, on, gn, "critic", slab_net(a, net != HP_NET_CRITIC), R, 1, clip_obs, A));
    A.act = R.act; A.q = q;
    return episode_net_launch(k_episode_q, a, A);
}

extern "C" {

int hp_episode_q(hp_agent *a, hp_norm *on, hp_norm *gn, int32_t net, const double *obs_dev, const double *g_dev,
                 const double *actions_dev, int64_t n_episodes, int32_t T, double clip_obs, float *q_dev) {
    HP_REQUIRE(a && on && gn && obs_dev && g_dev && actions_dev && q_dev, HP_ERR_INVALID, "hp_episode_q: null argument");
    HP_SERIALISE(a);
    HP_TRY(episode_one_context("hp_episode_q", a, on, gn));
    return episode_q_launch("hp_episode_q", a, on, gn, net, EpisodeRows{obs_dev, nullptr, g_dev, actions_dev, -1, -1, -1, n_episodes, T},
                            clip_obs, q_dev);
}

int hp_episode_q_block(hp_rollout *ro, hp_agent *a, hp_norm *on, hp_norm *gn, int32_t net, int64_t first_episode, int64_t n_episodes,
                       double clip_obs, float *q_dev) {
    HP_REQUIRE(ro && a && on && gn && q_dev, HP_ERR_INVALID, "hp_episode_q_block: null argument");
    HP_SERIALISE(ro);
    EpisodeRows rows;
    HP_TRY(episode_block_rows("hp_episode_q_block", ro, a, on, gn, first_episode, n_episodes, rows));
    return episode_q_launch("hp_episode_q_block", a, on, gn, net, rows, clip_obs, q_dev);
}

}  // extern "C"
