// policy_call.h -- what a policy call is made of, host side: which parameter set, which normalizer statistics, which clips, the
// argument block of the policy slab (PolicyArgs, slab8.h) and the refusals every caller shares.  One definition for the policy
// calls themselves (agent_forward.hip), the rollouts (rollout.hip) and the episode audits (episode_nets.h: episode_q.hip, episode_policy.hip,
// episode_action_grad.hip, episode_bellman.hip).
// Include it behind slab8.h (any slab height, S8_DEVICE_ONLY or not): PolicyArgs and SlabNetPtrs come from there.
#pragma once
#include <cmath>

#include "agent.h"

// the online (fragF / fragD / params) or the target (fragFT / targets; no dX fragments) parameter set, the whole arena
inline SlabNetPtrs slab_net(const hp_agent *a, bool target) {
    return target ? SlabNetPtrs{a->fragFT, nullptr, a->targets} : SlabNetPtrs{a->fragF, a->fragD, a->params};
}

// clip_obs <= 0 means "no clip" behind the ABI; tr_net_input takes a bound
inline double clip_or_inf(double clip_obs) { return clip_obs > 0 ? clip_obs : INFINITY; }

// a normalizer's device side as a policy call reads it: an hp_norm or a policy snapshot's copy of one
struct NormView {
    const NormDev *d;
    double clip;
    int size;
};
inline NormView norm_view(const hp_norm *n) { return NormView{n->d, n->clip, (int)n->size}; }

// the normalizer half of a PolicyArgs (the one argument block that carries one: the episode audits' kernels carry a PolicyArgs);
// clip_obs as clip_or_inf returns it
inline void set_norm_inputs(PolicyArgs &A, const NormView &on, const NormView &gn, double clip_obs) {
    A.od = on.size; A.gd = gn.size;
    A.onz = on.d; A.gnz = gn.d;
    A.clip_obs = clip_obs; A.clip_o = on.clip; A.clip_g = gn.clip;
}

// a zeroed PolicyArgs with everything set but the rows' own pointers (obs / g / x / actions)
inline PolicyArgs policy_args(const hp_agent *a, const SlabNetPtrs &net, const NormView &on, const NormView &gn, double clip_obs,
                              int64_t rows) {
    PolicyArgs P;
    memset(&P, 0, sizeof(P));
    set_norm_inputs(P, on, gn, clip_obs);
    P.rows = (int)rows;
    P.net = net;
    P.la = a->la; P.H = a->H; P.act_dim = a->cfg.act_dim; P.max_action = (float)a->cfg.max_action;
    return P;
}

// The rule of the 4-row policy slab (s8_policy_slab / s8_critic_slab): the thin-slab engine's fragment copies, 256-wide layers, an
// input row that fits S8_LDX and a head of at most four rows.  `code` and `tail` are the caller's: the audits answer HP_ERR_STATE,
// the fused rollout HP_ERR_INVALID and what the caller keeps instead
inline int require_slab_shaped(const char *entry, const hp_agent *a, int code, const char *tail = "") {
    HP_REQUIRE(a->slab8 && a->H == 256 && a->ldx <= 48 && a->cfg.act_dim <= 4, code,
               "%s: the agent is not slab-shaped (hidden %d, padded input width %d, act_dim %d, engine %s)%s", entry, a->H, a->ldx,
               a->cfg.act_dim, a->slab8 ? "slab8" : "other", tail);
    return HP_OK;
}

// What hp_agent_act, hp_agent_act_dev, hp_agent_actor_forward and hp_agent_critic_forward refuse behind their null checks, in their
// order: contexts, the net's family (`actor`: the entry evaluates an actor, else a critic), the row count, the normalizers' sizes.
// on == nullptr: the entry takes no normalizers (its rows are network inputs already)
inline int check_policy_call(const char *entry, const hp_agent *a, const hp_norm *on, const hp_norm *gn, int32_t net, bool actor,
                             int64_t rows) {
    HP_REQUIRE(!on || (on->ctx == a->ctx && gn->ctx == a->ctx), HP_ERR_INVALID, "%s: handles belong to different contexts", entry);
    HP_REQUIRE(actor ? (net == HP_NET_ACTOR || net == HP_NET_ACTOR_TARGET) : (net == HP_NET_CRITIC || net == HP_NET_CRITIC_TARGET),
               HP_ERR_INVALID, "%s: net must be %s", entry, actor ? "an actor" : "a critic");
    HP_REQUIRE(rows > 0 && rows < (1 << 24), HP_ERR_INVALID, "%s: rows out of range", entry);
    HP_REQUIRE(!on || on->size + gn->size == a->xdim, HP_ERR_INVALID, "%s: normalizer sizes %d+%d do not match the actor input %d",
               entry, on ? (int)on->size : 0, on ? (int)gn->size : 0, a->xdim);
    return HP_OK;
}
