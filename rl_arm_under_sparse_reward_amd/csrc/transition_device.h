// transition_device.h -- the arithmetic of one transition, stated once: the squared goal distance and the reward taken on it, a
// network input out of a float64 row value, where a sampled transition's goal lies, and the move of a double between lanes.
// Every gather (sampler.hip, agent_engines.hip, agent_forward.hip, slab8.h), the normalizer (norm.hip, norm_device.h), the episode audit
// (episode_stats.hip, episode_returns.hip, episode_q.hip) and the environments' success test (env_device.h) call these.  Two
// sites keep an expression written out, with a comment that points here (k_gather_dict's distance loop, s8_gather's two inputs:
// the generated code is the reason, profiles/transition_arithmetic_refactor.txt).  They sit outside every S8_NS namespace, so slab8.h's instantiations share one definition.
//
// The library exists to give the reference's bits, and these expressions decide them for every transition the learner sees.
// Every operation whose rounding numpy / torch eager fix is an explicit IEEE operation (__dsub_rn, __dmul_rn, ...): each is
// rounded on its own and none can be contracted into a fused multiply-add (the units are built with -ffp-contract=off as well).
#pragma once
#include "internal.h"

// np.clip == minimum(maximum(v, lo), hi)
__device__ __forceinline__ double clipd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// ---- squared goal distance (goal_distance, bmirobot_env_push_F.py:20-23; her.py:38) ----------------------------------------------
// sum((a - b)^2) over gd components: differences, products and sums each rounded on their own, summed left to right, the first
// term unsummed -- numpy's add.reduce over a contiguous axis of fewer than 8 elements is a plain left-to-right sum, (x0 x0 + x1 x1)
// + x2 x2.  No root here: the predicates are taken on the square (hp_reward below, squared_bound in internal.h).
// Serial form: a and b are contiguous gd-vectors, one thread walks them.
__device__ __forceinline__ double tr_sq_distance(const double *a, const double *b, int gd) {
    double s = 0.0;
    for (int c = 0; c < gd; ++c) {
        const double d = __dsub_rn(a[c], b[c]);
        const double sq = __dmul_rn(d, d);
        s = (c == 0) ? sq : __dadd_rn(s, sq);
    }
    return s;
}
// Lane form: lane `first` + c of the wave holds component c.  tr_sq_term is a lane's own square, tr_sq_distance_lanes the same
// left-to-right sum of the squares of lanes first .. first + gd - 1, valid in every lane.  How the operands get into the lanes is
// the caller's layout.
__device__ __forceinline__ double tr_sq_term(double a, double b) {
    const double d = __dsub_rn(a, b);
    return __dmul_rn(d, d);
}
__device__ __forceinline__ double tr_sq_distance_lanes(double sq, int first, int gd) {
    double s = 0.0;
    for (int c = 0; c < gd; ++c) {
        const double sc = __shfl(sq, first + c);
        s = (c == 0) ? sc : __dadd_rn(s, sc);
    }
    return s;
}

// Reward of a relabelled transition from the squared goal distance s (compute_reward, bmirobot_env_push_F.py:84-90):
//   sq_threshold >= 0: sparse, -(d > thr) == -(s >= sq_threshold) with sq_threshold the smallest double whose correctly
//                      rounded square root exceeds thr (the square root is monotone) -- no square root on the device;
//   sq_threshold <  0: dense, -d (the env returns it in float64; the learner narrows it to float32, ddpg_agent.py:243).
__device__ __forceinline__ float hp_reward(double s, double sq_threshold) {
    if (sq_threshold < 0.0) return (float)(-__dsqrt_rn(s));
    return (s >= sq_threshold) ? -1.0f : -0.0f;
}
// the value compute_reward itself returns: float32 widened (sparse) or float64 -d (dense)
__device__ __forceinline__ double hp_reward64(double s, double sq_threshold) {
    if (sq_threshold < 0.0) return -__dsqrt_rn(s);
    return (s >= sq_threshold) ? -1.0 : -0.0;
}

// ---- network input ------------------------------------------------------------------------------------------------------------------
// normalizer.normalize (normalizer.py:67-70): clip((v - mean) / std, -clip, clip) in float64, the float32 mean widened.
__device__ __forceinline__ double tr_normalize(double v, float mean, double std, double clip) {
    return clipd(__ddiv_rn(__dsub_rn(v, (double)mean), std), -clip, clip);
}
// One network input out of a float64 row value (ddpg_agent._preproc_og :214-217 and _preproc_inputs :163-171): clip at clip_obs,
// normalise, narrow to float32.  tr_normalize is not this with an infinite clip_obs: fmax(NaN, -inf) is -inf, so the first clip
// replaces a NaN before the subtraction sees it.  The branch-free gathers hand an action through this function with mean 0, std 1
// and infinite clips on purpose: (v - 0) / 1 between them is v, exactly.
__device__ __forceinline__ float tr_net_input(double raw, double clip_obs, float mean, double std, double clip) {
    return (float)tr_normalize(clipd(raw, -clip_obs, clip_obs), mean, std, clip);
}

// ---- relabelled goal (her.py:35-36) -------------------------------------------------------------------------------------------------
// The goal of a drawn transition in the float64 layout ag [.][T + 1][gd], g [.][T][gd]: the achieved goal of the future step when
// the record is relabelled, the episode's own goal at t otherwise.  rec is a PlanRec lvalue (it is named more than once).
// A macro on purpose: as a function the two arms are simplified on their own before they meet their caller -- they become selects
// of base, row length and step in front of one multiply, and the record one 16-byte load -- which moved the register figures of
// every gather (profiles/transition_arithmetic_refactor.txt).  Expanded in place, a gather keeps its branch and shares
// e (T + 1) with its observation row.
#define TR_GOAL_SRC(rec, ag, g, T, gd) \
    ((rec).her ? (ag) + ((long long)(rec).e * ((T) + 1) + (rec).fut) * (gd) : (g) + ((long long)(rec).e * (T) + (rec).t) * (gd))

// ---- a double between lanes, as its two dwords ----------------------------------------------------------------------------------------
// x of lane (i ^ M), M < 32: ds_swizzle in bit-mask mode (the LDS crossbar: no memory, no address register)
template <int M> __device__ __forceinline__ int lane_xor_i(int x) { return __builtin_amdgcn_ds_swizzle(x, (M << 10) | 0x1F); }
template <int M> __device__ __forceinline__ double lane_xor_d(double x) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)lane_xor_i<M>((int)(unsigned)b), hi = (unsigned)lane_xor_i<M>((int)(unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// x of lane l, l wave-uniform (v_readlane)
__device__ __forceinline__ double lane_read_d(double x, int l) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
