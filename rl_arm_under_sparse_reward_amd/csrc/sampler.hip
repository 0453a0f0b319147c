// sampler.hip -- the stand-alone sampler: HER gather / relabel / reward kernels over the replay storage of buffer.hip, their
// launchers, and the hp_buffer_sample* entries (reference: her.py:26-39, ddpg_agent.py:227-243, bmirobot_env_push_F.py:84-90).
//
// A sampled transition touches obs[e][t..t+1] (one contiguous 2*obs_dim run), ag[e][t..t+1], g[e][t], actions[e][t] and, when
// relabelled, ag[e][future_t] of the float64 arrays (layout: buffer.hip), or the throughput rows that buffer.hip packs from them.
//
// The arithmetic of a transition (reward, network input, relabelled goal): transition_device.h.
#include "transition_device.h"

// ----------------------------------------------------------------------------- kernels
// One wavefront per transition; lanes stride over the row elements (coalesced 8-byte loads).
// dict-mode output = the arrays her_sampler.sample_her_transitions returns (her.py:39).
__global__ __launch_bounds__(256) void k_gather_dict(const double *__restrict__ obs, const double *__restrict__ ag,
                                                     const double *__restrict__ g, const double *__restrict__ act,
                                                     const PlanRec *__restrict__ plan, long long batch, int T,
                                                     int obs_dim, int goal_dim, int act_dim, double sq_threshold,
                                                     double *o_obs, double *o_ag, double *o_g, double *o_act,
                                                     double *o_obs_next, double *o_ag_next, float *o_r,
                                                     double *o_r64) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= batch) return;
    const PlanRec rec = plan[i];
    const long long e = rec.e;
    const int t = rec.t;
    const double *obs_row = obs + (e * (T + 1) + t) * obs_dim;        // rows t and t+1 are adjacent
    const double *ag_row = ag + (e * (T + 1) + t) * goal_dim;
    const double *g_src = TR_GOAL_SRC(rec, ag, g, T, goal_dim);
    const double *act_row = act + (e * T + t) * act_dim;
    for (int c = lane; c < obs_dim; c += 64) {
        o_obs[i * obs_dim + c] = obs_row[c];
        o_obs_next[i * obs_dim + c] = obs_row[obs_dim + c];
    }
    for (int c = lane; c < goal_dim; c += 64) {
        o_ag[i * goal_dim + c] = ag_row[c];
        o_ag_next[i * goal_dim + c] = ag_row[goal_dim + c];
        o_g[i * goal_dim + c] = g_src[c];
    }
    for (int c = lane; c < act_dim; c += 64) o_act[i * act_dim + c] = act_row[c];
    if (lane == 0) {
        // tr_sq_distance (transition_device.h), written out: the index goal_dim + c is summed in int, as the copy loop above sums it;
        // handing ag_row + goal_dim to the function forms that address in 64 bits and costs the kernel two VGPRs and two SGPRs
        double s = 0.0;
        for (int c = 0; c < goal_dim; ++c) {
            const double d = __dsub_rn(ag_row[goal_dim + c], g_src[c]);
            const double sq = __dmul_rn(d, d);
            s = (c == 0) ? sq : __dadd_rn(s, sq);
        }
        o_r[i] = hp_reward(s, sq_threshold);  // -(d > thr).astype(float32), or float32(-d)
        // what compute_reward itself returns (:87-90): the float32 above widened (sparse) or -d in float64 (dense)
        if (o_r64) o_r64[i] = hp_reward64(s, sq_threshold);
    }
}

// The learner's view of a minibatch (ddpg_agent.py:227-243) straight out of the replay buffer: gather (her.py:26), relabel
// (:35-36), reward (:38), _preproc_og clip (:214-217), both normalizers (normalizer.py:67-70), concatenate, float32 -- the
// arithmetic of the chain kernels' in-launch gather (slab8.h s8_gather), as a kernel of its own with DEVICE outputs:
//   x [B][od+gd] = norm(clip(obs[e][t])) | norm(clip(g'))      x_next = norm(clip(obs[e][t+1])) | norm(clip(g'))
//   a [B][ad]    = float32(actions[e][t])  (the critic divides by max_action itself, models.py:38)     r [B]
// One wavefront per transition, FS_FLIGHT transitions in flight per wavefront.  A transition's source elements are
// [obs t | obs t+1 | ag t+1 | g' | action] = 2 od + 2 gd + ad doubles -- exactly 64 for the bmirobot shapes (27, 3, 4), i.e.
// ONE 8-byte load per lane, of which the first 54 lanes read one contiguous 432-byte run.  HBM-bound: 67 doubles read,
// 65 floats written per transition.
struct FusedSampleArgs {
    const double *obs, *ag, *g, *act;
    const PlanRec *plan;
    const NormDev *onz, *gnz;
    long long batch;
    int T, od, gd, ad;
    double sq_threshold, clip_obs, clip_o, clip_g;
    float *x, *xn, *a, *r;
    long long *o_e, *o_t, *o_fut;
    unsigned char *o_her;
    // fast draw (hp_buffer_sample_dev_fast; SURVEY 8b rng_mode = Philox): no plan, the index record of transition m of call
    // `fast_call` is Philox4x32-10((m, call); seed) -- fs_fast_rec below
    unsigned long long fast_seed, fast_call;
    int fast_n_eps;
    double fast_future_p;
};

// ---- fast draw: counter-based indices instead of the reference's sequential MT19937 stream (opt-in, NOT the reference's draws) ------
// her.py:24-33 draws e = randint(N), t = randint(T), u1, u2 from ONE global stream, which makes the index draw of a large batch a
// sequential kernel (2.0 ms per 2^18 transitions against 59 us for their gather).  Fast mode keys every transition by its own counter:
//   (r0, r1, r2, r3) = Philox4x32-10(counter = (m lo, m hi, call lo, call hi), key = (seed lo, seed hi))      [Random123, Salmon et al. SC11]
//   e = floor(r0 N / 2^32), t = floor(r1 T / 2^32), her = r2 2^-32 < future_p, future_t = t + 1 + floor(r3 (T - t) / 2^32)
// -- her.py's four draws with multiply-shift bounded integers (bias <= N / 2^32) -- so the draw costs a few dozen integer
// instructions inside the gather kernel.  Deterministic in (seed, call, m); pinned by Random123's known-answer vectors and an
// numpy twin in the test infrastructure (draw_her_indices_fast).
__device__ __forceinline__ void fs_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                                 unsigned (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ PlanRec fs_fast_rec(const FusedSampleArgs &A, long long m) {
    unsigned r[4];
    fs_philox4x32_10((unsigned)m, (unsigned)((unsigned long long)m >> 32), (unsigned)A.fast_call, (unsigned)(A.fast_call >> 32),
                     (unsigned)A.fast_seed, (unsigned)(A.fast_seed >> 32), r);
    PlanRec rec;
    rec.e = (int)(((unsigned long long)r[0] * (unsigned)A.fast_n_eps) >> 32);
    rec.t = (int)(((unsigned long long)r[1] * (unsigned)A.T) >> 32);
    rec.her = ((double)r[2] * 0x1p-32 < A.fast_future_p) ? 1 : 0;
    rec.fut = rec.t + 1 + (int)(((unsigned long long)r[3] * (unsigned)(A.T - rec.t)) >> 32);
    return rec;
}
// the records of the 2 x FLIGHT transitions of one pass: lane j draws transition base + j, every lane picks up its half's
template <int FLIGHT>
__device__ __forceinline__ void fs_fast_recs(const FusedSampleArgs &A, long long base, int lane, int h, PlanRec (&rec)[FLIGHT]) {
    const long long mj = base + (lane & (2 * FLIGHT - 1));
    const PlanRec mine = fs_fast_rec(A, mj < A.batch ? mj : A.batch - 1);
#pragma unroll
    for (int k = 0; k < FLIGHT; ++k) {
        const int src = 2 * k + h;
        rec[k].e = __shfl(mine.e, src);
        rec[k].t = __shfl(mine.t, src);
        rec[k].fut = __shfl(mine.fut, src);
        rec[k].her = __shfl(mine.her, src);
    }
}

// what the first lane of a transition leaves of it beside its rows: the reward (her.py:38) and the index record
__device__ __forceinline__ void fs_store_record(const FusedSampleArgs &A, long long m, double sq_distance, const PlanRec &rec) {
    if (A.r) A.r[m] = hp_reward(sq_distance, A.sq_threshold);
    if (A.o_e) A.o_e[m] = rec.e;
    if (A.o_t) A.o_t[m] = rec.t;
    if (A.o_fut) A.o_fut[m] = rec.fut;
    if (A.o_her) A.o_her[m] = (unsigned char)rec.her;
}

// FLIGHT transitions per wavefront and pass: 1 for small batches (one minibatch = two dependent memory latencies, as many
// wavefronts as transitions), 4 from 16 Ki transitions on (more bytes in flight per wavefront, grid-stride).  Every load of a
// pass -- the lanes' source elements AND the reward's operands -- is issued before the first value is used.
template <int FLIGHT>
__global__ __launch_bounds__(256) void k_gather_fused(const FusedSampleArgs A) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
    const int od = A.od, gd = A.gd, ad = A.ad, ldx = od + gd, Q = 2 * od + 2 * gd + ad;
    // what this lane's source element is in the first strip of 64 (the only one for the bmirobot shapes): 0 obs t, 1 obs t+1,
    // 2 ag t+1 (reward only), 3 g', 4 action, 5 nothing
    auto kind_of = [&](int q) { return q < od ? 0 : q < 2 * od ? 1 : q < 2 * od + gd ? 2 : q < 2 * od + 2 * gd ? 3 : q < Q ? 4 : 5; };
    auto col_of = [&](int q, int kind) { return kind == 0 ? q : kind == 1 ? q - od : kind == 2 ? q - 2 * od : kind == 3 ? q - 2 * od - gd : q - 2 * od - 2 * gd; };
    const int rc = lane < gd ? lane : gd - 1;      // reward operands: lanes < gd, one goal component each
    for (long long base = wave * FLIGHT; base < A.batch; base += n_waves * FLIGHT) {
        PlanRec rec[FLIGHT];
#pragma unroll
        for (int k = 0; k < FLIGHT; ++k) rec[k] = A.plan[base + k < A.batch ? base + k : A.batch - 1];
        const double *obs0[FLIGHT], *g_src[FLIGHT];
        double ra[FLIGHT], rg[FLIGHT];
#pragma unroll
        for (int k = 0; k < FLIGHT; ++k) {
            const long long e = rec[k].e;
            const int t = rec[k].t;
            obs0[k] = A.obs + (e * (A.T + 1) + t) * od;
            g_src[k] = TR_GOAL_SRC(rec[k], A.ag, A.g, A.T, gd);
            ra[k] = A.ag[(e * (A.T + 1) + t + 1) * gd + rc];
            rg[k] = g_src[k][rc];
        }
        for (int q0 = 0; q0 < Q; q0 += 64) {   // one pass for the bmirobot shapes
            const int q = q0 + lane, kind = kind_of(q), j = col_of(q, kind);
            float mu = 0.f;
            double sd = 1.0, clip = 0.0;
            if (kind <= 1) { mu = A.onz->mean[j]; sd = A.onz->std[j]; clip = A.clip_o; }
            if (kind == 3) { mu = A.gnz->mean[j]; sd = A.gnz->std[j]; clip = A.clip_g; }
            double v[FLIGHT];
#pragma unroll
            for (int k = 0; k < FLIGHT; ++k) {
                const long long e = rec[k].e;
                const int t = rec[k].t;
                // address-selected, unconditional load (idle lanes re-read element 0 of the observation row)
                const double *p = kind <= 1 ? obs0[k] + q : kind == 2 ? A.ag + (e * (A.T + 1) + t + 1) * gd + j
                                : kind == 3 ? g_src[k] + j : kind == 4 ? A.act + (e * A.T + t) * ad + j : obs0[k];
                v[k] = *p;
            }
#pragma unroll
            for (int k = 0; k < FLIGHT; ++k) {
                const long long m = base + k;
                if (m >= A.batch) continue;
                if (kind <= 1 || kind == 3) {
                    const float x = tr_net_input(v[k], A.clip_obs, mu, sd, clip);
                    if (kind == 0) { if (A.x) A.x[m * ldx + j] = x; }
                    else if (kind == 1) { if (A.xn) A.xn[m * ldx + j] = x; }
                    else {
                        if (A.x) A.x[m * ldx + od + j] = x;
                        if (A.xn) A.xn[m * ldx + od + j] = x;
                    }
                } else if (kind == 4) {
                    if (A.a) A.a[m * ad + j] = (float)v[k];
                }
            }
        }
        // reward: lanes < gd hold (ag_next - g')^2 of their component (tr_sq_distance_lanes)
#pragma unroll
        for (int k = 0; k < FLIGHT; ++k) {
            const long long m = base + k;
            const double s = tr_sq_distance_lanes(tr_sq_term(ra[k], rg[k]), 0, gd);
            if (m < A.batch && lane == 0) fs_store_record(A, m, s, rec[k]);
        }
    }
}

// The same kernel with 16-byte loads and TWO transitions per wavefront instruction (round 6).  A transition's sources are three
// vectors of doubles -- the contiguous [obs t | obs t+1] run (2 od), g' (gd), the action (ad) -- cut into units of two doubles: od +
// ceil(gd / 2) + ceil(ad / 2) units = 31 for the bmirobot shapes (27, 3, 4), so 32 lanes carry a transition with ONE 16-byte load
// each (rows are 8-byte aligned; the last unit of an odd-length vector loads [len - 2, len - 1] and keeps its second double, so no
// load reads past a row) and a wavefront instruction carries two.  Against k_gather_fused: half the load instructions per
// transition for the same bytes, 2 x FLIGHT transitions in flight per wavefront instead of FLIGHT, the normalizers' mean / std
// fetched once per lane instead of once per pass, g' of the reward taken from the units already loaded (one extra 8-byte load per
// transition pair for ag[t + 1] instead of two).  Same arithmetic per element: identical bits.  Shapes that do not fit 32 lanes
// take k_gather_fused.
// (us per 2^18 / 2^20 transitions, float64 rows | float32 rows, branch-free kernels: FLIGHT 2: 56.1 / 234.6 | 62.3 / 242.9; 4: 59.2 / 233.6 |
// 58.2 / 224.0; 8: 77.1 / 291.4 | 74.8 / 283.8)
#ifndef FS2_FLIGHT
#define FS2_FLIGHT 4
#endif
typedef double fs_d2 __attribute__((ext_vector_type(2), aligned(8)));
template <int FLIGHT, bool FAST = false>
__global__ __launch_bounds__(256) void k_gather_fused2(const FusedSampleArgs A) {
    const int lane = threadIdx.x & 63, l = lane & 31, h = lane >> 5;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
    const int od = A.od, gd = A.gd, ad = A.ad, ldx = od + gd;
    const int ug = (gd + 1) >> 1, ua = (ad + 1) >> 1;
    // this lane's unit: 0 = two doubles of the [obs t | obs t+1] run, 1 = of g', 2 = of the action, 3 = none
    const int unit = l < od ? 0 : l < od + ug ? 1 : l < od + ug + ua ? 2 : 3;
    const int j = unit == 0 ? l : unit == 1 ? l - od : l - od - ug;
    const int len = unit == 0 ? 2 * od : unit == 1 ? gd : ad;
    const bool tail = unit != 3 && 2 * j + 1 >= len;      // last unit of an odd-length vector
    const int e0 = unit == 3 ? 0 : (tail ? len - 2 : 2 * j);
    // per slot (the unit's two doubles): where it goes -- a primary output row (x, x_next or actions; nullptr: nowhere) and, for g',
    // x_next as well -- and the constants of ONE branch-free expression for every lane: normalised elements clip at clip_obs, subtract
    // their mean, divide by their std, clip at the normaliser's range; an action passes through it unchanged ((v - 0) / 1 between
    // infinite clips is v, exactly).  (The first version branched per destination: 142 branches in the kernel, as many scalar
    // instructions as vector ones.)
    float *p0[2], *p1[2];
    int stride0[2], off[2];
    float mu[2] = {0.f, 0.f};
    double sd[2] = {1.0, 1.0}, clip[2] = {INFINITY, INFINITY}, cobs[2] = {INFINITY, INFINITY};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int el = e0 + s;
        const bool ok = unit != 3 && !(tail && s == 0);
        p0[s] = p1[s] = nullptr;
        stride0[s] = ldx;
        off[s] = 0;
        if (ok && unit == 0) {
            const int col = el < od ? el : el - od;
            p0[s] = el < od ? A.x : A.xn;
            off[s] = col;
            mu[s] = A.onz->mean[col]; sd[s] = A.onz->std[col]; clip[s] = A.clip_o; cobs[s] = A.clip_obs;
        } else if (ok && unit == 1) {
            p0[s] = A.x;
            p1[s] = A.xn;               // g_next := g (ddpg_agent.py:231)
            off[s] = od + el;
            mu[s] = A.gnz->mean[el]; sd[s] = A.gnz->std[el]; clip[s] = A.clip_g; cobs[s] = A.clip_obs;
        } else if (ok) {
            p0[s] = A.a;
            stride0[s] = ad;
            off[s] = el;
        }
    }
    // reward operands: lanes l < gd of each half hold component l.  g'[c] sits in lane od + (c / 2) -- the last unit for the last
    // component of an odd gd -- slot c % 2 (slot 1 there)
    const int rc = l < gd ? l : gd - 1;
    const bool rc_tail = (gd & 1) && rc == gd - 1;
    const int g_lane = (h << 5) + od + (rc_tail ? ug - 1 : (rc >> 1)), g_slot = rc_tail ? 1 : (rc & 1);
    for (long long base = wave * (2 * FLIGHT); base < A.batch; base += n_waves * (2 * FLIGHT)) {
        PlanRec rec[FLIGHT];
        if constexpr (FAST) {
            fs_fast_recs<FLIGHT>(A, base, lane, h, rec);
        } else {
#pragma unroll
            for (int k = 0; k < FLIGHT; ++k) {
                const long long m = base + 2 * k + h;
                rec[k] = A.plan[m < A.batch ? m : A.batch - 1];
            }
        }
        fs_d2 v[FLIGHT];
        double ra[FLIGHT];
#pragma unroll
        for (int k = 0; k < FLIGHT; ++k) {      // every load of the pass before the first use
            const long long e = rec[k].e;
            const int t = rec[k].t;
            const double *obs0 = A.obs + (e * (A.T + 1) + t) * od;
            const double *g_src = TR_GOAL_SRC(rec[k], A.ag, A.g, A.T, gd);
            const double *p = unit == 0 ? obs0 + e0 : unit == 1 ? g_src + e0 : unit == 2 ? A.act + (e * A.T + t) * ad + e0 : obs0;
            v[k] = *reinterpret_cast<const fs_d2 *>(p);
            ra[k] = A.ag[(e * (A.T + 1) + t + 1) * gd + rc];
        }
#pragma unroll
        for (int k = 0; k < FLIGHT; ++k) {
            const long long m = base + 2 * k + h;
            const bool live = m < A.batch;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const double val = s ? v[k].y : v[k].x;
                const float x = tr_net_input(val, cobs[s], mu[s], sd[s], clip[s]);
                if (live && p0[s]) p0[s][m * stride0[s] + off[s]] = x;
                if (live && p1[s]) p1[s][m * ldx + off[s]] = x;
            }
            // reward (her.py:38): (ag_next - g')^2 per component in lanes l < gd of the half (tr_sq_distance_lanes)
            const double gx = __shfl(v[k].x, g_lane), gy = __shfl(v[k].y, g_lane);
            const double sum = tr_sq_distance_lanes(tr_sq_term(ra[k], g_slot ? gy : gx), h << 5, gd);
            if (live && l == 0) fs_store_record(A, m, sum, rec[k]);
        }
    }
}

// hp_buffer_sample_dev on the throughput rows (buffer.hip k_pack_rows: one (episode, timestep) = one 128-byte line of float32
// [obs_t | action_t | 0], the goals float64 as [ag_t | g_t | 0] per 64 bytes).  32 lanes per transition, two transitions per
// wavefront instruction, ONE 16-byte
// load per lane: lanes 0-14 the float4s of the two adjacent row lines (row t: obs | action, row t + 1: obs), lanes 15 and 31 the
// two halves of g' (= ag[future_t] when relabelled, her.py:35-36, else the g half of goal row t), lanes 16 and 17 ag[t + 1] for the
// reward.  Each row lane then hands components 2, 3 of its float4 to the lane 16 above it, so that all 32 lanes carry two
// elements through ONE pass of the float64 clip / normalise arithmetic (the kernel is bound by that arithmetic as much as by
// bytes: a first version that kept four components per lane ran 104 us per 2^18 transitions against 68 for the float64 rows).
// Needs obs_dim <= 28, obs_dim + act_dim <= 32, goal_dim <= 4 (hp_buffer_enable_f32_rows checks).
struct PackedSampleArgs {
    const float *p_row;
    const double *p_goal;
    int row_w, goal_w;
    FusedSampleArgs f;
};
template <int FLIGHT, bool FAST = false>
__global__ __launch_bounds__(256) void k_gather_packed(const PackedSampleArgs P) {
    const FusedSampleArgs &A = P.f;
    const int lane = threadIdx.x & 63, l = lane & 31, h = lane >> 5;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
    const int od = A.od, gd = A.gd, ad = A.ad, ldx = od + gd, rw = P.row_w, gw = P.goal_w;
    // what this lane LOADS: 0 a row float4 (lanes 0-14: column 4 l of the 64-float [row t | row t + 1] pair), 1 a g' half (lane
    // 15: doubles 0, 1; lane 31: doubles 2, 3), 2 an ag[t + 1] half (lanes 16, 17), 3 nothing
    const int load = l < 15 ? 0 : (l == 15 || l == 31) ? 1 : (l == 16 || l == 17) ? 2 : 3;
    const int gj = l == 31 ? 1 : 0;                        // which half of g'
    // what this lane COMPUTES, two slots: lanes 0-14 columns 4 l + s, lanes 16-30 columns 4 (l - 16) + 2 + s (handed down by lane
    // l - 16), lanes 15 / 31 the goal components 2 gj + s.  Per slot: a primary output row (x, x_next or actions; nullptr: nowhere),
    // x_next as well for a goal component, and the constants of one branch-free clip / normalise expression (an action passes
    // through it unchanged: (v - 0) / 1 between infinite clips), as in k_gather_fused2
    float *p0[2], *p1[2];
    int stride0[2], off[2];
    bool goal[2] = {false, false};
    float mu[2] = {0.f, 0.f};
    double sd[2] = {1.0, 1.0}, clip[2] = {INFINITY, INFINITY}, cobs[2] = {INFINITY, INFINITY};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        p0[s] = p1[s] = nullptr;
        stride0[s] = ldx;
        off[s] = 0;
        if (load == 1) {
            const int c = 2 * gj + s;
            if (c < gd) {
                goal[s] = true;
                p0[s] = A.x; p1[s] = A.xn;                               // g_next := g (ddpg_agent.py:231)
                off[s] = od + c; mu[s] = A.gnz->mean[c]; sd[s] = A.gnz->std[c]; clip[s] = A.clip_g; cobs[s] = A.clip_obs;
            }
        } else if (l != 15 && l != 31) {
            const int col = 4 * (l & 15) + 2 * (l >> 4) + s;          // column of the 64-float pair
            const int oc = col < rw ? col : col - rw;                 // ... inside its row
            if (oc < od) {
                p0[s] = col < rw ? A.x : A.xn;
                off[s] = oc; mu[s] = A.onz->mean[oc]; sd[s] = A.onz->std[oc]; clip[s] = A.clip_o; cobs[s] = A.clip_obs;
            } else if (col < rw && oc < od + ad) {
                p0[s] = A.a;
                stride0[s] = ad;
                off[s] = oc - od;
            }
        }
    }
    const int rc = l < gd ? l : gd - 1;                   // reward: lanes l < gd of each half hold component l
    const int a_lane = (h << 5) + 16 + (rc >> 1), g_lane = (h << 5) + (rc < 2 ? 15 : 31), r_slot = rc & 1;
    const int from = (h << 5) + (l & 15);                 // the row lane a lane 16-30 takes its components from
    typedef float f4_t __attribute__((ext_vector_type(4)));
    typedef double d2_t __attribute__((ext_vector_type(2)));
    typedef float f4_a8 __attribute__((ext_vector_type(4), aligned(8)));
    union Ld { f4_t f; d2_t d; };
    for (long long base = wave * (2 * FLIGHT); base < A.batch; base += n_waves * (2 * FLIGHT)) {
        PlanRec rec[FLIGHT];
        if constexpr (FAST) {
            fs_fast_recs<FLIGHT>(A, base, lane, h, rec);
        } else {
#pragma unroll
            for (int k = 0; k < FLIGHT; ++k) {
                const long long m = base + 2 * k + h;
                rec[k] = A.plan[m < A.batch ? m : A.batch - 1];
            }
        }
        Ld v[FLIGHT];
#pragma unroll
        for (int k = 0; k < FLIGHT; ++k) {      // every load of the pass before the first use
            const long long e = rec[k].e;
            const int t = rec[k].t;
            const float *row = P.p_row + (e * (A.T + 1) + t) * rw;
            const double *goal_t = P.p_goal + (e * (A.T + 1) + t) * gw;
            // g': the ag half of goal row future_t, or the g half (doubles gd ..) of goal row t -- her.py:35-36 on the packed goal
            // rows [ag_t | g_t], another layout than tr_goal_src's, so the selection is written out here
            const double *gsrc = rec[k].her ? P.p_goal + (e * (A.T + 1) + rec[k].fut) * gw : goal_t + gd;
            const void *p = load == 0 ? (const void *)(row + 4 * l) : load == 1 ? (const void *)(gsrc + 2 * gj)
                          : load == 2 ? (const void *)(goal_t + gw + 2 * (l - 16)) : (const void *)row;
            v[k].f = *reinterpret_cast<const f4_a8 *>(p);
        }
#pragma unroll
        for (int k = 0; k < FLIGHT; ++k) {
            const long long m = base + 2 * k + h;
            const bool live = m < A.batch;
            // components 2, 3 of row lane l go to lane l + 16
            const float z = __shfl(v[k].f[2], from), w = __shfl(v[k].f[3], from);
            const float lo = l < 16 ? v[k].f[0] : z, hi = l < 16 ? v[k].f[1] : w;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float raw = s ? hi : lo;
                const double x = goal[s] ? v[k].d[s] : (double)raw;
                const float o = tr_net_input(x, cobs[s], mu[s], sd[s], clip[s]);
                if (live && p0[s]) p0[s][m * stride0[s] + off[s]] = o;
                if (live && p1[s]) p1[s][m * ldx + off[s]] = o;
            }
            // reward (her.py:38) on the float64 goals (tr_sq_distance_lanes)
            const double ax = __shfl(v[k].d[0], a_lane), ay = __shfl(v[k].d[1], a_lane);
            const double gx = __shfl(v[k].d[0], g_lane), gy = __shfl(v[k].d[1], g_lane);
            const double sum = tr_sq_distance_lanes(tr_sq_term(r_slot ? ay : ax, r_slot ? gy : gx), h << 5, gd);
            if (live && l == 0) fs_store_record(A, m, sum, rec[k]);
        }
    }
}

// ------------------------------------------------------------------------------ launchers
int buffer_launch_gather_dict(hp_buffer *b, const PlanRec *d_plan, int64_t batch, double sq_threshold, double *d_out,
                              float *d_r, double *d_r64) {
    const int od = b->obs_dim, gd = b->goal_dim, ad = b->act_dim;
    double *o_obs = d_out;
    double *o_ag = o_obs + batch * od;
    double *o_g = o_ag + batch * gd;
    double *o_act = o_g + batch * gd;
    double *o_obs_next = o_act + batch * ad;
    double *o_ag_next = o_obs_next + batch * od;
    const int waves_per_block = 4;
    dim3 grid((unsigned)((batch + waves_per_block - 1) / waves_per_block));
    hipLaunchKernelGGL(k_gather_dict, grid, dim3(256), 0, b->ctx->stream, b->d_obs, b->d_ag, b->d_g, b->d_act, d_plan,
                       (long long)batch, (int)b->T, od, gd, ad, sq_threshold, o_obs, o_ag, o_g, o_act, o_obs_next,
                       o_ag_next, d_r, d_r64);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

// The launch rule of the fused kernels.  Transitions in flight per wavefront (or, the two-transition kernels, pairs of them): 1
// for small batches, `deep` from 16 Ki transitions on (the kernels' FLIGHT).  Grid: `per_wave` transitions per wavefront and
// pass, four wavefronts per workgroup, grid-stride beyond 32 workgroups per compute unit.
// (k_gather_fused, us per 262144 transitions of a 5000-episode shard: 4 in flight, grid capped at 8 / 32 workgroups per CU 126.8 /
// 121.0; 8 in flight 133.6; 2 in flight, cap 16: 130.5; 1 in flight, cap 64: 124.0 -- ~2.1 G transitions/s whatever the shape)
static int gather_flight(int64_t batch, int deep) { return batch >= 16384 ? deep : 1; }
static dim3 gather_grid(const hp_buffer *b, int64_t batch, int per_wave) {
    const int64_t waves = (batch + per_wave - 1) / per_wave, wgs = (waves + 3) / 4, cap = (int64_t)b->ctx->cu_count * 32;
    return dim3((unsigned)(wgs < cap ? wgs : cap));
}
// the <FLIGHT, FAST> instantiation of a two-transition kernel that the rule picks; K names the kernel (Fused2 / Packed below)
struct Fused2 {
    template <int FLIGHT, bool FAST> static constexpr auto kernel = k_gather_fused2<FLIGHT, FAST>;
};
struct Packed {
    template <int FLIGHT, bool FAST> static constexpr auto kernel = k_gather_packed<FLIGHT, FAST>;
};
template <class K, class Args> static void launch_gather2(const hp_buffer *b, int64_t batch, bool fast, const Args &args) {
    const int flight = gather_flight(batch, FS2_FLIGHT);
    const dim3 grid = gather_grid(b, batch, 2 * flight);
    hipStream_t s = b->ctx->stream;
    if (flight != 1 && fast) hipLaunchKernelGGL((K::template kernel<FS2_FLIGHT, true>), grid, dim3(256), 0, s, args);
    else if (flight != 1) hipLaunchKernelGGL((K::template kernel<FS2_FLIGHT, false>), grid, dim3(256), 0, s, args);
    else if (fast) hipLaunchKernelGGL((K::template kernel<1, true>), grid, dim3(256), 0, s, args);
    else hipLaunchKernelGGL((K::template kernel<1, false>), grid, dim3(256), 0, s, args);
}

// replay_buffer.sample + the learner's preprocessing (ddpg_agent.py:227-243) with device outputs: the fused gather behind an
// index draw.  f32_rows: from the throughput rows (k_gather_packed); else 16-byte loads where the shapes fit 32 lanes
// (k_gather_fused2: the reference's shapes), else k_gather_fused.  Asynchronous on the context's stream; the outputs are
// caller-owned device memory (e.g. torch tensors).
struct FastDraw {   // hp_buffer_sample_dev_fast: counter-based index draw inside the gather kernel (fs_fast_rec)
    uint64_t seed, call;
    double future_p;
};
static int launch_gather(hp_buffer *b, bool f32_rows, const PlanRec *d_plan, hp_norm *on, hp_norm *gn, int64_t batch,
                         double sq_threshold, double clip_obs, const hp_sample_dev_out *o, const FastDraw *fast = nullptr) {
    PackedSampleArgs P;
    P.p_row = b->p_row; P.p_goal = b->p_goal; P.row_w = b->row_w; P.goal_w = b->goal_w;
    FusedSampleArgs &A = P.f;
    A.fast_seed = fast ? fast->seed : 0ull; A.fast_call = fast ? fast->call : 0ull;
    A.fast_n_eps = (int)b->current_size; A.fast_future_p = fast ? fast->future_p : 0.0;
    A.obs = b->d_obs; A.ag = b->d_ag; A.g = b->d_g; A.act = b->d_act;
    A.plan = d_plan;
    A.onz = on->d; A.gnz = gn->d;
    A.batch = batch;
    A.T = b->T; A.od = b->obs_dim; A.gd = b->goal_dim; A.ad = b->act_dim;
    A.sq_threshold = sq_threshold;
    A.clip_obs = clip_obs;
    A.clip_o = on->clip; A.clip_g = gn->clip;
    A.x = o->x; A.xn = o->x_next; A.a = o->actions; A.r = o->r;
    A.o_e = reinterpret_cast<long long *>(o->e); A.o_t = reinterpret_cast<long long *>(o->t);
    A.o_fut = reinterpret_cast<long long *>(o->future_t);
    A.o_her = o->her;
    const int ug = (b->goal_dim + 1) / 2, ua = (b->act_dim + 1) / 2;
    if (!f32_rows && b->obs_dim + ug + ua <= 32 && b->goal_dim >= 2 && b->act_dim >= 2) {
        HP_KLOG("k_gather_fused2");
        launch_gather2<Fused2>(b, batch, fast != nullptr, A);
    } else if (!f32_rows) {
        HP_REQUIRE(!fast, HP_ERR_INVALID, "hp_buffer_sample_dev_fast: needs obs_dim + ceil(goal_dim / 2) + ceil(act_dim / 2) <= 32 and goal_dim, act_dim >= 2");
        const int flight = gather_flight(batch, 4);
        HP_KLOG("k_gather_fused");
        if (flight == 4) hipLaunchKernelGGL(k_gather_fused<4>, gather_grid(b, batch, flight), dim3(256), 0, b->ctx->stream, A);
        else hipLaunchKernelGGL(k_gather_fused<1>, gather_grid(b, batch, flight), dim3(256), 0, b->ctx->stream, A);
    } else {
        HP_KLOG("k_gather_packed");
        launch_gather2<Packed>(b, batch, fast != nullptr, P);
    }
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

// what every device-output entry asks of its arguments.  fast: the fast draw, which has no stream (rng is null) and never
// reaches k_gather_fused, the kernel that needs goal_dim <= 64
static int sample_dev_check(hp_buffer *b, hp_rng *rng, hp_norm *on, hp_norm *gn, int64_t batch, double clip_obs,
                            const hp_sample_dev_out *o, const char *who, bool fast = false) {
    HP_REQUIRE(b && (rng || fast) && on && gn && o, HP_ERR_INVALID, "%s: null argument", who);
    HP_REQUIRE(on->ctx == b->ctx && gn->ctx == b->ctx && (!rng || rng->ctx == b->ctx), HP_ERR_INVALID, "%s: handles of different contexts", who);
    HP_REQUIRE(on->size == b->obs_dim && gn->size == b->goal_dim, HP_ERR_INVALID,
               "%s: normalizer sizes (%d, %d) do not match the buffer's observation / goal widths (%d, %d)", who, on->size, gn->size,
               b->obs_dim, b->goal_dim);
    HP_REQUIRE(batch > 0, HP_ERR_INVALID, "%s: batch must be positive", who);
    HP_REQUIRE(clip_obs > 0, HP_ERR_INVALID, "%s: clip_obs must be positive (arguments.py:87; pass a huge value for none)", who);
    HP_REQUIRE(fast || b->goal_dim <= 64, HP_ERR_INVALID, "%s: goal_dim > 64", who);
    return HP_OK;
}

// The sampling scratch.  Growing `plan` / `out` frees memory that earlier asynchronous launches may still read: wait for them
// explicitly instead of relying on hipFree's implicit device synchronisation.  (The dict-layout entries, hp_buffer_sample and
// hp_buffer_sample_device_us, grow both with a plain ensure, as they always have: they rely on that synchronisation of hipFree.)
static int scratch_grow(hp_buffer *b, DevBuf &d, size_t need) {
    if (need > d.bytes) HP_CHECK_HIP(hipStreamSynchronize(b->ctx->stream));
    return d.ensure(need);
}
static int plan_for(hp_buffer *b, int64_t batch, PlanRec **d_plan) {
    HP_TRY(scratch_grow(b, b->plan, batch * sizeof(PlanRec)));
    *d_plan = b->plan.as<PlanRec>();
    return HP_OK;
}
// device outputs in `out` for the timing entries: x | x_next | actions | r, nothing else asked for
static int scratch_out_for(hp_buffer *b, int64_t batch, hp_sample_dev_out *o) {
    const size_t ldx = (size_t)(b->obs_dim + b->goal_dim);
    HP_TRY(scratch_grow(b, b->out, (size_t)batch * (2 * ldx + b->act_dim + 1) * 4));
    memset(o, 0, sizeof(*o));
    o->x = b->out.as<float>();
    o->x_next = o->x + batch * ldx;
    o->actions = o->x_next + batch * ldx;
    o->r = o->actions + batch * b->act_dim;
    return HP_OK;
}

// The timing entries' bracket: device microseconds per launch of up to two stages, `reps` launches of the first back to back, then
// of the second, between HIP events on the stream.  create() comes before the entry's warm launches, stage() after them;
// launch(i) enqueues repetition i.
struct Events {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    int n = 0;                                      // stages run
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }   // destroyed on every exit path
    int create(int stages) {
        for (int i = 0; i <= stages; ++i) HP_CHECK_HIP(hipEventCreate(&e[i]));
        return HP_OK;
    }
    template <class Launch> int stage(hipStream_t s, int32_t reps, Launch launch) {
        if (n == 0) HP_CHECK_HIP(hipEventRecord(e[0], s));
        for (int i = 0; i < reps; ++i) HP_TRY(launch(i));
        HP_CHECK_HIP(hipEventRecord(e[++n], s));
        return HP_OK;
    }
    int finish(int32_t reps, double *us0, double *us1 = nullptr) {
        double *const us[2] = {us0, us1};
        HP_CHECK_HIP(hipEventSynchronize(e[n]));
        for (int k = 0; k < n; ++k) {
            float ms = 0.f;
            HP_CHECK_HIP(hipEventElapsedTime(&ms, e[k], e[k + 1]));
            *us[k] = 1e3 * ms / reps;
        }
        return HP_OK;
    }
};

// --------------------------------------------------------------------------------- C ABI
extern "C" {

// diagnostic: device time of the standalone sampler kernels (no host copies): one index draw, then `reps` launches each of
// the index-draw kernel and of the gather / relabel / reward kernel on that plan, bracketed by HIP events.  The stream
// position advances by 1 + reps draws.
int hp_buffer_sample_device_us(hp_buffer *b, hp_rng *rng, int64_t batch, double future_p, double sq_threshold,
                               int32_t reps, double *draw_us, double *gather_us) {
    HP_REQUIRE(b && rng && draw_us && gather_us && batch > 0 && reps > 0, HP_ERR_INVALID, "hp_buffer_sample_device_us: bad argument");
    HP_SERIALISE(b);
    HP_REQUIRE(b->current_size > 0, HP_ERR_EMPTY, "high <= 0");
    const size_t row = (size_t)(2 * b->obs_dim + 3 * b->goal_dim + b->act_dim);
    HP_TRY(b->plan.ensure(batch * sizeof(PlanRec)));
    HP_TRY(b->out.ensure(batch * row * 8 + batch * 4));
    PlanRec *d_plan = b->plan.as<PlanRec>();
    double *d_out = b->out.as<double>();
    float *d_r = reinterpret_cast<float *>(d_out + batch * row);
    auto draw = [&](int) { return rng_launch_plan(rng, b->d_meta, 0, b->T, batch, 1, future_p, d_plan); };
    auto gather = [&](int) { return buffer_launch_gather_dict(b, d_plan, batch, sq_threshold, d_out, d_r, nullptr); };
    Events ev;
    HP_TRY(ev.create(2));
    HP_TRY(draw(0));
    HP_TRY(gather(0));   // warm
    HP_TRY(ev.stage(b->ctx->stream, reps, draw));
    HP_TRY(ev.stage(b->ctx->stream, reps, gather));
    return ev.finish(reps, draw_us, gather_us);
}

int hp_buffer_sample(hp_buffer *b, hp_rng *rng, int64_t batch, double future_p, double sq_threshold,
                     const hp_sample_out *o) {
    HP_REQUIRE(b && rng && o, HP_ERR_INVALID, "hp_buffer_sample: null argument");
    HP_SERIALISE(b);
    HP_REQUIRE(batch > 0, HP_ERR_INVALID, "hp_buffer_sample: batch must be positive");
    HP_REQUIRE(b->current_size > 0, HP_ERR_EMPTY, "high <= 0");  // np.random.randint(0, 0, B), her.py:24
    hipStream_t s = b->ctx->stream;
    const int od = b->obs_dim, gd = b->goal_dim, ad = b->act_dim;
    const size_t row = (size_t)(2 * od + 3 * gd + ad);
    HP_TRY(b->plan.ensure(batch * sizeof(PlanRec)));
    HP_TRY(b->out.ensure(batch * row * 8 + batch * 8 + batch * 4));
    PlanRec *d_plan = b->plan.as<PlanRec>();
    double *d_out = b->out.as<double>();
    double *d_r64 = d_out + batch * row;
    float *d_r = reinterpret_cast<float *>(d_r64 + batch);
    HP_TRY(rng_launch_plan_sample(rng, b->d_meta, b->T, batch, future_p, d_plan));
    HP_TRY(buffer_launch_gather_dict(b, d_plan, batch, sq_threshold, d_out, d_r, o->r64 ? d_r64 : nullptr));
    double *p = d_out;
    auto pull = [&](double *dst, size_t n) -> hipError_t {
        hipError_t e = dst ? hipMemcpyAsync(dst, p, n * 8, hipMemcpyDeviceToHost, s) : hipSuccess;
        p += n;
        return e;
    };
    HP_CHECK_HIP(pull(o->obs, batch * od));
    HP_CHECK_HIP(pull(o->ag, batch * gd));
    HP_CHECK_HIP(pull(o->g, batch * gd));
    HP_CHECK_HIP(pull(o->actions, batch * ad));
    HP_CHECK_HIP(pull(o->obs_next, batch * od));
    HP_CHECK_HIP(pull(o->ag_next, batch * gd));
    if (o->r) HP_CHECK_HIP(hipMemcpyAsync(o->r, d_r, batch * 4, hipMemcpyDeviceToHost, s));
    if (o->r64) HP_CHECK_HIP(hipMemcpyAsync(o->r64, d_r64, batch * 8, hipMemcpyDeviceToHost, s));
    std::vector<PlanRec> hplan;
    if (o->e || o->t || o->future_t || o->her) {
        hplan.resize(batch);
        HP_CHECK_HIP(hipMemcpyAsync(hplan.data(), d_plan, batch * sizeof(PlanRec), hipMemcpyDeviceToHost, s));
    }
    HP_CHECK_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < hplan.size(); ++i) {
        if (o->e) o->e[i] = hplan[i].e;
        if (o->t) o->t[i] = hplan[i].t;
        if (o->future_t) o->future_t[i] = hplan[i].fut;
        if (o->her) o->her[i] = (uint8_t)hplan[i].her;
    }
    return HP_OK;
}

// hp_buffer_sample_dev, and (f32_rows) hp_buffer_sample_dev_f32: the same draws from the same stream, the same indices, relabelled
// goals, rewards and goal columns bit for bit out of the throughput rows (buffer.hip: hp_buffer_enable_f32_rows); the
// observation columns are those of float32-rounded observations (storage_dtype = fp32)
static int sample_dev(hp_buffer *b, bool f32_rows, hp_rng *rng, hp_norm *on, hp_norm *gn, int64_t batch, double future_p,
                      double sq_threshold, double clip_obs, const hp_sample_dev_out *o, const char *who) {
    HP_TRY(sample_dev_check(b, rng, on, gn, batch, clip_obs, o, who));
    HP_SERIALISE(b);
    HP_REQUIRE(!f32_rows || b->p_row, HP_ERR_STATE, "%s: hp_buffer_enable_f32_rows first", who);
    HP_REQUIRE(b->current_size > 0, HP_ERR_EMPTY, "high <= 0");  // np.random.randint(0, 0, B), her.py:24
    PlanRec *d_plan = nullptr;
    HP_TRY(plan_for(b, batch, &d_plan));
    HP_TRY(rng_launch_plan_sample(rng, b->d_meta, b->T, batch, future_p, d_plan));
    return launch_gather(b, f32_rows, d_plan, on, gn, batch, sq_threshold, clip_obs, o);
}
int hp_buffer_sample_dev(hp_buffer *b, hp_rng *rng, hp_norm *on, hp_norm *gn, int64_t batch, double future_p,
                         double sq_threshold, double clip_obs, const hp_sample_dev_out *o) {
    return sample_dev(b, false, rng, on, gn, batch, future_p, sq_threshold, clip_obs, o, "hp_buffer_sample_dev");
}
int hp_buffer_sample_dev_f32(hp_buffer *b, hp_rng *rng, hp_norm *on, hp_norm *gn, int64_t batch, double future_p,
                             double sq_threshold, double clip_obs, const hp_sample_dev_out *o) {
    return sample_dev(b, true, rng, on, gn, batch, future_p, sq_threshold, clip_obs, o, "hp_buffer_sample_dev_f32");
}

// Fast draw (SURVEY 8b rng_mode = Philox; opt-in, NOT the reference's random stream): hp_buffer_sample_dev / _f32 with the index
// draw inside the gather kernel, keyed by (seed, call, transition) -- no hp_rng, no sequential draw kernel, one launch.  The caller
// owns the counter: the same (seed, call) gives the same minibatch; a training loop passes seed + rank and call = 0, 1, 2, ...
int hp_buffer_sample_dev_fast(hp_buffer *b, hp_norm *on, hp_norm *gn, int64_t batch, double future_p, double sq_threshold,
                              double clip_obs, uint64_t seed, uint64_t call, int32_t f32_rows, const hp_sample_dev_out *o) {
    HP_TRY(sample_dev_check(b, nullptr, on, gn, batch, clip_obs, o, "hp_buffer_sample_dev_fast", true));
    HP_SERIALISE(b);
    HP_REQUIRE(!f32_rows || b->p_row, HP_ERR_STATE, "hp_buffer_sample_dev_fast: hp_buffer_enable_f32_rows first");
    HP_REQUIRE(b->current_size > 0, HP_ERR_EMPTY, "high <= 0");
    const FastDraw fd{seed, call, future_p};
    return launch_gather(b, f32_rows != 0, nullptr, on, gn, batch, sq_threshold, clip_obs, o, &fd);
}

// diagnostic: device microseconds per hp_buffer_sample_dev_fast launch (outputs into library scratch), `reps` back to back
int hp_buffer_sample_dev_fast_us(hp_buffer *b, hp_norm *on, hp_norm *gn, int64_t batch, double future_p, double sq_threshold,
                                 double clip_obs, int32_t reps, int32_t f32_rows, double *us) {
    HP_REQUIRE(b && on && gn && us && batch > 0 && reps > 0, HP_ERR_INVALID, "hp_buffer_sample_dev_fast_us: bad argument");
    HP_SERIALISE(b);
    hp_sample_dev_out o;
    HP_TRY(scratch_out_for(b, batch, &o));
    auto sample = [&](uint64_t call) { return hp_buffer_sample_dev_fast(b, on, gn, batch, future_p, sq_threshold, clip_obs, 1, call, f32_rows, &o); };
    Events ev;
    HP_TRY(ev.create(1));
    HP_TRY(sample(0));   // warm
    HP_TRY(ev.stage(b->ctx->stream, reps, [&](int i) { return sample(1 + i); }));
    return ev.finish(reps, us);
}

// diagnostic twin of hp_buffer_sample_device_us for the fused kernel (outputs into library scratch); f32_rows != 0: the
// throughput-rows kernel (hp_buffer_sample_dev_f32)
int hp_buffer_sample_dev_us(hp_buffer *b, hp_rng *rng, hp_norm *on, hp_norm *gn, int64_t batch, double future_p,
                            double sq_threshold, double clip_obs, int32_t reps, int32_t f32_rows, double *draw_us,
                            double *gather_us) {
    hp_sample_dev_out o;
    memset(&o, 0, sizeof(o));
    HP_TRY(sample_dev_check(b, rng, on, gn, batch, clip_obs, &o, "hp_buffer_sample_dev_us"));
    HP_REQUIRE(draw_us && gather_us && reps > 0, HP_ERR_INVALID, "hp_buffer_sample_dev_us: bad argument");
    HP_SERIALISE(b);
    HP_REQUIRE(b->current_size > 0, HP_ERR_EMPTY, "high <= 0");
    HP_REQUIRE(!f32_rows || b->p_row, HP_ERR_STATE, "hp_buffer_sample_dev_us: hp_buffer_enable_f32_rows first");
    PlanRec *d_plan = nullptr;
    HP_TRY(plan_for(b, batch, &d_plan));
    HP_TRY(scratch_out_for(b, batch, &o));
    auto draw = [&](int) { return rng_launch_plan_sample(rng, b->d_meta, b->T, batch, future_p, d_plan); };
    auto gather = [&](int) { return launch_gather(b, f32_rows != 0, d_plan, on, gn, batch, sq_threshold, clip_obs, &o); };
    Events ev;
    HP_TRY(ev.create(2));
    HP_TRY(draw(0));
    HP_TRY(gather(0));   // warm
    HP_TRY(ev.stage(b->ctx->stream, reps, draw));
    HP_TRY(ev.stage(b->ctx->stream, reps, gather));
    return ev.finish(reps, draw_us, gather_us);
}

}  // extern "C"
