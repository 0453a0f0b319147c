// agent_engines.hip -- the update's device code and its launch logic on gfx950: row-slab chain kernels (slab8.h: 4/8/16-row
// slabs on v_mfma_f32_4x4x1, slab32.h: 32-row slabs on v_mfma_f32_32x32x2), weight-gradient launches (gemm_lds.h 32 x 32
// tiles, dw64.h split 64 x 64 tiles) with the optimizer in their epilogue and the sampler's look-ahead riding along,
// the peer-exchange optimizer kernels and polyak.  (The rollout-side forward -- policy / critic rows -- is agent_forward.hip; of it
// this unit compiles the kernels: the policy slab's, beside the chain kernels whose device functions it is made of, with its
// launcher, and the four pack kernels of forward_kernels.h.)
// Reference: models.py:11-44, ddpg_agent.py:214-277, torch.optim.Adam (ddpg_agent.py:42-43).
//
// ---- why it is shaped like this (measured) -------------------------------------
// One update at batch 256 is 0.7 GFLOP over ~16 strictly dependent layers: microseconds of FP32-MFMA time, so the cost
// is the number of dependent launches and the per-CU weight stream, not math.  Every product is fp32 MFMA (no TF32 on
// gfx950; the 1e-5 loss parity needs fp32); all state is device resident and every kernel argument is constant across
// updates, so a whole training cycle is one cached hipGraph (agent.hip).
#ifdef SLAB_TIMELINE
#define ADAM_TL 1
#endif
#include "agent_device.h"
#include "gemm_lds.h"
#include "transition_device.h"

// One row per kernel: the name the launch log records (hp_agent_update_kernels) beside the kernel launched under it.  Each launch
// family of the host side has ONE place that maps its run-time choice to a row, and launch_row reads both from it: the log cannot
// name another kernel than the one enqueued.
template <class... A> struct KernRow { const char *name; void (*fn)(A...); };
template <class... A> static KernRow<A...> row(const char *name, void (*fn)(A...)) { return {name, fn}; }
template <class... A, class... B>
static int launch_row(const KernRow<A...> &k, unsigned grid, unsigned threads, hipStream_t s, const B &...args) {
    HP_KLOG(k.name);
    hipLaunchKernelGGL(k.fn, dim3(grid), dim3(threads), 0, s, args...);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

// gradients: barrier + rank-ordered sum + Adam.  n4 = arena floats / 4; u = index of the update in its sequence.
__global__ __launch_bounds__(256) void k_peer_adam(const PeerDev D, const AdamFuse F, int n4, int u, int mean) {
    const unsigned long long epoch = D.epoch[0] + (unsigned long long)u + 1ull;
    const int par = (int)(epoch & 1ull);
    if (blockIdx.x == 0) peer_signal(D, D.flags_g, epoch);
    if (!peer_wait(D, D.flags_g[D.rank], epoch)) return;   // dead exchange: no step from a partial sum (peer.h)
    if (blockIdx.x == 0 && threadIdx.x < 64) loss_finalize(F);
    split_reset_by_block0(F);
    const int t0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (t0 >= n4) return;
    bool quad;
    const int idx0 = adam_quad_remap(F.am, t0, quad), t = idx0 >> 2;   // which float4 of the arena this thread steps (agent_device.h)
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const size_t bytes = (size_t)n4 * 16;
    for (int q = 0; q < D.world; ++q) {   // rank order: the same float32 sum on every rank
        const float4 v = peer_load4(D.grad[q][par], bytes, (unsigned)t * 16u, q == D.rank);
        if (q == 0) acc = v;
        else { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
    }
    if (mean) {   // SUM / world, float32 true division (what the RCCL path's k_scale_div does)
        const float w = (float)D.world;
        acc.x /= w; acc.y /= w; acc.z /= w; acc.w /= w;
    }
    const float g[4] = {acc.x, acc.y, acc.z, acc.w};
    if (F.keep_grads) *reinterpret_cast<float4 *>(const_cast<float *>(F.grads_base) + 4 * (size_t)t) = acc;
    if (quad) adam_step4_quad(F, idx0, g);
    else adam_apply4(F, idx0, g);
}


// two-phase exchange, phase 2 (phase 1 = k_peer_reduce_slice in peer.hip): every element's sum comes from the rank that
// owns its slice; Adam on all of them.  Same values as k_peer_adam computes itself: bit-identical.
__global__ __launch_bounds__(256) void k_peer_adam2(const PeerDev D, const AdamFuse F, int n4, int u) {
    const unsigned long long epoch = D.epoch[0] + (unsigned long long)u + 1ull;
    const int par = (int)(epoch & 1ull);
    if (blockIdx.x == 0) peer_signal(D, D.flags_r, epoch);
    if (!peer_wait(D, D.flags_r[D.rank], epoch, 3u)) return;
    if (blockIdx.x == 0 && threadIdx.x < 64) loss_finalize(F);
    split_reset_by_block0(F);
    const int t0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (t0 >= n4) return;
    bool quad;
    const int idx0 = adam_quad_remap(F.am, t0, quad), t = idx0 >> 2;
    const int owner = t / peer_slice_len(D, n4);
    const float4 acc = peer_load4(D.red[owner][par], (size_t)n4 * 16, (unsigned)t * 16u, owner == D.rank);
    const float g[4] = {acc.x, acc.y, acc.z, acc.w};
    if (F.keep_grads) *reinterpret_cast<float4 *>(const_cast<float *>(F.grads_base) + 4 * (size_t)t) = acc;
    if (quad) adam_step4_quad(F, idx0, g);
    else adam_apply4(F, idx0, g);
}

static int peer_enqueue_adam(hp_peer *p, const AdamFuse &F, int n_arena, int u, bool mean) {
    const int n4 = n_arena / 4;
    if (p->phases == 2) {
        HP_TRY(peer_enqueue_reduce_slice(p, n4, u, mean));
        HP_TRY(peer_enqueue_gate(p, 3, u));
        return launch_row(row("k_peer_adam2", k_peer_adam2), (n4 + 255) / 256, 256, p->ctx->stream, p->dev, F, n4, u);
    }
    HP_TRY(peer_enqueue_gate(p, 1, u));
    return launch_row(row("k_peer_adam", k_peer_adam), (n4 + 255) / 256, 256, p->ctx->stream, p->dev, F, n4, u, mean ? 1 : 0);
}

// the 4x4x1 slab engine, compiled for two slab heights (see slab8.h)
#define S8_NRG 1
#define S8_NS s8r4
#include "slab8.h"
#undef S8_NRG
#undef S8_NS
#define S8_NRG 2
#define S8_NS s8r8
#include "slab8.h"
#undef S8_NRG
#undef S8_NS
#define S8_NRG 4
#define S8_NS s8r16
#include "slab8.h"
#undef S8_NRG
#undef S8_NS
#undef S8_ROWS
#undef S8_RING
#undef S8_RPW
#include "slab32.h"

// Weight-gradient tiles (+ optimizer) with the sampler's look-ahead riding along.  When the chain kernel occupies every
// CU (batch 1024: 256 chain workgroups) it has no room for its spare workgroups -- a workgroup appended to a full launch
// starts when the first chain ends and then runs alone (k_fb_slab8 51.5 instead of 37.8 us) -- so the index plan of
// update u + 2 and the gather of update u + 1's inputs move into THIS launch, whose 296 tile workgroups leave half of the
// CUs' slots free: blocks [tiles, tiles + n_plan) draw, the next n_ahead gather.  Same device functions as the chain
// kernel's spare workgroups, same order of draws in the stream: identical bits.
struct RideArgs {
    int n_plan, n_ahead;
    MtState *rng;
    const BufMeta *meta;
    PlanRec *next_plan;
    double future_p;
    int T, plan_batch;
    GatherSrc ahead;
    float *aXT, *aXA, *aXP;
    int ldx, act_off, act_dim;
    float max_action;
};

template <bool ADAM, bool UNI = false, bool PEER = false>
__device__ __forceinline__ void gemm_ride_body(const GemmGroup &grp, const AdamFuse *F, const RideArgs &R, int tiles,
                                               const PeerTile *PT = nullptr, const TileHead *TH = nullptr) {
    __shared__ __attribute__((aligned(16))) float lds[GL_LDS_FLOATS];
    __shared__ float bsum[GL_WAVES][32];
    if (ADAM && !PEER && grp.loss_wg && blockIdx.x == gridDim.x - 1) {   // behind the riders: the loss log's own workgroup (gemm_lds.h)
        gemm_loss_wg(*F);
        return;
    }
    if (grp.bias0 > 0 && (int)blockIdx.x >= grp.bias0 && (int)blockIdx.x < tiles) {   // (`tiles` counts the bias panels behind the tiles)
        gemm_bias_tile<ADAM>(grp, F, (int)blockIdx.x - grp.bias0, lds, bsum);
        return;
    }
    if ((int)blockIdx.x < tiles) {
        gemm_tile<ADAM, UNI, false, PEER>(grp, F, (int)blockIdx.x, lds, bsum, blockIdx.x == 0 && (PEER || !grp.loss_wg), PT, TH);
        return;
    }
    const int extra = (int)blockIdx.x - tiles;
#ifdef SLAB_TIMELINE   // riders stamp start / end like the tiles (slot 7: 1 = index plan, 2 = gather)
    if (threadIdx.x == 0 && blockIdx.x < 512) { g_gemm_tl_wg[blockIdx.x][0] = wall_clock64(); g_gemm_tl_wg[blockIdx.x][7] = extra < R.n_plan ? 1 : 2; }
#endif
    if (extra < R.n_plan) {
        if (threadIdx.x >= MT_THREADS) return;   // ended waves take no part in the barriers of the draw
        // the sequential draw is the longest single job of this launch at batch 1024 (as long as the tiles): let its waves
        // issue ahead of the tile workgroup that shares the CU
        __builtin_amdgcn_s_setprio(3);
        mt_her_plan(R.rng, R.meta->current_size, R.T, R.plan_batch, 1, R.future_p, R.next_plan,
                    reinterpret_cast<uint32_t(*)[MT_N]>(lds), reinterpret_cast<int *>(&bsum[0][0]));
    } else {
        s8r4::s8_gather_ahead(R.ahead, R.aXT, R.aXA, R.aXP, R.ldx, R.act_off, R.act_dim, R.max_action, extra - R.n_plan,
                              R.n_ahead);
    }
#ifdef SLAB_TIMELINE
    if (threadIdx.x == 0 && blockIdx.x < 512) g_gemm_tl_wg[blockIdx.x][5] = wall_clock64();
#endif
}
__global__ __launch_bounds__(GL_THREADS) void k_gemm_lds_ride(const GemmGroup grp, const RideArgs R, int tiles) {
    gemm_ride_body<false>(grp, nullptr, R, tiles);
}
__global__ __launch_bounds__(GL_THREADS) void k_gemm_lds_adam_ride(unsigned long long t03, unsigned long long t47, int tiles,
                                                                   const GemmGroup grp, const AdamFuse F, const RideArgs R) {
    const TileHead TH{t03, t47};   // (leading scalars: preloaded with the wave, gemm_lds.h)
    const unsigned sink = kernarg_prefetch<24 + sizeof(GemmGroup) + sizeof(AdamFuse) + sizeof(RideArgs)>();
    gemm_ride_body<true>(grp, &F, R, tiles, nullptr, &TH);
    kernarg_prefetch_keep(sink);
}

__global__ __launch_bounds__(GL_THREADS) void k_gemm_lds_ride_u(const GemmGroup grp, const RideArgs R, int tiles) {
    gemm_ride_body<false, true>(grp, nullptr, R, tiles);
}
__global__ __launch_bounds__(GL_THREADS) void k_gemm_lds_adam_ride_u(unsigned long long t03, unsigned long long t47, int tiles,
                                                                     const GemmGroup grp, const AdamFuse F, const RideArgs R) {
    const TileHead TH{t03, t47};
    const unsigned sink = kernarg_prefetch<24 + sizeof(GemmGroup) + sizeof(AdamFuse) + sizeof(RideArgs)>();
    gemm_ride_body<true, true>(grp, &F, R, tiles, nullptr, &TH);
    kernarg_prefetch_keep(sink);
}

// data-parallel ranks, tile-wise one-shot exchange (gemm_lds.h PEER): weight gradients + rank exchange + optimizer step in ONE
// launch, the riders behind the tiles as above.  Replaces k_gemm_lds -> k_peer_adam (its kernel boundary, its second pass over
// the gradients: +6 us per update at world size 1), and lets early tiles exchange while later ones still multiply.
// row0: first flag row of this launch's tiles (0; the actor's tile launch behind a split launch: the critic's tile count)
// t03 / t47: the tile -> problem table as leading scalars (preloaded with the wave, gemm_lds.h TileHead), as in k_gemm_lds_adam
__global__ __launch_bounds__(GL_THREADS) void k_gemm_lds_adam_peer(unsigned long long t03, unsigned long long t47, const GemmGroup grp,
                                                                   const AdamFuse F, const RideArgs R, int tiles, const PeerDev D, int u,
                                                                   int mean, int row0) {
    const TileHead TH{t03, t47};
    const PeerTile PT{&D, u, mean, row0};
    gemm_ride_body<true, false, true>(grp, &F, R, tiles, &PT, &TH);
}
__global__ __launch_bounds__(GL_THREADS) void k_gemm_lds_adam_peer_u(unsigned long long t03, unsigned long long t47, const GemmGroup grp,
                                                                     const AdamFuse F, const RideArgs R, int tiles, const PeerDev D, int u,
                                                                     int mean, int row0) {
    const TileHead TH{t03, t47};
    const PeerTile PT{&D, u, mean, row0};
    gemm_ride_body<true, true, true>(grp, &F, R, tiles, &PT, &TH);
}

// Large minibatches: 64 x 64 tiles with the batch rows split over workgroups (dw64.h), same riders behind the tiles
#include "dw64.h"
template <bool ADAM>
__device__ __forceinline__ void dw64_ride_body(const GemmGroup &grp, const AdamFuse *F, const RideArgs &R, const Dw64Args &X) {
    __shared__ __attribute__((aligned(16))) float lds[DW_LDS_FLOATS];
    __shared__ int aux[256];
    if ((int)blockIdx.x < X.n_wg) {
        dw64_tile<ADAM>(grp, F, X, (int)blockIdx.x, lds, aux);
        return;
    }
    const int extra = (int)blockIdx.x - X.n_wg;
    if (extra < R.n_plan) {
        if (threadIdx.x >= MT_THREADS) return;
        __builtin_amdgcn_s_setprio(3);
        mt_her_plan(R.rng, R.meta->current_size, R.T, R.plan_batch, 1, R.future_p, R.next_plan,
                    reinterpret_cast<uint32_t(*)[MT_N]>(lds), aux);
    } else {
        s8r4::s8_gather_ahead(R.ahead, R.aXT, R.aXA, R.aXP, R.ldx, R.act_off, R.act_dim, R.max_action, extra - R.n_plan,
                              R.n_ahead);
    }
}
__global__ __launch_bounds__(DW_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_dw64(const GemmGroup grp, const RideArgs R, const Dw64Args X) {
    dw64_ride_body<false>(grp, nullptr, R, X);
}
__global__ __launch_bounds__(DW_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_dw64_adam(const GemmGroup grp, const AdamFuse F, const RideArgs R, const Dw64Args X) {
    dw64_ride_body<true>(grp, &F, R, X);
}


// canonical arena -> fragment-ordered copies of the slab engines (hp_agent_set_params, sync_targets)
__global__ void k_relayout(const float *__restrict__ canon, float *fragF, float *fragD, int n, const ArenaMap am) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    int of, od;
    frag_offsets_any(am, idx, of, od);
    const float v = canon[idx];
    if (of >= 0) fragF[of] = v;
    if (od >= 0 && fragD) fragD[od] = v;
}

__global__ __launch_bounds__(256) void k_gather_fused(const double *__restrict__ obs, const double *__restrict__ ag,
                                                      const double *__restrict__ g, const double *__restrict__ act,
                                                      const PlanRec *__restrict__ plan, int batch, int T, int obs_dim,
                                                      int goal_dim, int act_dim, double sq_threshold,
                                                      const NormDev *__restrict__ onz, const NormDev *__restrict__ gnz,
                                                      double clip_obs, double clip_range, float max_action, int ldx,
                                                      int act_off, float *XA, float *XP, float *XT, float *R) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= batch) return;
    const PlanRec rec = plan[i];
    const long long e = rec.e;
    const int t = rec.t;
    const double *obs_row = obs + (e * (T + 1) + t) * obs_dim;
    const double *ag_next = ag + (e * (T + 1) + t + 1) * goal_dim;
    const double *g_src = TR_GOAL_SRC(rec, ag, g, T, goal_dim);
    const double *act_row = act + (e * T + t) * act_dim;
    float *xa = XA + (long long)i * ldx, *xp = XP + (long long)i * ldx, *xt = XT + (long long)i * ldx;
    for (int c = lane; c < 2 * obs_dim; c += 64) {
        const int col = (c < obs_dim) ? c : c - obs_dim;
        const float x = tr_net_input(obs_row[c], clip_obs, onz->mean[col], onz->std[col], clip_range);
        if (c < obs_dim) {
            xa[col] = x;
            xp[col] = x;
        } else {
            xt[col] = x;
        }
    }
    for (int c = lane; c < goal_dim; c += 64) {
        const float x = tr_net_input(g_src[c], clip_obs, gnz->mean[c], gnz->std[c], clip_range);
        xa[obs_dim + c] = x;
        xp[obs_dim + c] = x;
        xt[obs_dim + c] = x;   // g_next := g (ddpg_agent.py:231)
    }
    for (int c = lane; c < act_dim; c += 64) xa[act_off + c] = (float)act_row[c] / max_action;  // models.py:38
    if (lane == 0) R[i] = hp_reward(tr_sq_distance(ag_next, g_src, goal_dim), sq_threshold);
}

// slab engine: Adam that also refreshes the fragment-ordered copies and finishes the loss log
__global__ __launch_bounds__(256) void k_adam_frag(const AdamFuse F, const float *__restrict__ g, int n) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 64) loss_finalize(F);
    split_reset_by_block0(F);
    if (idx >= n) return;
    adam_apply(F, idx, g[idx]);
}

// 4 consecutive arena elements per thread (n % 4 == 0)
__global__ __launch_bounds__(256) void k_adam_frag4(const AdamFuse F, const float *__restrict__ g, int n4) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 64) loss_finalize(F);
    split_reset_by_block0(F);
    if (t >= n4) return;
    bool quad;
    const int idx0 = adam_quad_remap(F.am, t, quad);   // the 256-wide layers dealt in 4-row x 64-column blocks (agent_device.h)
    const float4 g4 = *reinterpret_cast<const float4 *>(g + idx0);
    const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
    if (quad) adam_step4_quad(F, idx0, gv);
    else adam_apply4(F, idx0, gv);
}

__global__ void k_polyak_frag(float *__restrict__ tgt, const float *__restrict__ src, float *fragFT, int n,
                              float one_minus, float polyak, const ArenaMap am) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const float t = __fadd_rn(__fmul_rn(one_minus, src[idx]), __fmul_rn(polyak, tgt[idx]));
    tgt[idx] = t;
    int of, od;
    frag_offsets_any(am, idx, of, od);
    if (of >= 0) fragFT[of] = t;
}

// the layer-per-launch forward chain's pack kernels (launched by agent_forward.hip), compiled where they always were
#define FORWARD_KERNELS_HERE
#include "forward_kernels.h"

// ------------------------------------------------------------------------------- host side
int launch_group(hp_agent *a, const Launch &L, int which) {
    ProfScope ps(a, which);
    return launch_row(L.g.uni ? row("k_gemm_lds_u", k_gemm_lds_u) : row("k_gemm_lds", k_gemm_lds), L.tiles, GL_THREADS, a->ctx->stream, L.g);
}

// k_policy_slab8 and its grid rule, a workgroup per 4 rows: the one launch site of the policy calls (agent_forward.hip)
int launch_policy_slab(hipStream_t stream, const PolicyArgs &P) {
    static_assert(sizeof(s8r4::PolicyLds) <= 160 * 1024, "the policy slab's LDS fits a CU");
    hipLaunchKernelGGL(s8r4::k_policy_slab8, dim3((unsigned)((P.rows + 3) / 4)), dim3(S8_THREADS), 0, stream, P);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

int enqueue_gather(hp_agent *a, hp_buffer *b, hp_norm *on, hp_norm *gn, const PlanRec *plan, double sq, int xset,
                   hipStream_t stream) {
    ProfScope ps(a, PROF_SAMPLE);
    return launch_row(row("k_gather_fused", k_gather_fused), (a->B + 3) / 4, 256, stream ? stream : a->ctx->stream, b->d_obs, b->d_ag,
                      b->d_g, b->d_act, plan, a->B, (int)b->T, (int)b->obs_dim, (int)b->goal_dim, (int)b->act_dim, sq, on->d,
                      gn->d, a->cfg.clip_obs, a->cfg.clip_range, (float)a->cfg.max_action, a->ldx, a->act_off,
                      xset ? a->XA2 : a->XA, xset ? a->XP2 : a->XP, xset ? a->XT2 : a->XT, xset ? a->R2 : a->R);
}

static ArenaMap arena_map(const hp_agent *a) {
    ArenaMap am;
    am.la = a->la;
    am.lc = a->lc;
    am.H = a->H;
    am.mode = a->slab32 ? 2 : a->slab ? 1 : 0;
    return am;
}

static AdamFuse adam_fuse(hp_agent *a) {
    AdamFuse F;
    F.p = a->params; F.p_out = a->params; F.m = a->adam_m; F.v = a->adam_v; F.fragF = a->fragF; F.fragD = a->fragD;
    F.grads_base = a->grads; F.st = a->d_state; F.scal = &a->d_state->neg_step_actor; F.am = arena_map(a); F.n_actor = a->la.total;
    F.keep_grads = 1;
    F.tgt = nullptr; F.fragFT = nullptr; F.polyak = 0.f; F.one_minus = 0.f;
    F.gate = nullptr; F.gate_need = 0u; F.gate_sel = 0u; F.fault = nullptr; F.fault_host = nullptr; F.gate_ticks = 0ull; F.reset_sync = nullptr; F.tl_mark = 0;
    F.w = (float)(1.0 - a->cfg.adam_beta1); F.b2 = (float)a->cfg.adam_beta2;
    F.omb2 = (float)(1.0 - a->cfg.adam_beta2); F.eps = (float)a->cfg.adam_eps;
    F.part = a->part; F.nslab = a->Mp / (a->slab8 ? a->s8_rows : S32_ROWS); F.B = a->B;
    F.act_dim = a->cfg.act_dim;
    F.action_l2 = (float)a->cfg.action_l2; F.loss_log = a->loss_log;
    F.wt = a->Mp <= 768 ? 1 : 0;   // us/update without / with: 40.9 / 40.3 at 256, 44.9 / 44.4 at 384, 46.9 / 46.1 at 512 k8, 53.1 / 52.9 at 768, 55.6 / 55.8 at 1024
    return F;
}

#define SPLIT_WAIT_TICKS 50000000ull   // bounded in-launch waits: 0.5 s of the 100 MHz wall clock, three orders of magnitude beyond a launch

// What an optimizer block needs to know about its launch beyond the update it steps (adam_block)
struct OptGates {
    enum { IN_TILES, ADAM_KERNEL, PEER_KERNEL } where = IN_TILES;   // the weight-gradient tiles' epilogue, k_adam_frag*, k_peer_adam*
    const unsigned *gate = nullptr;   // k_fb_split8's tiles: the counter set their steps wait on (gate_need chains, gate_sel per problem)
    unsigned need = 0, sel = 0;
    int tl_mark = 0;                  // time-line builds: this launch records its gate stamps
    unsigned *reset_sync = nullptr;   // the launch behind a split launch: clears the counter set that launch counted in
};

// The optimizer argument block of one launch.  gc: the sampled update it steps (nullptr: staged minibatch, lone step, prologue).
static AdamFuse adam_block(hp_agent *a, const GatherCtx *gc, const OptGates &g = {}) {
    AdamFuse F = adam_fuse(a);
    // inside a sampled update loop nobody reads the gradient vector (hp_agent_get_grads documents this): the launches that compute or
    // exchange it leave it out of memory (1.17 MB of the ~6.7 MB the tile launch leaves dirty in L2) unless RLARM_KEEP_GRADS=1, when
    // hp_agent_get_grads returns the exchanged sum.  k_adam_frag* reads it from memory.
    F.keep_grads = (!gc || a->keep_grads_dbg || g.where == OptGates::ADAM_KERNEL) ? 1 : 0;
    if (gc && gc->polyak_after) {   // the optimizer launch also steps the targets
        F.tgt = a->targets; F.fragFT = a->fragFT;
        F.polyak = (float)a->cfg.polyak; F.one_minus = (float)(1.0 - a->cfg.polyak);
    }
    if (g.gate) {
        F.gate = g.gate; F.gate_need = g.need; F.gate_sel = g.sel;
        F.fault = a->k1_sync + SPLIT_FAULT; F.fault_host = a->fault_host_dev; F.gate_ticks = SPLIT_WAIT_TICKS;
        F.tl_mark = g.tl_mark;
    }
    F.reset_sync = g.reset_sync;
    // plain stores in the stand-alone optimizer kernels: write-through (adam_fuse: small minibatches) pays inside a tile launch,
    // where other workgroups still multiply while the stepped state drains; a kernel that does nothing else only waits for its
    // own acknowledgements (forced data-parallel world 1, us/update: RCCL form 44.7 -> 43.5, separate peer exchange 45.3 -> 44.9)
    if (g.where != OptGates::IN_TILES) F.wt = 0;
    return F;
}

int enqueue_relayout(hp_agent *a, bool targets) {
    const int n = a->n_arena;
    hipLaunchKernelGGL(k_relayout, dim3((n + 255) / 256), dim3(256), 0, a->ctx->stream,
                       targets ? a->targets : a->params, targets ? a->fragFT : a->fragF,
                       targets ? (float *)nullptr : a->fragD, n, arena_map(a));
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

// ---- the eight weight-gradient problems of one update: the only products that reduce over the batch.  Each is stated once
// (add_dw_prob); a launch is a list of them.
enum { DW_ACTOR = 0, DW_CRITIC = 1 };
struct DwProb { int net, layer; };   // layer 1-4 of the actor / the critic
// dW = dY^T X, db = column sums of dY of one layer.  sX: the input set its network read (X operand of layer 1); grads: base of the
// gradient arena [actor | critic]
static void add_dw_prob(const hp_agent *a, Launch &L, DwProb q, const float *sX, float *grads) {
    const bool c = q.net == DW_CRITIC;
    const NetLayout &l = c ? a->lc : a->la;
    const int H = a->H;
    const struct { const float *dY, *X; int w, b; } of[4] = {
        {c ? a->dA1 : a->dK1, sX, l.w1, l.b1},
        {c ? a->dA2 : a->dK2, c ? a->CA.h1 : a->AP.h1, l.w2, l.b2},
        {c ? a->dA3 : a->dK3, c ? a->CA.h2 : a->AP.h2, l.w3, l.b3},
        {c ? a->dQA : a->dZ, c ? a->CA.h3 : a->AP.h3, l.w4, l.b4}};
    const auto &p = of[q.layer - 1];
    const int ny = q.layer == 4 ? 16 : H;   // outputs = dY's row stride: the heads are [Mp][16]
    float *G = grads + (c ? a->la.total : 0);
    add_dw(L, p.dY, ny, ny, p.X, q.layer == 1 ? a->ldx : H, q.layer == 1 ? l.K1 : H, G + p.w, G + p.b, a->Mp, q.layer);
}

// all of them as one launch (input sets sXA / sXP)
Launch build_dw_group(const hp_agent *a, const float *sXA, const float *sXP, float *grads) {
    const int Mp = a->Mp;
    if (!grads) grads = a->grads;
    // the four 256 x 256 problems first: Launch::place_on_xcds gives each of them one pair of XCDs.
    // The narrow problems (heads, first layers: 40 tiles at the reference shapes) follow as second workgroups on CUs that
    // already hold a 256 x 256 tile; with a long reduction their batch rows are split over ks workgroups each, so that no CU
    // carries two full tiles (gemm_lds.h)
    static const DwProb joint[8] = {{DW_CRITIC, 3}, {DW_CRITIC, 2}, {DW_ACTOR, 3}, {DW_ACTOR, 2},
                                    {DW_CRITIC, 4}, {DW_CRITIC, 1}, {DW_ACTOR, 4}, {DW_ACTOR, 1}};
    const int ks = (!a->dw64 && a->gl_part && a->dw_ksplit > 1 && Mp >= GL_RING_MIN_K) ? a->dw_ksplit : 1;   // ring path only
    Launch L;
    for (int i = 0; i < 8; ++i) {
        add_dw_prob(a, L, joint[i], joint[i].net == DW_CRITIC ? sXA : sXP, grads);
        if (i >= 4 && ks > 1) L.split_last(ks);
    }
    L.g.part = a->gl_part;
    L.g.ticket = a->gl_ticket;
    L.g.uni = (Mp > 256 && Mp <= 640) ? 1 : 0;   // gemm_lds.h, note at `wave`
    L.place_on_xcds();
    return L;
}

// tile table + exchange buffers of the large-minibatch weight-gradient launch (dw64.h)
static int dw64_args(hp_agent *a, const Launch &L, Dw64Args &X) {
    memset(&X, 0, sizeof(X));
    X.S = a->dw_S;
    int K = 0, tiles = 0;
    for (int i = 0; i < L.g.n; ++i) {
        const GemmProb &p = L.g.p[i];
        HP_REQUIRE(p.a_si == 1 && p.b_sj == 1 && p.M % 8 == 0 && p.N % 8 == 0 && p.K % DW_KH == 0, HP_ERR_INVALID,
                   "dw64: operand layout");
        X.tile0[i] = tiles;
        X.tiles_n[i] = (p.N + 63) / 64;
        tiles += ((p.M + 63) / 64) * X.tiles_n[i];
        K = p.K > K ? p.K : K;
    }
    X.kslice = ((K + X.S - 1) / X.S + DW_KH - 1) / DW_KH * DW_KH;
    X.n_wg = X.S * tiles;
    // allocated by hp_agent_create (this runs under stream capture)
    HP_REQUIRE(a->dw_part.bytes >= (size_t)tiles * X.S * DW_PART * sizeof(float) && a->dw_ticket.bytes >= sizeof(unsigned long long) * (size_t)tiles,
               HP_ERR_INVALID, "dw64: exchange buffers too small");
    X.part = a->dw_part.as<float>();
    X.ticket = a->dw_ticket.as<unsigned long long>();
    return HP_OK;
}

// ---- split launch (slab8_split.h) ------------------------------------------------------------------------------------------
static int split_warmers(const hp_agent *a) {   // L2 warmers per XCD that still fit beside three kinds of chains + the spare workgroups
    const int per_xcd = a->ctx->cu_count / 8;
    const int nslab = a->Mp / a->s8_rows;
    const int chains = 3 * ((nslab + 7) / 8) + 1;   // worst XCD: its share of every kind of chain + a plan / gather workgroup
    return per_xcd - chains >= 2 ? 2 : (per_xcd - chains >= 1 ? 1 : 0);
}
// three kinds of chains of `rows`-row slabs + a plan / gather workgroup per XCD on this device's CUs?
bool split_fits_rows(const hp_agent *a, int rows) {
    if (a->ctx->cu_count % 8 != 0 || rows != 4) return false;   // (the kernel is compiled for 4-row slabs only)
    const int per_xcd = a->ctx->cu_count / 8, nslab = a->Mp / rows;
    return 3 * ((nslab + 7) / 8) + 1 <= per_xcd;
}
// Data-parallel ranks take the split launch too (round 6): with the tile-wise peer exchange the critic's in-launch tiles exchange
// and step by themselves (SPLIT_TILES_PEER), with any other transport -- RCCL, the two-phase or gated peer forms, a caller that
// exchanges itself -- they leave the gradients to the exchange + optimizer launches that follow (SPLIT_TILES_GRADS).
// Not when ranks SHARE a device (rehearsals on a 1-GPU box; hp_peer_set_gate is how the library is told): the in-launch waits of
// one rank's tiles for its own chains assume that the launch is resident as a whole, and eight ranks' launches on one device are
// not (measured: the bounded hand-off of an 8-rank rehearsal gave up, fault word 0x11) -- those keep the two-launch form.
bool split_fits(const hp_agent *a) {
    if (!a->slab8 || a->dw64 || !a->fuse_adam_ok) return false;
    if (a->peer && a->peer->gate) return false;
    if (a->Mp < GL_RING_MIN_K || a->dw_ksplit > 1) return false;   // the in-launch tiles take the ring path, unsplit
    return split_fits_rows(a, a->s8_rows);
}

// Who runs where.  Workgroup b of the launch lands on XCD b % 8, and within an XCD in index order: chains first, then the spare
// workgroups, the weight-gradient tiles last (they wait for chains).  The actor-side chains run ALONE on XCDs 0-3 -- the launch's
// critical path keeps an L2 to itself, 16 streams per XCD like in k_fb_slab8 -- and every short chain on XCDs 4-7, whose 32
// streams per XCD saturate their L2s (the short chains end 1.5 us later: they have 10 us of slack): 38.3 us/update at batch 256
// against 39.8 with every kind of chain spread evenly over the XCDs and 39.2 with the critic chains on both halves (round 4,
// profiles/r04_ab_split_place_b256.txt; those placements are gone).  Shapes whose chains do not divide that way are spread evenly.
static unsigned build_split_roles(const hp_agent *a, FbSplitArgs &Q, bool chains_ac, bool chains_t, int n_plan, int n_ahead,
                                  int n_tiles) {
    const int nslab = a->Mp / a->s8_rows, per_xcd = a->ctx->cu_count / 8;
    int n[8][SR_N];
    memset(n, 0, sizeof(n));
    auto spread = [&](int role, int count, int x0, int nx) {   // evenly over XCDs x0 .. x0 + nx - 1, remainder to the first ones
        for (int i = 0; i < nx; ++i) n[x0 + i][role] += count / nx + (i < count % nx ? 1 : 0);
    };
    const bool half = nslab % 8 == 0 && chains_ac && 3 * (nslab / 8) + 2 <= per_xcd && 2 * (nslab / 4) <= per_xcd;
    if (half) {   // the actor-side chains alone on XCDs 0-3 (as in k_fb_slab8), every short chain on XCDs 4-7
        spread(SR_A, nslab, 0, 4);
        spread(SR_C, nslab, 4, 4);
        if (chains_t) spread(SR_T, nslab, 4, 4);
    } else {
        if (chains_ac) { spread(SR_A, nslab, 0, 8); spread(SR_C, nslab, 0, 8); }
        if (chains_t) spread(SR_T, nslab, 0, 8);
    }
    for (int i = 0; i < n_plan; ++i) n[i % (half ? 4 : 8)][SR_PLAN] += 1;
    for (int i = 0; i < n_ahead; ++i) n[(n_plan + i) % (half ? 4 : 8)][SR_AHEAD] += 1;
    const int warm = split_warmers(a);
    Q.warm_side = 0u;
    for (int x = 0; x < 8; ++x) {
        int used = 0;
        for (int r = 0; r < SR_WARM; ++r) used += n[x][r];
        const int w = (per_xcd - used) < warm ? (per_xcd - used > 0 ? per_xcd - used : 0) : warm;
        n[x][SR_WARM] = (!chains_ac && !chains_t) ? 0 : w;
        // what this XCD's chains stream: 1 = the actor side's sets, 0 = the critic side's (targets + critic), 2 = all
        const unsigned side = half ? (x < 4 ? 1u : 0u) : (chains_ac ? 2u : 0u);
        Q.warm_side |= side << (4 * x);
    }
    // tiles: dealt to the XCDs in proportion to the CUs their short chains (C, T) and idle CUs leave them; the kernel numbers
    // them slot-major across the XCDs (slab8_split.h)
    if (n_tiles > 0) {
        int room[8], total = 0;
        for (int x = 0; x < 8; ++x) {
            room[x] = per_xcd - n[x][SR_A] - n[x][SR_PLAN] - n[x][SR_AHEAD] - n[x][SR_WARM];
            if (room[x] < 0) room[x] = 0;
            total += room[x];
        }
        int given = 0;
        for (int x = 0; x < 8; ++x) {
            n[x][SR_TILE] = total ? n_tiles * room[x] / total : 0;
            given += n[x][SR_TILE];
        }
        while (given < n_tiles) {   // the remainder: one at a time to the XCD with the most room left (never to one without, while any has)
            int best = 0;
            for (int x = 1; x < 8; ++x)
                if (room[x] - n[x][SR_TILE] > room[best] - n[best][SR_TILE]) best = x;
            n[best][SR_TILE] += 1;
            ++given;
        }
    }
    unsigned rows = 0;
    for (int x = 0; x < 8; ++x) {
        unsigned long long packed = 0ull;
        unsigned tot = 0;
        for (int r = 0; r < SR_N; ++r) {
            packed |= (unsigned long long)(n[x][r] & 0xff) << (8 * r);
            tot += (unsigned)n[x][r];
        }
        Q.nrole[x] = packed;
        rows = tot > rows ? tot : rows;
    }
    return 8u * rows;   // grid: workgroup b = 8 * slot + XCD; slots past an XCD's list exit at once
}

// the weight-gradient problems of one network (critic: inside the split launch; actor: the launch behind it)
// The critic's list is the order in which the critic chains publish the operands: W3, W4 (stage 0), W2 (stage 1), W1 (stage 2).
// The two tables behind it follow THAT order, 4 bits per problem, and change with it: SPLIT_TILE_STAGE, the counter that says a
// problem's operands are published (FbSplitArgs::tile_stage), and SPLIT_TILE_GATE, the counter its optimizer step waits on -- W3c
// after the actor-side chains' first critic dX layer (counter 4), W4c / W1c after their critic forward (3), W2c after the second
// dX layer (5).
static const DwProb DW_CRITIC_ORDER[4] = {{DW_CRITIC, 3}, {DW_CRITIC, 4}, {DW_CRITIC, 2}, {DW_CRITIC, 1}};
static const unsigned SPLIT_TILE_STAGE = 0u | (0u << 4) | (1u << 8) | (2u << 12);
static const unsigned SPLIT_TILE_GATE = 4u | (3u << 4) | (5u << 8) | (3u << 12);
// The actor's: its two 256 x 256 problems first, four XCDs each (gemm_tile: placed2)
static const DwProb DW_ACTOR_ORDER[4] = {{DW_ACTOR, 3}, {DW_ACTOR, 2}, {DW_ACTOR, 4}, {DW_ACTOR, 1}};
static Launch build_dw_half(const hp_agent *a, bool critic, const float *sX, float *grads) {
    const int Mp = a->Mp;
    Launch L;
    for (int i = 0; i < 4; ++i) add_dw_prob(a, L, (critic ? DW_CRITIC_ORDER : DW_ACTOR_ORDER)[i], sX, grads ? grads : a->grads);
    if (!critic && L.g.p[0].tiles_n == 8 && L.g.p[0].M == 256 && L.g.p[1].tile0 == 64 && L.g.p[1].tiles_n == 8 && L.g.p[1].M == 256)
        L.g.xcd = 2;
    L.g.uni = (Mp > 256 && Mp <= 640) ? 1 : 0;
    return L;
}

// ---- the riders of one update: the draw of a LATER update's index plan and the look-ahead gather of update u + 1's inputs (plan
// gc->ahead_plan) into the input set this update does not read.  Decided here, once per update: whether each runs, where -- in
// spare workgroups of the chain launch (split launch included) or behind the tiles of the weight-gradient launch (seq->ride ==
// RIDE_DW) --, with how many workgroups, and on what.  Both argument blocks are filled from the result (riders_into_chain,
// riders_into_tiles).
struct Riders {
    enum Where { NOWHERE, CHAIN, TILES };
    Where plan = NOWHERE, gather = NOWHERE;
    int gather_wgs = 0;
    int n_plan(Where w) const { return plan == w ? 1 : 0; }   // workgroups of each job in the launch `w`
    int n_ahead(Where w) const { return gather == w ? gather_wgs : 0; }
    // the draw (mt_her_plan)
    MtState *rng = nullptr;
    const BufMeta *meta = nullptr;
    PlanRec *next_plan = nullptr;
    double future_p = 0.0;
    int T = 0;
    // the gather (s8_gather_ahead): the next update's plan, reward vector and input sets
    const PlanRec *ahead_plan = nullptr;
    float *R = nullptr, *XT = nullptr, *XA = nullptr, *XP = nullptr;
};
static Riders riders_of(const hp_agent *a, const GatherCtx *gc) {
    Riders r;
    if (!gc) return r;   // staged minibatch: nothing to draw or gather
    const Riders::Where at = gc->seq->ride == SeqPlan::RIDE_DW ? Riders::TILES : Riders::CHAIN;
    if (gc->next_plan && gc->rng) {
        r.plan = at;
        r.rng = gc->rng->d_state; r.meta = gc->b->d_meta; r.next_plan = gc->next_plan; r.future_p = gc->future_p; r.T = gc->b->T;
    }
    if (gc->ahead_plan) {
        r.gather = at;
        // behind the tiles: one pass of 32 rows (8 waves x 4 rows in flight) per gather workgroup: each pass is two dependent HBM
        // latencies, so fewer, longer workgroups made that launch 3 us longer than its tiles (61.0 vs 58.6 us/update at
        // batch 1024 with 8 vs 32 of them)
        r.gather_wgs = at == Riders::CHAIN ? S8_AHEAD_WGS : std::min((a->B + 31) / 32, 64);
        const bool xs = gc->xset != 0;
        r.ahead_plan = gc->ahead_plan;
        r.R = xs ? a->R : a->R2; r.XT = xs ? a->XT : a->XT2; r.XA = xs ? a->XA : a->XA2; r.XP = xs ? a->XP : a->XP2;
    }
    return r;
}
// the gather's source and destinations, as both argument blocks hold them (gs: this update's own source)
static void aim_ahead(const Riders &r, const GatherSrc &gs, GatherSrc &ahead, float *&aXT, float *&aXA, float *&aXP) {
    ahead = gs;
    ahead.plan = r.ahead_plan;
    ahead.plan_any = r.ahead_plan;
    ahead.R = r.R;
    aXT = r.XT; aXA = r.XA; aXP = r.XP;
}
// spare workgroups of the chain launch (P.f.gs is set)
static void riders_into_chain(const hp_agent *a, const Riders &r, FbSlabArgs &P) {
    const bool draw = r.plan == Riders::CHAIN;
    P.b.rng = draw ? r.rng : nullptr;
    P.b.meta = draw ? r.meta : nullptr;
    P.b.next_plan = draw ? r.next_plan : nullptr;
    P.b.future_p = draw ? r.future_p : 0.0;
    P.b.T = draw ? r.T : 0;
    P.b.plan_batch = a->B;
    P.n_plan = r.n_plan(Riders::CHAIN);
    P.n_ahead = r.n_ahead(Riders::CHAIN);
    P.ahead = P.f.gs;
    P.aXT = P.aXA = P.aXP = nullptr;
    if (P.n_ahead) aim_ahead(r, P.f.gs, P.ahead, P.aXT, P.aXA, P.aXP);   // next update's inputs into the other set
}
// workgroups behind the tiles of the weight-gradient launch (all zero: no riders there)
static void riders_into_tiles(const hp_agent *a, const Riders &r, const GatherSrc &gs, RideArgs &R) {
    memset(&R, 0, sizeof(R));
    R.n_plan = r.n_plan(Riders::TILES);
    R.n_ahead = r.n_ahead(Riders::TILES);
    if (R.n_plan) {
        R.rng = r.rng; R.meta = r.meta; R.next_plan = r.next_plan; R.future_p = r.future_p;
        R.T = r.T; R.plan_batch = a->B;
    }
    if (R.n_ahead) {
        aim_ahead(r, gs, R.ahead, R.aXT, R.aXA, R.aXP);
        R.ldx = a->ldx; R.act_off = a->act_off; R.act_dim = a->cfg.act_dim; R.max_action = (float)a->cfg.max_action;
    }
}

// argument blocks of the chain kernels for one update (gc as in enqueue_forward_backward_slab), with the riders the chain launch
// carries
struct FbBuilt {
    FbSlabArgs P;
    int nslab;
    float *sXA, *sXP;
};
static void build_fb_args(hp_agent *a, const GatherCtx *gc, const Riders &riders, FbBuilt &O) {
    const int Mp = a->Mp;
    const int nslab = Mp / (a->slab8 ? a->s8_rows : S32_ROWS);
    FbSlabArgs &P = O.P;
    const int xs = gc ? gc->xset : 0;
    float *sXA = xs ? a->XA2 : a->XA, *sXP = xs ? a->XP2 : a->XP, *sXT = xs ? a->XT2 : a->XT, *sR = xs ? a->R2 : a->R;
    // what the forward and the backward half both take: the online nets, layouts, dims, activations, Q vectors
    auto shared = [&](auto &A) {
        A.online = SlabNetPtrs{a->fragF, a->fragD, a->params};
        A.la = a->la; A.lc = a->lc; A.H = a->H; A.ldx = a->ldx; A.act_off = a->act_off; A.act_dim = a->cfg.act_dim; A.Mp = Mp;
        A.max_action = (float)a->cfg.max_action;
        A.XP = sXP; A.TP = a->TP;
        A.CAh1 = a->CA.h1; A.CAh2 = a->CA.h2; A.CAh3 = a->CA.h3;
        A.APh1 = a->AP.h1; A.APh2 = a->AP.h2; A.APh3 = a->AP.h3;
        A.CPh1 = a->CP.h1; A.CPh2 = a->CP.h2; A.CPh3 = a->CP.h3;
        A.QT = a->QT; A.QA = a->QA; A.QP = a->QP;
    };
    {
        FwdSlabArgs &A = P.f;
        shared(A);
        A.tl = a->timeline;
        memset(&A.gs, 0, sizeof(A.gs));
        A.gs.plan_any = a->plan.as<PlanRec>();
        A.gs.B = a->B;
        if (gc) {
            hp_buffer *b = gc->b;
            A.gs.obs = b->d_obs; A.gs.ag = b->d_ag; A.gs.g = b->d_g; A.gs.act = b->d_act;
            A.gs.plan = gc->pregathered ? nullptr : gc->plan; A.gs.plan_any = gc->plan;
            A.gs.onz = gc->on->d; A.gs.gnz = gc->gn->d;
            A.gs.sq_threshold = gc->sq; A.gs.clip_obs = a->cfg.clip_obs; A.gs.clip_range = a->cfg.clip_range;
            A.gs.T = b->T; A.gs.obs_dim = b->obs_dim; A.gs.goal_dim = b->goal_dim; A.gs.B = a->B;
            A.gs.R = sR;
        }
        A.target = SlabNetPtrs{a->fragFT, nullptr, a->targets};
        A.XA = sXA; A.XT = sXT;
    }
    {
        BwdSlabArgs &A = P.b;
        shared(A);
        A.tl = a->timeline + 96;
        A.B = a->B;
        A.gamma = (float)a->cfg.gamma;
        A.clip_ret = (float)(1.0 / (1.0 - a->cfg.gamma)); A.action_l2 = (float)a->cfg.action_l2;
        A.R = sR;
        A.dQA = a->dQA; A.dA3 = a->dA3; A.dA2 = a->dA2; A.dA1 = a->dA1;
        A.dZ = a->dZ; A.dK3 = a->dK3; A.dK2 = a->dK2; A.dK1 = a->dK1;
        A.part = a->part; A.st = a->d_state; A.adam = adam_cfg(a);
        A.nslab = nslab;
    }
    riders_into_chain(a, riders, P);
    P.xcd_split = P.n_pref = 0;
    O.nslab = nslab; O.sXA = sXA; O.sXP = sXP;
}

// bias gradients + their optimizer step in workgroups of their own behind the tiles (gemm_lds.h: gemm_bias_tile; the ring path's
// summation order only; inside the tn == 0 tiles otherwise, and in the launches that exchange tile-wise between ranks: same bits)
static bool sep_bias_on(const hp_agent *a) { return a->Mp >= GL_RING_MIN_K && !a->dw64; }

// One weight-gradient launch: 32 x 32 tiles (gemm_lds.h) or 64 x 64 tiles with split batch rows (dw64.h), the optimizer step in
// their epilogue (F) or not, the plan draw / look-ahead gather (R) behind the tiles; peer_u >= 0: the tiles exchange between ranks
// by themselves (gemm_lds.h PEER) from flag row row0 on
static int launch_dw(hp_agent *a, Launch &L, const AdamFuse *F, const RideArgs &R, int peer_u = -1, int row0 = 0) {
    const int riders = R.n_plan + R.n_ahead;
    if (!a->dw64 && !F && !riders) return launch_group(a, L, PROF_DW);
    ProfScope ps(a, PROF_DW);
    hipStream_t s = a->ctx->stream;
    const bool uni = L.g.uni != 0;
    if (a->dw64) {
        // large minibatch: 64 x 64 tiles, batch rows split over workgroups (dw64.h); the riders follow the tiles
        Dw64Args X;
        HP_TRY(dw64_args(a, L, X));
        const unsigned grid = X.n_wg + riders;
        if (F) return launch_row(row("k_dw64_adam", k_dw64_adam), grid, DW_THREADS, s, L.g, *F, R, X);
        return launch_row(row("k_dw64", k_dw64), grid, DW_THREADS, s, L.g, R, X);
    }
    if (peer_u >= 0) {
        // data-parallel ranks: the tiles exchange by themselves; riders, if any, behind them
        HP_REQUIRE(F && a->peer && row0 + L.tiles <= HP_PEER_TILES, HP_ERR_STATE, "tile-wise exchange: %d tiles exceed the flag rows",
                   row0 + L.tiles);
        return launch_row(uni ? row("k_gemm_lds_adam_peer_u", k_gemm_lds_adam_peer_u) : row("k_gemm_lds_adam_peer", k_gemm_lds_adam_peer),
                          L.tiles + riders, GL_THREADS, s, L.head(0), L.head(1), L.g, *F, R, L.tiles, a->peer->dev, peer_u,
                          a->grad_mean ? 1 : 0, row0);
    }
    // tiles, then the bias panels, then the riders; with the optimizer, the loss log's own workgroup last
    const int front = L.tiles + (sep_bias_on(a) ? L.separate_bias() : 0);
    if (F) L.g.loss_wg = a->loss_wg;
    const unsigned grid = front + riders + L.g.loss_wg;
    if (F && riders)
        return launch_row(uni ? row("k_gemm_lds_adam_ride_u", k_gemm_lds_adam_ride_u) : row("k_gemm_lds_adam_ride", k_gemm_lds_adam_ride),
                          grid, GL_THREADS, s, L.head(0), L.head(1), front, L.g, *F, R);
    if (riders)
        return launch_row(uni ? row("k_gemm_lds_ride_u", k_gemm_lds_ride_u) : row("k_gemm_lds_ride", k_gemm_lds_ride), grid, GL_THREADS, s,
                          L.g, R, front);
    return launch_row(uni ? row("k_gemm_lds_adam_u", k_gemm_lds_adam_u) : row("k_gemm_lds_adam", k_gemm_lds_adam), grid, GL_THREADS, s,
                      L.head(0), L.head(1), L.g, *F);
}

// The chain launch's kernel: slab height x store policy of the chains' outputs (slab8.h) -- write-through unless
// RLARM_ENGINE=chain_plain: ordinary stores measured no gain in this launch (batch 512 k8 and 1024); the log names
// both k_fb_slab8 -- or the 32-row engine's
static KernRow<FbSlabArgs> chain_kernel(const hp_agent *a) {
    if (!a->slab8) return row("k_fb_slab32", s32::k_fb_slab32);
    const bool wt = a->chain_wt != 0;
    return row("k_fb_slab8", a->s8_rows == 4   ? (wt ? s8r4::k_fb_slab8 : s8r4::k_fb_slab8_plain)
                             : a->s8_rows == 8 ? (wt ? s8r8::k_fb_slab8 : s8r8::k_fb_slab8_plain)
                                               : (wt ? s8r16::k_fb_slab8 : s8r16::k_fb_slab8_plain));
}

// The plan an update is launched by: a sampled update's is its sequence's (seq_plan, agent.hip).  A staged minibatch has no sequence
// and takes a default one -- no riders, no split launch, the optimizer in the tiles' epilogue (staged_step) or nowhere.
static const SeqPlan &plan_of(const GatherCtx *gc, bool staged_step) {
    static const SeqPlan none, step = [] { SeqPlan p; p.opt = SeqPlan::OPT_TILES; return p; }();
    return gc ? *gc->seq : staged_step ? step : none;
}

// slab engines: forwards + losses + backwards of one update (inputs in XA/XP/XT/R): chain kernel + weight-gradient launch
// only = 1 / 2: just the chain kernel / just the weight-gradient launch (timing diagnostics, hp_agent_debug_chain)
static int enqueue_split_update(hp_agent *a, const GatherCtx *gc, FbBuilt &built, int only);
int enqueue_forward_backward_slab(hp_agent *a, const GatherCtx *gc, int only, bool staged_step) {
    HP_REQUIRE(!gc || gc->seq, HP_ERR_INVALID, "a sampled update without its sequence's plan");
    const SeqPlan &seq = plan_of(gc, staged_step);
    hipStream_t s = a->ctx->stream;
    const Riders riders = riders_of(a, gc);
    FbBuilt built;
    build_fb_args(a, gc, riders, built);
    FbSlabArgs &P = built.P;
    const int nslab = built.nslab;
    if (seq.split) return enqueue_split_update(a, gc, built, only);
    if (only == 2) {
    } else if (a->slab8) {
        // one launch: each workgroup carries its rows through forward AND backward (k_fb_slab8)
        ProfScope ps(a, PROF_GEMM_FWD);
        // chains split across XCD halves: measured (us/update, split vs not) 42.0 vs 43.5 at batch 128, 44.0 vs 45.2 at 256,
        // 46.6 vs 46.6 at 384, 48.0 vs 47.8 at 448, 77.3 vs 74.6 at 1024 -- it pays while the chains leave half of the CUs free
        const int n_chain = chain_wgs(a);
        P.xcd_split = (nslab % 4 == 0) && 4 * nslab <= a->ctx->cu_count;
        // L2 warmers: spare workgroups (the same number on every XCD) while the launch still fits the CUs.  Measured (us/update, with
        // 8 vs without): 39.9 vs 42.4 at batch 128, 42.1 vs 44.4 at 256, 46.4 vs 46.6 at 384, 52.8 vs 54.2 at 512, 56.6 vs 57.1 at 768.
        // Two per XCD instead of one (round 3, after the entry reordering): 39.65 vs 39.82 at batch 256, 41.3 vs 43.0 at 384; 24 / 32: no
        // further gain (40.0 / 40.0 vs 39.95 with 16).
        const int fit = a->ctx->cu_count - (n_chain + P.n_plan + P.n_ahead);
        P.n_pref = fit >= 16 ? 16 : (fit >= 8 ? 8 : 0);
        HP_TRY(launch_row(chain_kernel(a), n_chain + P.n_plan + P.n_ahead + P.n_pref, S8_THREADS, s, P));
    } else {
        // 32-row slabs, forward + backward of a chain in one workgroup; inputs come gathered (enqueue_updates)
        ProfScope ps(a, PROF_GEMM_FWD);
        HP_TRY(launch_row(chain_kernel(a), 2 * nslab + P.n_plan, S32_THREADS, s, P));
    }
    if (only == 1) return HP_OK;
    // all weight gradients (+ the optimizer where the plan puts it in their epilogue) as their own launch
    Launch L = build_dw_group(a, built.sXA, built.sXP, gc ? gc->grads_out : nullptr);
    RideArgs R;
    riders_into_tiles(a, riders, P.f.gs, R);
    const AdamFuse F = adam_block(a, gc);
    const bool step = seq.opt == SeqPlan::OPT_TILES || seq.opt == SeqPlan::OPT_PEER_TILES;
    return launch_dw(a, L, step ? &F : nullptr, R, seq.opt == SeqPlan::OPT_PEER_TILES ? gc->u : -1);
}

// ---- one update in the split form: k_fb_split8 (chains + the critic's tiles and optimizer step), then the actor's tiles
// The split launch's kernel: the instantiation of a tiles mode x the store policy of the actor-side chains -- write-through
// (a_wt, RLARM_ENGINE=chain_wt: k_fb_split8_wt) instead of ordinary stores (slab8.h, "store policy"); the log names both k_fb_split8<n>
static auto split_kernel(int tiles_mode, bool a_wt) {
    using namespace s8r4;
    switch (tiles_mode) {
        case SPLIT_TILES_PEER: return row("k_fb_split8<1>", a_wt ? k_fb_split8_wt<SPLIT_TILES_PEER> : k_fb_split8<SPLIT_TILES_PEER>);
        case SPLIT_TILES_GRADS: return row("k_fb_split8<2>", a_wt ? k_fb_split8_wt<SPLIT_TILES_GRADS> : k_fb_split8<SPLIT_TILES_GRADS>);
        default: return row("k_fb_split8<0>", a_wt ? k_fb_split8_wt<SPLIT_TILES_ADAM> : k_fb_split8<SPLIT_TILES_ADAM>);
    }
}
// k_fb_split8 with its role table as leading scalar arguments: word r = role r, byte x = its workgroups on XCD x
static int launch_split(const hp_agent *a, unsigned grid, const FbSplitArgs &Q, int tiles_mode) {
    unsigned long long w[SR_N];
    for (int r = 0; r < SR_N; ++r) {
        w[r] = 0ull;
        for (int x = 0; x < 8; ++x) w[r] |= ((Q.nrole[x] >> (8 * r)) & 0xffull) << (8 * x);
    }
    return launch_row(split_kernel(tiles_mode, a->chain_wt == 1), grid, S8_THREADS, a->ctx->stream, w[0], w[1], w[2], w[3], w[4], w[5],
                      w[6], Q);
}

// The argument block of a split launch and its grid.  An update's launch (`tiles`: the critic's weight-gradient problems): every kind
// of chain, the riders of P, the critic's tiles behind their gates, counter set gc->qset, target chains on the NEXT update's plan
// (gc->t_plan; none: the sequence's last update).  The sequence's prologue (tiles == nullptr): target chains only, on the first
// update's OWN plan (gc->plan) into Q' set 0 -- no A / C chains, no tiles (need_c = 0), an optimizer block that steps nothing, set 1
// (sync_other = set 0, the first update's), reset_sync: it clears the counters.
static unsigned build_split_args(hp_agent *a, const GatherCtx *gc, const FbSlabArgs &P, const Launch *tiles, FbSplitArgs &Q) {
    const bool prologue = tiles == nullptr;
    const int set = prologue ? 1 : gc->qset;
    const PlanRec *t_plan = prologue ? gc->plan : gc->t_plan;
    static FbSplitArgs Qz;   // zero template (the struct has padding the kernel never reads)
    Q = Qz;
    Q.s = P;
    Q.tgs = P.f.gs;
    if (t_plan) {
        Q.tgs.plan = t_plan;
        Q.tgs.plan_any = t_plan;
    }
    Q.tgs.R = nullptr;
    Q.qt_in = set ? a->QT2 : a->QT;
    Q.qt_out = set ? a->QT : a->QT2;
    Q.sync = a->k1_sync + (set & 1) * SPLIT_SET_WORDS;
    Q.sync_other = a->k1_sync + ((set + 1) & 1) * SPLIT_SET_WORDS;
    Q.fault = a->k1_sync + SPLIT_FAULT;
    Q.fault_host = a->fault_host_dev;
    Q.wait_ticks = SPLIT_WAIT_TICKS;
    if (prologue) {
        Q.reset_sync = 1;
        Q.adam = adam_block(a, nullptr);
        return build_split_roles(a, Q, false, true, 0, 0, 0);
    }
    const unsigned nslab = (unsigned)P.b.nslab;
    Q.tile_stage = SPLIT_TILE_STAGE;
    Q.tiles = tiles->g;
    Q.need_c = nslab;
    // time-line builds: the last launch with target chains AND a plan workgroup stamps
    Q.tl_mark = (t_plan != nullptr && P.n_plan > 0) ? 1 : 0;
    Q.adam = adam_block(a, gc, {OptGates::IN_TILES, Q.sync, nslab, SPLIT_TILE_GATE, Q.tl_mark});
    if (gc->seq->tiles_mode == SPLIT_TILES_PEER) {
        Q.peer = a->peer->d_dev;
        Q.peer_u = gc->u;
        Q.peer_mean = a->grad_mean ? 1 : 0;
    }
    return build_split_roles(a, Q, true, t_plan != nullptr, P.n_plan, P.n_ahead, tiles->tiles);
}

static int enqueue_split_update(hp_agent *a, const GatherCtx *gc, FbBuilt &built, int only) {
    HP_REQUIRE(only == 0 && split_fits(a), HP_ERR_STATE, "split launch: not available for this engine / call");
    // what the in-launch tiles do behind their products (slab8_split_args.h): the optimizer step (single rank), the tile-wise rank
    // exchange + the step (data-parallel ranks on a device each, gemm_lds.h PEER), or nothing -- the caller exchanges the gradient
    // vector and steps in launches of its own (RCCL; two-phase / gated peer memory)
    const int mode = gc->seq->tiles_mode;
    // The critic's tiles ride in the split launch; the actor's are the launch behind it (the form that held them in the split launch
    // too, behind an "actor-side chains done" counter, measured 45.7 vs 38.0 us/update in round 4 and is gone).
    Launch L = build_dw_half(a, true, built.sXA, mode == SPLIT_TILES_GRADS ? gc->grads_out : nullptr);
    Launch La = build_dw_half(a, false, built.sXP, mode == SPLIT_TILES_GRADS ? gc->grads_out : nullptr);
    HP_REQUIRE(mode != SPLIT_TILES_PEER || (a->peer && a->peer->d_dev && L.tiles + La.tiles <= HP_PEER_TILES), HP_ERR_STATE,
               "tile-wise exchange in the split launch: %d + %d tiles exceed the flag rows", L.tiles, La.tiles);
    FbSplitArgs Q;
    const unsigned grid = build_split_args(a, gc, built.P, &L, Q);
    {
        ProfScope ps(a, PROF_GEMM_FWD);
        HP_TRY(launch_split(a, grid, Q, mode));
    }
    // the actor's weight gradients (+ optimizer step): 144 tiles at the reference shapes, one per CU.  The launch clears this
    // launch's counter set, so that every split launch starts from a clean set whatever the parity of the sequence before it
    // (gradients only: the optimizer launch behind the exchange does, enqueue_updates).  Tile-wise exchange: flag rows behind the
    // critic's; tile 0 writes the loss log and clears the set (the bias gradients stay inside the tn == 0 tiles, as in every
    // tile-wise launch).
    OptGates g;
    g.reset_sync = Q.sync;
    const AdamFuse Fa = adam_block(a, gc, g);
    RideArgs R;
    riders_into_tiles(a, Riders(), built.P.f.gs, R);   // (a split sequence's riders are the split launch's spare workgroups)
    return launch_dw(a, La, mode == SPLIT_TILES_GRADS ? nullptr : &Fa, R, mode == SPLIT_TILES_PEER ? gc->u : -1, L.tiles);
}

// target chains of the sequence's first update (its plan: gc->plan) -> Q' set 0; also clears the first update's counter set
int enqueue_split_prologue(hp_agent *a, const GatherCtx *gc) {
    HP_REQUIRE(gc && gc->seq && split_fits(a), HP_ERR_STATE, "split launch: not available for this engine");
    FbBuilt built;
    build_fb_args(a, gc, Riders(), built);   // (the sequence's first gc: its own inputs, no riders)
    FbSplitArgs Q;
    const unsigned grid = build_split_args(a, gc, built.P, nullptr, Q);
    ProfScope ps(a, PROF_PLAN);   // (once per sequence, with the index draws: not an update's launch)
    // (no tiles here: the instantiation the sequence's updates run, so that a rank executes ONE k_fb_split8)
    return launch_split(a, grid, Q, gc->seq->tiles_mode);
}

int enqueue_adam(hp_agent *a, const GatherCtx *gc, unsigned *reset_sync) {
    ProfScope ps(a, PROF_ADAM);
    if (!a->slab) return layers_enqueue_adam(a);
    OptGates g;
    g.where = OptGates::ADAM_KERNEL;
    g.reset_sync = reset_sync;
    const AdamFuse F = adam_block(a, gc, g);
    const int n = a->n_arena;
    if (n % 4 == 0 && a->la.total % 4 == 0)
        return launch_row(row("k_adam_frag4", k_adam_frag4), (n / 4 + 255) / 256, 256, a->ctx->stream, F, a->grads, n / 4);
    return launch_row(row("k_adam_frag", k_adam_frag), (n + 255) / 256, 256, a->ctx->stream, F, a->grads, n);
}

int enqueue_polyak(hp_agent *a) {
    ProfScope ps(a, PROF_ADAM);
    const int n = a->n_arena;
    const double om = 1.0 - a->cfg.polyak;
    if (a->slab)
        return launch_row(row("k_polyak_frag", k_polyak_frag), (n + 255) / 256, 256, a->ctx->stream, a->targets, a->params, a->fragFT, n,
                          (float)om, (float)a->cfg.polyak, arena_map(a));
    return layers_enqueue_polyak(a);
}

// one update's forwards + backwards.  A sampled update (gc) is launched by its sequence's plan, gc->seq, the optimizer's placement
// included.  gc == nullptr: the minibatch is already staged in XA/XP/XT/R and there is no sequence; staged_step: the optimizer step
// follows immediately on this rank: where tiles_step(a) says so the slab engines apply it in the weight-gradient GEMM's epilogue and
// the caller must NOT enqueue Adam again.
int enqueue_forward_backward(hp_agent *a, const GatherCtx *gc, bool staged_step) {
    // Adam in the weight-gradient GEMM's epilogue (k_gemm_lds_adam).  The first version (one element at a time: four
    // serialised cold round trips per thread for p/m/v) measured 92.9 vs 67.5 us per update and was parked; with four
    // elements per thread (one float4 load per state array, float4 store into the forward fragment copy) it is the
    // faster path, 57.2 vs 60.5 us, and the default.  RLARM_FUSE_ADAM=0 keeps the separate k_adam_frag4 launch for A/B.
    if (a->slab) return enqueue_forward_backward_slab(a, gc, 0, staged_step && tiles_step(a));   // gather fused into the forward kernel
    if (gc) HP_TRY(enqueue_gather(a, gc->b, gc->on, gc->gn, gc->plan, gc->sq));
    return enqueue_forward_backward_layers(a);
}

int enqueue_peer_adam(hp_agent *a, const GatherCtx *gc, unsigned *reset_sync) {
    OptGates g;
    g.where = OptGates::PEER_KERNEL;
    g.reset_sync = reset_sync;
    const AdamFuse F = adam_block(a, gc, g);
    ProfScope ps(a, PROF_ADAM);
    return peer_enqueue_adam(a->peer, F, a->n_arena, gc->u, a->grad_mean);
}

extern "C" {

// diagnostic: time `n` back-to-back launches of ONE stage of the update as a captured hipGraph.
//   kind 6: optimizer kernel   8: polyak   10: forward + backward of the active engine (inputs as staged)
//   11: chain kernel only   12: weight-gradient launch (+ optimizer) only
int hp_agent_debug_chain(hp_agent *a, int32_t kind, int32_t n, double *us_per_launch) {
    HP_REQUIRE(a && us_per_launch && n > 0, HP_ERR_INVALID, "hp_agent_debug_chain: bad argument");
    HP_SERIALISE(a);
    hipStream_t s = a->ctx->stream;
    auto one = [&]() -> int {
        switch (kind) {
            case 6: return enqueue_adam(a);
            case 8: return enqueue_polyak(a);
            case 10: return enqueue_forward_backward(a);   // whole forward+backward of the active engine
            case 11: return a->slab ? enqueue_forward_backward_slab(a, nullptr, 1, true) : (int)HP_ERR_STATE;  // chain kernel(s) only
            case 12: return a->slab ? enqueue_forward_backward_slab(a, nullptr, 2, true) : (int)HP_ERR_STATE;  // weight gradients + Adam only
            default: hp_set_error("hp_agent_debug_chain: unknown kind %d", kind); return HP_ERR_INVALID;
        }
    };
    HP_CHECK_HIP(hipStreamSynchronize(s));
    const Captured c = capture_graph(s, [&] {
        for (int i = 0; i < n; ++i) HP_TRY(one());
        return (int)HP_OK;
    });
    HP_TRY(c.status());
    HP_CHECK_HIP(hipGraphLaunch(c.exec.h, s));
    HP_CHECK_HIP(hipEventRecord(a->ev0, s));
    HP_CHECK_HIP(hipGraphLaunch(c.exec.h, s));
    HP_CHECK_HIP(hipEventRecord(a->ev1, s));
    HP_CHECK_HIP(hipEventSynchronize(a->ev1));
    float ms = 0.f;
    HP_CHECK_HIP(hipEventElapsedTime(&ms, a->ev0, a->ev1));
    *us_per_launch = 1e3 * ms / n;
    return HP_OK;
}

// diagnostic: stage-boundary time stamps (100 MHz ticks) written by a -DSLAB_TIMELINE build of the slab
// kernels: out[chain * 32 + k] for the forward kernel, out[96 + chain * 32 + k] for the backward kernel
int hp_agent_debug_timeline(hp_agent *a, uint64_t *out192) {
    HP_REQUIRE(a && out192, HP_ERR_INVALID, "hp_agent_debug_timeline: bad argument");
    HP_SERIALISE(a);
    HP_CHECK_HIP(hipMemcpyAsync(out192, a->timeline, 192 * 8, hipMemcpyDeviceToHost, a->ctx->stream));
    HP_CHECK_HIP(hipStreamSynchronize(a->ctx->stream));
#ifdef SLAB_TIMELINE   // weight-gradient GEMM stamps: first workgroup at [160..175], last at [176..191]
    HP_CHECK_HIP(hipMemcpyFromSymbol(out192 + 160, HIP_SYMBOL(g_gemm_tl), 32 * 8));
#endif
    return HP_OK;
}

#ifdef SLAB_TIMELINE
// time-line builds only (not part of the ABI): stage stamps of every workgroup of the last 32 x 32-tile launch
int hp_debug_gemm_wg_timeline(uint64_t *out4096) {
    HP_CHECK_HIP(hipDeviceSynchronize());
    HP_CHECK_HIP(hipMemcpyFromSymbol(out4096, HIP_SYMBOL(g_gemm_tl_wg), 512 * 8 * 8));
    return HP_OK;
}
// every workgroup of the last k_fb_split8 launch: out[5 * b + 0..3] = {start, hand-off point, gate reached (tiles), end}, [4] = role
int hp_debug_split_timeline(uint64_t *out5120) {
    HP_CHECK_HIP(hipDeviceSynchronize());
    static unsigned long long tl[1024][4], gate[1024][2];
    static int role[1024];
    HP_CHECK_HIP(hipMemcpyFromSymbol(tl, HIP_SYMBOL(g_split_tl), sizeof(tl)));
    HP_CHECK_HIP(hipMemcpyFromSymbol(gate, HIP_SYMBOL(g_split_tl_gate), sizeof(gate)));
    HP_CHECK_HIP(hipMemcpyFromSymbol(role, HIP_SYMBOL(g_split_role), sizeof(role)));
    for (int b = 0; b < 1024; ++b) {
        out5120[5 * b + 0] = tl[b][0]; out5120[5 * b + 1] = tl[b][1]; out5120[5 * b + 2] = gate[b][0]; out5120[5 * b + 3] = tl[b][3];
        out5120[5 * b + 4] = (uint64_t)role[b] | (gate[b][1] << 8);   // role | gate passed << 8 (the stamps are < 2^56)
    }
    return HP_OK;
}
int hp_debug_split_entry(uint64_t *out1024) {   // wall clock at each workgroup's first instruction (before any kernel argument is read)
    HP_CHECK_HIP(hipDeviceSynchronize());
    HP_CHECK_HIP(hipMemcpyFromSymbol(out1024, HIP_SYMBOL(g_split_entry), 1024 * 8));
    return HP_OK;
}
int hp_debug_gemm_blk_timeline(uint64_t *out512) {   // [wave][block]{landed, issued} of one workgroup's product loop
    HP_CHECK_HIP(hipDeviceSynchronize());
    HP_CHECK_HIP(hipMemcpyFromSymbol(out512, HIP_SYMBOL(g_gemm_tl_blk), 8 * 32 * 2 * 8));
    return HP_OK;
}
#endif

}  // extern "C"
