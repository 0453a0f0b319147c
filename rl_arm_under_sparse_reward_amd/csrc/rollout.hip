// rollout.hip -- the experience half of a cycle on the device (ddpg_agent.py:101-137 for a vectorised simulator whose state
// already lives in device memory): no host copy and no host wait per timestep.
//
// A wave block holds n episodes in the staging layout of hp_buffer_store_pinned / feeder._Layout,
//     [obs n x (T+1) x obs_dim | ag n x (T+1) x goal_dim | g n x T x goal_dim | actions n x T x act_dim]   (float64),
// so a finished wave is stored and trained on by hp_buffer_store_dev / hp_agent_train_cycle_dev with one device-to-device copy.
//
// One timestep is TWO launches:
//   1. the policy kernel (k_policy_slab8, the kernel of hp_agent_act, reading the simulator's rows in place), one 4-row slab per
//      workgroup across the chip;
//   2. k_rollout_step: workgroup 0 is the one wave that walks the exploration draws of ddpg_agent._select_actions (:174-184) in
//      the host's order -- for env i = 0 .. n-1: randn(act), uniform(act), binomial(1) -- out of the reference's MT19937 stream
//      (mt19937_wave.h) and writes the actions; the other workgroups record obs / ag / g of this timestep into the block.
// They stay two because they have opposite shapes: the policy is wide (every row independent) and the draw is one sequential
// walk whose word count is data dependent; folded into one launch the walk would either wait behind a grid-wide hand-off inside
// the kernel or run once per workgroup.  Recording rides along with the walk for free.
#include "agent.h"
#include "mt19937_wave.h"

#define RO_MAX_ACT 16

struct hp_rollout {
    hp_ctx *ctx = nullptr;
    int64_t n = 0;                 // episodes the block holds
    int32_t T = 0, od = 0, gd = 0, ad = 0;
    int64_t first = 0, rows = 0;   // the wave being collected: episodes [first, first + rows)
    double action_max = 1.0;       // of the policy whose outputs a teacher-forced step is handed (hp_rollout_set_action_max)
    double *block = nullptr;
    int64_t o_ag = 0, o_g = 0, o_act = 0, elems = 0;   // offsets in float64 elements (feeder._Layout)
};

struct RolloutStepArgs {
    const double *obs, *ag, *g;    // this timestep's rows [rows][dim] (g == nullptr: the closing record of row T)
    double *b_obs, *b_ag, *b_g, *b_act;   // block arrays, already offset to episode `first`
    float *pi;                     // [rows][ad]: policy outputs in, actions out
    MtState *st;
    int rows, T, t, od, gd, ad;
    int explore, record_blocks;
    double noise_scale;            // noise_eps * action_max (the reference's float64 product)
    double amax, random_eps, qn, clip_abs;
};

// element e of this timestep's rows -> its place in the block
__device__ __forceinline__ void ro_record(const RolloutStepArgs &A, long long e0, long long stride) {
    const long long n_o = (long long)A.rows * A.od, n_g = (long long)A.rows * A.gd;
    const long long total = n_o + n_g + (A.g ? n_g : 0);
    for (long long e = e0; e < total; e += stride) {
        if (e < n_o) {
            const long long i = e / A.od, c = e - i * A.od;
            A.b_obs[(i * (A.T + 1) + A.t) * A.od + c] = A.obs[e];
        } else if (e < n_o + n_g) {
            const long long k = e - n_o, i = k / A.gd, c = k - i * A.gd;
            A.b_ag[(i * (A.T + 1) + A.t) * A.gd + c] = A.ag[k];
        } else {
            const long long k = e - n_o - n_g, i = k / A.gd, c = k - i * A.gd;
            A.b_g[(i * A.T + A.t) * A.gd + c] = A.g[k];
        }
    }
}

// ddpg_agent._select_actions (:174-184) for row i of the wave, out of the stream loaded into w: randn(act), uniform(act),
// binomial(1).  Shared by the single-stream walk and the per-environment form, so one stream gives the same bits in both.
__device__ __forceinline__ void ro_explore_row(const RolloutStepArgs &A, MwState &w, double *zs, int i) {
    const int lane = threadIdx.x, ad = A.ad;
    const float amax = (float)A.amax, clipf = (float)A.clip_abs;
    // :177 action += noise_eps * max_action * randn(act): float32 array += float64 array, rounded once
    mw_draw_normal(w, ad, [&](long long k, double z) { zs[k] = z; });
    __syncthreads();
    float a = 0.f;
    if (lane < ad) {
        a = A.pi[(long long)i * ad + lane];
        a = (float)__dadd_rn((double)a, __dmul_rn(A.noise_scale, zs[lane]));
        a = fminf(fmaxf(a, -amax), amax);                                          // :178 np.clip in float32
    }
    __syncthreads();   // zs is rewritten by the next environment's normals
    double ra = 0.0;
    mw_draw_uniform(w, -A.amax, __dsub_rn(A.amax, -A.amax), ad, [&](int, double u) { ra = u; });   // :179-180
    const int b = mw_draw_binomial1(w, A.random_eps, A.qn);                        // :182
    if (lane < ad) {
        // :182 action += binomial * (random_actions - action), float64 arithmetic rounded to float32 once
        a = (float)__dadd_rn((double)a, __dmul_rn((double)b, __dsub_rn(ra, (double)a)));
        if (A.clip_abs > 0) a = fminf(fmaxf(a, -clipf), clipf);                    // :118-119, float32
        A.pi[(long long)i * ad + lane] = a;
        A.b_act[((long long)i * A.T + A.t) * ad + lane] = (double)a;
    }
}

__global__ __launch_bounds__(MW_THREADS) void k_rollout_step(const RolloutStepArgs A) {
    __shared__ uint32_t ring[4][MT_N];
    __shared__ double zs[RO_MAX_ACT];
    const int lane = threadIdx.x;
    if (blockIdx.x > 0) {
        ro_record(A, (long long)(blockIdx.x - 1) * MW_THREADS + lane, (long long)A.record_blocks * MW_THREADS);
        return;
    }
    if (!A.pi) return;   // closing record only
    const int ad = A.ad;
    if (!A.explore) {
        // ddpg_agent.collect_episodes with explore=False: action = pi.astype(float64), clipped in float64 from epoch 100 on
        for (long long e = lane; e < (long long)A.rows * ad; e += MW_THREADS) {
            double a = (double)A.pi[e];
            if (A.clip_abs > 0) a = fmin(fmax(a, -A.clip_abs), A.clip_abs);
            const long long i = e / ad, j = e - i * ad;
            A.b_act[(i * A.T + A.t) * ad + j] = a;
            A.pi[e] = (float)a;
        }
        return;
    }
    MwState w(A.st, ring);
    for (int i = 0; i < A.rows; ++i) ro_explore_row(A, w, zs, i);
    w.store(A.st);
}

// The same step with one stream per environment (hp_rollout_step_streams): workgroup i < rows is the one wave that draws row i's
// exploration out of stream i -- the draws of ro_explore_row, the code of the single-stream walk, on an LDS ring of its own --
// and the workgroups behind them record the rows.  No wave loops over environments: the grid grows with the active rows, and
// a partial wave leaves the streams behind it alone.  State traffic per environment and step: the key is read (2.5 KB); what is
// written back is pos and the cached normal (16 bytes) unless the walk ended in a block generated here (mt_commit's rule), which
// for 4 action components (about 20 words a step) is one step in thirty -- only then is the key rewritten.
__global__ __launch_bounds__(MW_THREADS) void k_rollout_step_streams(const RolloutStepArgs A) {
    __shared__ uint32_t ring[4][MT_N];
    __shared__ double zs[RO_MAX_ACT];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= A.rows) {
        ro_record(A, (long long)((int)blockIdx.x - A.rows) * MW_THREADS + lane, (long long)A.record_blocks * MW_THREADS);
        return;
    }
    const int i = blockIdx.x;
    MtState *st = A.st + i;
    MwState w(st, ring);
    ro_explore_row(A, w, zs, i);
    w.store(st);
}

static int rollout_launch(hp_rollout *ro, RolloutStepArgs &A, int t, bool per_env_streams = false) {
    A.b_obs = ro->block + ro->first * (ro->T + 1) * ro->od;
    A.b_ag = ro->block + ro->o_ag + ro->first * (ro->T + 1) * ro->gd;
    A.b_g = ro->block + ro->o_g + ro->first * ro->T * ro->gd;
    A.b_act = ro->block + ro->o_act + ro->first * ro->T * ro->ad;
    A.rows = (int)ro->rows; A.T = ro->T; A.t = t; A.od = ro->od; A.gd = ro->gd; A.ad = ro->ad;
    const long long elems = ro->rows * (ro->od + 2 * ro->gd);
    long long nb = (elems + 4 * MW_THREADS - 1) / (4 * MW_THREADS);   // four elements per thread
    A.record_blocks = (int)(nb < 1 ? 1 : (nb > 2048 ? 2048 : nb));
    if (per_env_streams)
        hipLaunchKernelGGL(k_rollout_step_streams, dim3(A.rows + A.record_blocks), dim3(MW_THREADS), 0, ro->ctx->stream, A);
    else
        hipLaunchKernelGGL(k_rollout_step, dim3(1 + A.record_blocks), dim3(MW_THREADS), 0, ro->ctx->stream, A);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

// the part of a step both stream forms share: the policy launch, then the draw + record launch.  `st` is the single stream's state
// or -- per_env_streams -- the first of one state per row
static int rollout_step(const char *entry, hp_rollout *ro, hp_agent *a, hp_norm *on, hp_norm *gn, MtState *st, bool per_env_streams, int32_t t,
                        const double *obs_dev, const double *ag_dev, const double *g_dev, int32_t explore, double noise_eps,
                        double random_eps, double qn, double clip_abs, float *actions_f32_dev) {
    double amax = ro->action_max;
    if (a) {   // a == NULL: actions_f32_dev already holds the policy outputs (teacher-forced tests)
        HP_REQUIRE(a->ctx == ro->ctx && on->ctx == ro->ctx && gn->ctx == ro->ctx, HP_ERR_INVALID,
                   "%s: handles belong to different contexts", entry);
        HP_REQUIRE(a->cfg.act_dim == ro->ad && on->size == ro->od && gn->size == ro->gd, HP_ERR_INVALID,
                   "%s: agent / normalizer dimensions differ from the block's", entry);
        HP_TRY(agent_act_dev(a, on, gn, HP_NET_ACTOR, obs_dev, g_dev, ro->rows, 0.0, actions_f32_dev));
        amax = a->cfg.max_action;
    }
    RolloutStepArgs A;
    memset(&A, 0, sizeof(A));
    A.obs = obs_dev; A.ag = ag_dev; A.g = g_dev;
    A.pi = actions_f32_dev;
    A.st = st;
    A.explore = explore ? 1 : 0;
    A.amax = amax;
    A.noise_scale = noise_eps * amax;
    A.random_eps = random_eps; A.qn = qn; A.clip_abs = clip_abs;
    return rollout_launch(ro, A, t, per_env_streams && explore);   // explore == 0 touches no stream: the single-stream kernel's path
}

extern "C" {

int hp_rollout_create(hp_ctx *ctx, hp_buffer *buf, int64_t n_envs, hp_rollout **out) {
    HP_REQUIRE(ctx && buf && out, HP_ERR_INVALID, "hp_rollout_create: null argument");
    HP_REQUIRE(buf->ctx == ctx, HP_ERR_INVALID, "hp_rollout_create: buffer belongs to another context");
    HP_REQUIRE(n_envs > 0 && n_envs < (1 << 24), HP_ERR_INVALID, "hp_rollout_create: n_envs out of range");
    HP_REQUIRE(buf->act_dim <= RO_MAX_ACT, HP_ERR_INVALID, "hp_rollout_create: at most %d action components", RO_MAX_ACT);
    CtxGuard guard(ctx);
    hp_rollout *ro = new hp_rollout();
    ro->ctx = ctx; ro->n = n_envs; ro->T = buf->T; ro->od = buf->obs_dim; ro->gd = buf->goal_dim; ro->ad = buf->act_dim;
    ro->first = 0; ro->rows = n_envs;
    ro->o_ag = n_envs * (int64_t)buf->ep_obs();
    ro->o_g = ro->o_ag + n_envs * (int64_t)buf->ep_ag();
    ro->o_act = ro->o_g + n_envs * (int64_t)buf->ep_g();
    ro->elems = ro->o_act + n_envs * (int64_t)buf->ep_act();
    hipError_t e = hipMalloc((void **)&ro->block, (size_t)ro->elems * 8);
    if (e == hipSuccess) e = hipMemsetAsync(ro->block, 0, (size_t)ro->elems * 8, ctx->stream);
    if (e != hipSuccess) {
        hp_set_error("hp_rollout_create: device allocation failed: %s", hipGetErrorString(e));
        if (ro->block) (void)hipFree(ro->block);
        delete ro;
        return HP_ERR_HIP;
    }
    *out = ro;
    return HP_OK;
}

int hp_rollout_begin(hp_rollout *ro, int64_t first_episode, int64_t n_rows) {
    HP_REQUIRE(ro, HP_ERR_INVALID, "hp_rollout_begin: null handle");
    HP_SERIALISE(ro);
    HP_REQUIRE(first_episode >= 0 && n_rows > 0 && first_episode + n_rows <= ro->n, HP_ERR_INVALID,
               "hp_rollout_begin: episodes [%lld, %lld) outside the block of %lld", (long long)first_episode,
               (long long)(first_episode + n_rows), (long long)ro->n);
    ro->first = first_episode;
    ro->rows = n_rows;
    return HP_OK;
}

int hp_rollout_block(hp_rollout *ro, void **block_dev, int64_t *n_episodes, int64_t *offsets4, int64_t *elems) {
    HP_REQUIRE(ro && block_dev, HP_ERR_INVALID, "hp_rollout_block: null argument");
    *block_dev = ro->block;
    if (n_episodes) *n_episodes = ro->n;
    if (offsets4) { offsets4[0] = 0; offsets4[1] = ro->o_ag; offsets4[2] = ro->o_g; offsets4[3] = ro->o_act; }
    if (elems) *elems = ro->elems;
    return HP_OK;
}

int hp_rollout_step(hp_rollout *ro, hp_agent *a, hp_norm *on, hp_norm *gn, hp_rng *rng, int32_t t, const double *obs_dev,
                    const double *ag_dev, const double *g_dev, int32_t explore, double noise_eps, double random_eps, double qn,
                    double clip_abs, float *actions_f32_dev) {
    HP_REQUIRE(ro && obs_dev && ag_dev && g_dev && actions_f32_dev, HP_ERR_INVALID, "hp_rollout_step: null argument");
    HP_REQUIRE(!explore || rng, HP_ERR_INVALID, "hp_rollout_step: exploration needs the random stream");
    HP_REQUIRE(!a || (on && gn), HP_ERR_INVALID, "hp_rollout_step: the policy needs both normalizers");
    HP_SERIALISE(ro);
    HP_REQUIRE(t >= 0 && t < ro->T, HP_ERR_INVALID, "hp_rollout_step: t=%d outside [0, %d)", t, ro->T);
    HP_REQUIRE(!rng || rng->ctx == ro->ctx, HP_ERR_INVALID, "hp_rollout_step: random stream belongs to another context");
    HP_REQUIRE(!explore || (random_eps >= 0.0 && random_eps <= 1.0), HP_ERR_INVALID, "p < 0, p > 1 or p is NaN");
    return rollout_step("hp_rollout_step", ro, a, on, gn, rng ? rng->d_state : nullptr, false, t, obs_dev, ag_dev, g_dev, explore, noise_eps, random_eps, qn,
                        clip_abs, actions_f32_dev);
}

int hp_rollout_step_streams(hp_rollout *ro, hp_agent *a, hp_norm *on, hp_norm *gn, hp_rng_streams *streams, int32_t t,
                            const double *obs_dev, const double *ag_dev, const double *g_dev, int32_t explore, double noise_eps,
                            double random_eps, double qn, double clip_abs, float *actions_f32_dev) {
    HP_REQUIRE(ro && obs_dev && ag_dev && g_dev && actions_f32_dev, HP_ERR_INVALID, "hp_rollout_step_streams: null argument");
    HP_REQUIRE(!explore || streams, HP_ERR_INVALID, "hp_rollout_step_streams: exploration needs the stream array");
    HP_REQUIRE(!a || (on && gn), HP_ERR_INVALID, "hp_rollout_step_streams: the policy needs both normalizers");
    HP_SERIALISE(ro);
    HP_REQUIRE(t >= 0 && t < ro->T, HP_ERR_INVALID, "hp_rollout_step_streams: t=%d outside [0, %d)", t, ro->T);
    HP_REQUIRE(!streams || streams->ctx == ro->ctx, HP_ERR_INVALID, "hp_rollout_step_streams: stream array belongs to another context");
    HP_REQUIRE(!explore || ro->rows <= streams->n, HP_ERR_INVALID,
               "hp_rollout_step_streams: a wave of %lld environments is wider than the array of %lld streams", (long long)ro->rows,
               (long long)streams->n);
    HP_REQUIRE(ro->ad <= RO_MAX_ACT, HP_ERR_INVALID, "hp_rollout_step_streams: at most %d action components", RO_MAX_ACT);
    HP_REQUIRE(!explore || (random_eps >= 0.0 && random_eps <= 1.0), HP_ERR_INVALID, "p < 0, p > 1 or p is NaN");
    return rollout_step("hp_rollout_step_streams", ro, a, on, gn, streams ? streams->d_state : nullptr, true, t, obs_dev, ag_dev, g_dev, explore, noise_eps,
                        random_eps, qn, clip_abs, actions_f32_dev);
}

int hp_rollout_set_action_max(hp_rollout *ro, double action_max) {
    HP_REQUIRE(ro && action_max > 0, HP_ERR_INVALID, "hp_rollout_set_action_max: bad argument");
    HP_SERIALISE(ro);
    ro->action_max = action_max;
    return HP_OK;
}

int hp_rollout_finish(hp_rollout *ro, const double *obs_dev, const double *ag_dev) {
    HP_REQUIRE(ro && obs_dev && ag_dev, HP_ERR_INVALID, "hp_rollout_finish: null argument");
    HP_SERIALISE(ro);
    RolloutStepArgs A;
    memset(&A, 0, sizeof(A));
    A.obs = obs_dev; A.ag = ag_dev;
    return rollout_launch(ro, A, ro->T);
}

int hp_rollout_read(hp_rollout *ro, int32_t which, double *host_out) {
    HP_REQUIRE(ro && host_out, HP_ERR_INVALID, "hp_rollout_read: null argument");
    HP_SERIALISE(ro);
    HP_REQUIRE(which >= 0 && which < 4, HP_ERR_INVALID, "hp_rollout_read: which must be 0 (obs), 1 (ag), 2 (g) or 3 (actions)");
    const int64_t off[5] = {0, ro->o_ag, ro->o_g, ro->o_act, ro->elems};
    HP_CHECK_HIP(hipMemcpyAsync(host_out, ro->block + off[which], (size_t)(off[which + 1] - off[which]) * 8, hipMemcpyDeviceToHost,
                                ro->ctx->stream));
    HP_CHECK_HIP(hipStreamSynchronize(ro->ctx->stream));
    return HP_OK;
}

void hp_rollout_destroy(hp_rollout *ro) {
    if (!ro) return;
    if (ro->block) (void)hipFree(ro->block);
    delete ro;
}

}  // extern "C"
