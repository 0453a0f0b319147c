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
//
// A whole wave is ONE launch (k_rollout_episodes, hp_rollout_episodes) when nothing is left that needs a launch boundary per
// timestep: the environment's dynamics are device functions of the library (env_device.h) and every row draws from its own stream
// (or nothing is drawn).  Workgroup b owns rows 4b .. 4b+3 and loops over t by itself -- no cross-workgroup hand-off, no grid-wide
// wait, no host in the loop -- through the SAME device functions: the policy slab of k_policy_slab8 (s8_policy_slab), ro_explore_row
// and the noise-free branch of k_rollout_step (ro_plain_row).
//
// All waves of a call are ONE launch too (hp_rollout_waves) once the environment is reset on the device (env_device.h: reset out
// of one reset stream per environment): the same kernel loops over the waves, resets a row's environment between two episodes on
// the row's own wave, and writes every environment and every stream back once.  hp_env_reset is that reset as a launch of its own,
// for the per-step path.
//
// This unit compiles the two per-step kernels and the host side of every entry.  The whole-episode kernels and the reset are
// templates over an environment kind (rollout_episodes.h) that each kind's own unit instantiates (env_point_mass.hip,
// env_push_block.hip); the entries here reach them through the kind's row of the table below (env_kind_lookup) and know no kind by name.
#include <algorithm>

#include "rollout_episodes.h"   // ExploreArgs, ro_explore_row, PolicyArgs (slab8.h), EpisodesArgs and EnvKind
#include "demo_episodes.h"      // DemoArgs (the kernel is instantiated by the kinds' demo units, through EnvKind::launch_demo), CompactArgs
#include "policy_call.h"        // policy_args, slab_net, require_slab_shaped

struct RolloutStepArgs {
    const double *obs, *ag, *g;    // this timestep's rows [rows][dim] (g == nullptr: the closing record of row T)
    double *b_obs, *b_ag, *b_g, *b_act;   // block arrays, already offset to episode `first`
    float *pi;                     // [rows][ad]: policy outputs in, actions out
    MtState *st;
    int rows, T, t, od, gd, ad;
    int explore, record_blocks;
    ExploreArgs x;
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
        for (long long e = lane; e < (long long)A.rows * ad; e += MW_THREADS) {
            const long long i = e / ad, j = e - i * ad;
            ro_plain_element(A.x, A.pi + e, A.b_act + (i * A.T + A.t) * ad + j);
        }
        return;
    }
    MwState w(A.st, ring);
    for (int i = 0; i < A.rows; ++i) ro_explore_row(A.x, w, zs, A.pi + (long long)i * ad, A.b_act + ((long long)i * A.T + A.t) * ad);
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
    ro_explore_row(A.x, w, zs, A.pi + (long long)i * A.ad, A.b_act + ((long long)i * A.T + A.t) * A.ad);
    w.store(st);
}

static int rollout_launch(hp_rollout *ro, RolloutStepArgs &A, int t, bool per_env_streams = false) {
    rollout_arrays_at(ro, ro->first, A);
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

// A step of either stream form: the checks, the policy launch, then the draw + record launch.  `st` is the single stream's state
// (n_streams < 0) or the first of n_streams states, one per row; st_ctx is the context of its handle and `what` names that handle
// in a refusal.  st == nullptr: the caller passed no handle
static int rollout_step(const char *entry, const char *what, hp_rollout *ro, hp_agent *a, hp_norm *on, hp_norm *gn, hp_ctx *st_ctx,
                        MtState *st, int64_t n_streams, int32_t t, const double *obs_dev, const double *ag_dev, const double *g_dev,
                        int32_t explore, double noise_eps, double random_eps, double qn, double clip_abs, float *actions_f32_dev) {
    const bool per_env_streams = n_streams >= 0;
    HP_REQUIRE(ro && obs_dev && ag_dev && g_dev && actions_f32_dev, HP_ERR_INVALID, "%s: null argument", entry);
    HP_REQUIRE(!explore || st, HP_ERR_INVALID, "%s: exploration needs the %s", entry, what);
    HP_REQUIRE(!a || (on && gn), HP_ERR_INVALID, "%s: the policy needs both normalizers", entry);
    HP_SERIALISE(ro);
    HP_REQUIRE(t >= 0 && t < ro->T, HP_ERR_INVALID, "%s: t=%d outside [0, %d)", entry, t, ro->T);
    HP_REQUIRE(!st || st_ctx == ro->ctx, HP_ERR_INVALID, "%s: %s belongs to another context", entry, what);
    if (per_env_streams) {
        HP_REQUIRE(!explore || ro->rows <= n_streams, HP_ERR_INVALID, "%s: a wave of %lld environments is wider than the array of %lld streams",
                   entry, (long long)ro->rows, (long long)n_streams);
        HP_REQUIRE(ro->ad <= RO_MAX_ACT, HP_ERR_INVALID, "%s: at most %d action components", entry, RO_MAX_ACT);
    }
    HP_REQUIRE(!explore || (random_eps >= 0.0 && random_eps <= 1.0), HP_ERR_INVALID, "p < 0, p > 1 or p is NaN");
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
    A.x.ad = ro->ad;
    A.x.amax = amax;
    A.x.noise_scale = noise_eps * amax;
    A.x.random_eps = random_eps; A.x.qn = qn; A.x.clip_abs = clip_abs;
    return rollout_launch(ro, A, t, per_env_streams && explore);   // explore == 0 touches no stream: the single-stream kernel's path
}

// A call over episodes [first, first + total) of the block as launches, for either argument block (EpisodesArgs, DemoArgs).  A
// describes the whole call; it is issued as consecutive launches of at most ro->launch_cap timesteps (whole waves of n_envs
// environments, at least one), each a call of its own on the episodes, flags, streams and final states the one before it left.
// The loop sets what every launch has -- its block arrays, rows and waves -- and launch(L, live, done) adds what is the form's own
// and issues it, returning the hipError_t: live = the environments that take part in the launch at all, done = the episodes of
// the launches before it.  The same for every kind.
template <class Args, class Launch>
static int rollout_split_launches(const hp_rollout *ro, const Args &A, int64_t first, int64_t total, int64_t n_envs, int32_t *launches,
                                  Launch launch) {
    int64_t per = ro->launch_cap / (ro->T > 0 ? ro->T : 1);   // waves per launch
    if (per < 1) per = 1;
    int n = 0;
    for (int64_t done = 0; done < total; ++n) {
        const int64_t left = total - done, waves = std::min<int64_t>((left + n_envs - 1) / n_envs, per);
        const int64_t rows = std::min(left, waves * n_envs), live = std::min(rows, n_envs);
        Args L = A;
        rollout_arrays_at(ro, first + done, L);
        L.rows = (int)rows; L.waves = (int)waves;
        HP_CHECK_HIP(launch(L, live, done));
        done += rows;
    }
    if (launches) *launches = n;
    return HP_OK;
}

// The table of environment kinds: one row per kind, defined by the kind's own unit -- and the refusal of every entry for a
// descriptor whose kind has no row
static int env_kind_lookup(const char *entry, const hp_env_desc *env, const EnvKind *&kind) {
    static const EnvKind *const kinds[] = {&env_kind_point_mass, &env_kind_push_block, &env_kind_pick_place};
    kind = nullptr;
    for (const EnvKind *k : kinds)
        if (k->kind == env->kind) {
            kind = k;
            break;
        }
    HP_REQUIRE(kind, HP_ERR_INVALID, "%s: env->kind %d is not an environment kind of this build", entry, (int)env->kind);
    return HP_OK;
}

// A descriptor against its kind's row, in the order every entry refuses in: the state arrays, the block's dimensions (ro ==
// nullptr: the entry has no block), the reset on the device where the entry needs one
static int env_desc_check(const char *entry, const EnvKind *kind, const hp_env_desc *env, const hp_rollout *ro, bool needs_reset) {
    for (int k = 0; k < kind->state_arrays; ++k)
        HP_REQUIRE(env->state_dev[k], HP_ERR_INVALID, "%s: env->state_dev[%d] is null", entry, k);
    HP_REQUIRE(!ro || (ro->od == kind->obs && ro->gd == kind->goal && ro->ad == kind->act), HP_ERR_INVALID,
               "%s: env->kind %d has dimensions %d / %d / %d, the block has %d / %d / %d", entry, (int)env->kind, kind->obs, kind->goal,
               kind->act, ro ? ro->od : 0, ro ? ro->gd : 0, ro ? ro->ad : 0);
    HP_REQUIRE(!needs_reset || kind->reset_draws > 0, HP_ERR_INVALID, "%s: env->kind %d has no reset on the device", entry, (int)env->kind);
    return HP_OK;
}

// what hp_rollout_episodes and hp_rollout_waves share: the checks on agent, normalizers, block and streams, and the arguments of the
// kernel (`entry` names the caller in every refusal).  reset_streams == nullptr: one wave of ro->rows environments
static int rollout_episodes(const char *entry, hp_rollout *ro, hp_agent *a, hp_norm *on, hp_norm *gn, hp_rng_streams *streams,
                            hp_rng_streams *reset_streams, const hp_env_desc *env, int64_t n_envs, int32_t explore, double noise_eps,
                            double random_eps, double qn, double clip_abs, float *success_dev, int32_t *launches) {
    HP_REQUIRE(a->ctx == ro->ctx && on->ctx == ro->ctx && gn->ctx == ro->ctx && (!streams || streams->ctx == ro->ctx) &&
                   (!reset_streams || reset_streams->ctx == ro->ctx),
               HP_ERR_INVALID, "%s: handles belong to different contexts", entry);
    const EnvKind *kind;
    HP_TRY(env_kind_lookup(entry, env, kind));
    HP_TRY(require_slab_shaped(entry, a, HP_ERR_INVALID, ": it keeps the per-step calls"));
    HP_REQUIRE(a->cfg.act_dim == ro->ad && on->size == ro->od && gn->size == ro->gd && on->size + gn->size == a->xdim, HP_ERR_INVALID,
               "%s: agent / normalizer dimensions differ from the block's", entry);
    HP_REQUIRE(!explore || streams, HP_ERR_INVALID, "%s: explore != 0 needs `streams`", entry);
    const int64_t width = std::min<int64_t>(ro->rows, n_envs);   // the widest wave of the call
    HP_REQUIRE(!explore || width <= streams->n, HP_ERR_INVALID,
               "%s: a wave of %lld environments is wider than the array of %lld streams", entry, (long long)width,
               (long long)streams->n);
    HP_REQUIRE(!reset_streams || n_envs <= reset_streams->n, HP_ERR_INVALID,
               "%s: %lld environments, but the array holds %lld reset streams", entry, (long long)n_envs, (long long)reset_streams->n);
    HP_REQUIRE(!explore || (random_eps >= 0.0 && random_eps <= 1.0), HP_ERR_INVALID, "p < 0, p > 1 or p is NaN");
    HP_TRY(env_desc_check(entry, kind, env, ro, reset_streams != nullptr));
    EpisodesArgs A;
    memset(&A, 0, sizeof(A));
    A.P = policy_args(a, slab_net(a, false), norm_view(on), norm_view(gn), clip_or_inf(0.0), 0);   // agent_act_dev with clip_obs = 0; rows: per launch
    A.st = explore ? streams->d_state : nullptr;
    A.reset_st = reset_streams ? reset_streams->d_state : nullptr;
    A.rows = (int)ro->rows; A.T = ro->T; A.explore = explore ? 1 : 0;
    A.n_envs = (int)n_envs;
    A.waves = (int)((ro->rows + n_envs - 1) / n_envs);   // of the whole call; a launch holds at most launch_cap / T of them
    A.x.ad = ro->ad;
    A.x.amax = a->cfg.max_action;
    A.x.noise_scale = noise_eps * a->cfg.max_action;
    A.x.random_eps = random_eps; A.x.qn = qn; A.x.clip_abs = clip_abs;
    A.env = *env;
    A.success = success_dev;
    return rollout_split_launches(ro, A, ro->first, ro->rows, n_envs, launches, [&](EpisodesArgs &L, int64_t live, int64_t done) {
        L.success += done;
        L.P.rows = (int)live;              // the environments that take part in the launch at all
        return kind->launch_episodes(ro->ctx->stream, (unsigned)((live + 3) / 4), L);
    });
}

// what hp_demo_episodes and hp_demo_episodes_pick share -- everything but the type of the script: the checks (`entry` names the
// caller in every refusal), the arguments of the kernel and the split into launches.  Exactly one of push / pick is given, and
// which one says which controller the launches run (DemoArgs::controller): a value of the call, not a property of the kind
static int demo_episodes(const char *entry, hp_ctx *ctx, const hp_env_desc *env, hp_rng_streams *reset_streams, const hp_demo_script *push,
                         const hp_pick_script *pick, int64_t n_envs, int64_t first_episode, int64_t n_episodes, int32_t T,
                         hp_rollout *block, float *success_dev, float *step_success_dev, int32_t *launches_out) {
    HP_REQUIRE(ctx && env && reset_streams && (push || pick) && block && success_dev && step_success_dev, HP_ERR_INVALID,
               "%s: null argument", entry);
    CtxGuard guard(ctx);
    hp_rollout *ro = block;
    HP_REQUIRE(reset_streams->ctx == ctx && ro->ctx == ctx, HP_ERR_INVALID, "%s: handles belong to different contexts", entry);
    HP_REQUIRE(n_envs > 0 && n_envs < (1 << 24), HP_ERR_INVALID, "%s: n_envs %lld out of range", entry, (long long)n_envs);
    HP_REQUIRE(n_envs <= reset_streams->n, HP_ERR_INVALID, "%s: %lld environments, but the array holds %lld reset streams", entry,
               (long long)n_envs, (long long)reset_streams->n);
    HP_REQUIRE(first_episode >= 0 && n_episodes > 0 && first_episode + n_episodes <= ro->n, HP_ERR_INVALID,
               "%s: episodes [%lld, %lld) outside the block of %lld", entry, (long long)first_episode,
               (long long)(first_episode + n_episodes), (long long)ro->n);
    HP_REQUIRE(T == ro->T, HP_ERR_INVALID, "%s: T = %d, the block has T = %d", entry, (int)T, (int)ro->T);
    const EnvKind *kind;
    HP_TRY(env_kind_lookup(entry, env, kind));
    HP_TRY(env_desc_check(entry, kind, env, ro, true));
    const int32_t *phase_end = push ? push->phase_end : pick->phase_end;
    for (int k = 0; k < 5; ++k)
        HP_REQUIRE(phase_end[k] >= 0 && (k == 0 || phase_end[k] > phase_end[k - 1]), HP_ERR_INVALID,
                   "%s: script->phase_end[%d] = %d: the phase ends must be increasing", entry, k, (int)phase_end[k]);
    DemoArgs A;
    memset(&A, 0, sizeof(A));
    A.reset_st = reset_streams->d_state;
    A.T = ro->T; A.n_envs = (int)n_envs;
    A.controller = push ? DEMO_PUSH : DEMO_PICK;
    if (push) A.s = *push;
    else A.p = *pick;
    A.env = *env;
    return rollout_split_launches(ro, A, first_episode, n_episodes, n_envs, launches_out, [&](DemoArgs &L, int64_t live, int64_t done) {
        L.success = success_dev + done;
        L.step_success = step_success_dev + done * ro->T;
        return kind->launch_demo(ctx->stream, (unsigned)live, L);
    });
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
    return rollout_step("hp_rollout_step", "random stream", ro, a, on, gn, rng ? rng->ctx : nullptr, rng ? rng->d_state : nullptr, -1, t,
                        obs_dev, ag_dev, g_dev, explore, noise_eps, random_eps, qn, clip_abs, actions_f32_dev);
}

int hp_rollout_step_streams(hp_rollout *ro, hp_agent *a, hp_norm *on, hp_norm *gn, hp_rng_streams *streams, int32_t t,
                            const double *obs_dev, const double *ag_dev, const double *g_dev, int32_t explore, double noise_eps,
                            double random_eps, double qn, double clip_abs, float *actions_f32_dev) {
    return rollout_step("hp_rollout_step_streams", "stream array", ro, a, on, gn, streams ? streams->ctx : nullptr,
                        streams ? streams->d_state : nullptr, streams ? streams->n : 0, t, obs_dev, ag_dev, g_dev, explore, noise_eps,
                        random_eps, qn, clip_abs, actions_f32_dev);
}

int hp_rollout_episodes(hp_rollout *ro, hp_agent *a, hp_norm *on, hp_norm *gn, hp_rng_streams *streams, const hp_env_desc *env,
                        int32_t explore, double noise_eps, double random_eps, double qn, double clip_abs, float *success_dev) {
    HP_REQUIRE(ro && a && on && gn && env && success_dev, HP_ERR_INVALID, "hp_rollout_episodes: null argument");
    HP_SERIALISE(ro);
    return rollout_episodes("hp_rollout_episodes", ro, a, on, gn, streams, nullptr, env, ro->rows, explore, noise_eps, random_eps, qn,
                            clip_abs, success_dev, nullptr);
}

int hp_rollout_waves(hp_rollout *ro, hp_agent *a, hp_norm *on, hp_norm *gn, hp_rng_streams *streams, hp_rng_streams *reset_streams,
                     const hp_env_desc *env, int64_t n_envs, int32_t explore, double noise_eps, double random_eps, double qn,
                     double clip_abs, float *success_dev, int32_t *launches_out) {
    HP_REQUIRE(ro && a && on && gn && reset_streams && env && success_dev, HP_ERR_INVALID, "hp_rollout_waves: null argument");
    HP_SERIALISE(ro);
    HP_REQUIRE(n_envs > 0 && n_envs < (1 << 24), HP_ERR_INVALID, "hp_rollout_waves: n_envs %lld out of range", (long long)n_envs);
    HP_REQUIRE(ro->rows > 0 && ro->first + ro->rows <= ro->n, HP_ERR_INVALID, "hp_rollout_waves: episodes [%lld, %lld) outside the block of %lld",
               (long long)ro->first, (long long)(ro->first + ro->rows), (long long)ro->n);
    return rollout_episodes("hp_rollout_waves", ro, a, on, gn, streams, reset_streams, env, n_envs, explore, noise_eps, random_eps, qn,
                            clip_abs, success_dev, launches_out);
}

int hp_env_reset(hp_ctx *ctx, const hp_env_desc *env, hp_rng_streams *reset_streams, int64_t rows) {
    HP_REQUIRE(ctx && env && reset_streams, HP_ERR_INVALID, "hp_env_reset: null argument");
    CtxGuard guard(ctx);
    HP_REQUIRE(reset_streams->ctx == ctx, HP_ERR_INVALID, "hp_env_reset: handles belong to different contexts");
    HP_REQUIRE(rows > 0 && rows <= reset_streams->n, HP_ERR_INVALID,
               "hp_env_reset: %lld environments, but the array holds %lld reset streams", (long long)rows, (long long)reset_streams->n);
    const EnvKind *kind;
    HP_TRY(env_kind_lookup("hp_env_reset", env, kind));
    HP_TRY(env_desc_check("hp_env_reset", kind, env, nullptr, true));
    HP_CHECK_HIP(kind->launch_reset(ctx->stream, *env, reset_streams->d_state, rows));
    return HP_OK;
}

int hp_demo_episodes(hp_ctx *ctx, const hp_env_desc *env, hp_rng_streams *reset_streams, const hp_demo_script *script, int64_t n_envs,
                     int64_t first_episode, int64_t n_episodes, int32_t T, hp_rollout *block, float *success_dev, float *step_success_dev,
                     int32_t *launches_out) {
    return demo_episodes("hp_demo_episodes", ctx, env, reset_streams, script, nullptr, n_envs, first_episode, n_episodes, T, block,
                         success_dev, step_success_dev, launches_out);
}

int hp_demo_episodes_pick(hp_ctx *ctx, const hp_env_desc *env, hp_rng_streams *reset_streams, const hp_pick_script *script, int64_t n_envs,
                          int64_t first_episode, int64_t n_episodes, int32_t T, hp_rollout *block, float *success_dev,
                          float *step_success_dev, int32_t *launches_out) {
    return demo_episodes("hp_demo_episodes_pick", ctx, env, reset_streams, nullptr, script, n_envs, first_episode, n_episodes, T, block,
                         success_dev, step_success_dev, launches_out);
}

int hp_demo_compact(hp_ctx *ctx, hp_rollout *src, const float *success_dev, const float *step_success_dev, int64_t n_episodes,
                    hp_rollout *dst, float *dst_step_success_dev, int64_t n_demos, int64_t kept, int32_t *kept_dev) {
    HP_REQUIRE(ctx && src && success_dev && step_success_dev && dst && dst_step_success_dev && kept_dev, HP_ERR_INVALID,
               "hp_demo_compact: null argument");
    CtxGuard guard(ctx);
    HP_REQUIRE(src->ctx == ctx && dst->ctx == ctx, HP_ERR_INVALID, "hp_demo_compact: handles belong to different contexts");
    HP_REQUIRE(src != dst, HP_ERR_INVALID, "hp_demo_compact: source and destination are the same block");
    HP_REQUIRE(src->T == dst->T && src->od == dst->od && src->gd == dst->gd && src->ad == dst->ad, HP_ERR_INVALID,
               "hp_demo_compact: the source block has T %d and dimensions %d / %d / %d, the destination %d and %d / %d / %d", src->T,
               src->od, src->gd, src->ad, dst->T, dst->od, dst->gd, dst->ad);
    HP_REQUIRE(n_episodes > 0 && n_episodes <= src->n && n_episodes < (1 << 24), HP_ERR_INVALID,
               "hp_demo_compact: episodes [0, %lld) outside the source block of %lld", (long long)n_episodes, (long long)src->n);
    HP_REQUIRE(n_demos > 0 && n_demos <= dst->n, HP_ERR_INVALID, "hp_demo_compact: episodes [0, %lld) outside the destination block of %lld",
               (long long)n_demos, (long long)dst->n);
    HP_REQUIRE(kept >= 0 && kept <= n_demos, HP_ERR_INVALID, "hp_demo_compact: kept = %lld outside [0, %lld]", (long long)kept,
               (long long)n_demos);
    CompactArgs A;
    memset(&A, 0, sizeof(A));
    A.s_obs = src->block; A.s_ag = src->block + src->o_ag; A.s_g = src->block + src->o_g; A.s_act = src->block + src->o_act;
    A.d_obs = dst->block; A.d_ag = dst->block + dst->o_ag; A.d_g = dst->block + dst->o_g; A.d_act = dst->block + dst->o_act;
    A.success = success_dev; A.s_step = step_success_dev; A.d_step = dst_step_success_dev;
    A.n = (int)n_episodes; A.T = src->T; A.od = src->od; A.gd = src->gd; A.ad = src->ad;
    A.kept = kept; A.n_demos = n_demos;
    A.kept_out = kept_dev;
    HP_CHECK_HIP(demo_launch_compact(ctx->stream, (unsigned)n_episodes, A));
    return HP_OK;
}

int hp_rollout_debug_set_launch_cap(hp_rollout *ro, int64_t timesteps) {
    HP_REQUIRE(ro && timesteps >= 0, HP_ERR_INVALID, "hp_rollout_debug_set_launch_cap: bad argument");
    HP_SERIALISE(ro);
    ro->launch_cap = timesteps ? timesteps : HP_ROLLOUT_MAX_LAUNCH_TIMESTEPS;
    return HP_OK;
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
