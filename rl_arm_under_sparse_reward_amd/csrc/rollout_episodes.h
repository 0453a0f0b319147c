// rollout_episodes.h -- whole episodes in one launch: the kernels of hp_rollout_episodes / hp_rollout_waves and hp_env_reset as
// templates over an environment kind (env_device.h), with their argument block and LDS layout, and the table row of a kind
// (EnvKind, env_kind_entry) through which rollout.hip reaches them.
//
// Nothing is instantiated here and nothing in rollout.hip: every kind has a translation unit of its own (env_point_mass.hip,
// env_push_block.hip) that includes this file and defines the kind's row, and env_kind_entry<Env> is the one place that names the
// kernels of a kind -- so each unit compiles the policy slab's body (the bulk of its compile) exactly once.  What the kernels
// borrow comes in with this file: agent_device.h and the 4-row policy slab's device functions as namespace s8ro.
#pragma once
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wundefined-inline"   // agent_device.h declares the 32-row engine's fragment map, which no code here calls
#include "agent_device.h"
#pragma clang diagnostic pop

// the 4-row policy slab's device functions (no kernel of slab8.h is compiled by an includer of this file)
#define S8_DEVICE_ONLY
#define S8_NRG 1
#define S8_NS s8ro
#include "slab8.h"
#undef S8_NRG
#undef S8_NS
#undef S8_DEVICE_ONLY

#include "env_device.h"
#include "mt19937_wave.h"

#define RO_MAX_ACT 16

// what turns a policy output into an action: the constants of ddpg_agent._select_actions (:174-184) and of the +-0.15 clip (:118-119)
struct ExploreArgs {
    int ad;
    double noise_scale;            // noise_eps * action_max (the reference's float64 product)
    double amax, random_eps, qn, clip_abs;
};

// ddpg_agent._select_actions (:174-184) for one row, out of the stream loaded into w: randn(act), uniform(act), binomial(1).
// pi: the row's policy outputs in, its actions out (float32 [ad]); act: its place in the block (float64 [ad]); zs: ad doubles of
// LDS of this wave's own.  One wave, wave-local barriers (mt19937_wave.h).  Shared by the single-stream walk, the per-environment
// form and the whole-episode kernel, so one stream gives the same bits in all three.
__device__ __forceinline__ void ro_explore_row(const ExploreArgs &A, MwState &w, double *zs, float *pi, double *act) {
    const int lane = mw_lane(), ad = A.ad;
    const float amax = (float)A.amax, clipf = (float)A.clip_abs;
    // :177 action += noise_eps * max_action * randn(act): float32 array += float64 array, rounded once
    mw_draw_normal(w, ad, [&](long long k, double z) { zs[k] = z; });
    mw_sync();
    float a = 0.f;
    if (lane < ad) {
        a = pi[lane];
        a = (float)__dadd_rn((double)a, __dmul_rn(A.noise_scale, zs[lane]));
        a = fminf(fmaxf(a, -amax), amax);                                          // :178 np.clip in float32
    }
    mw_sync();   // zs is rewritten by the next normals
    double ra = 0.0;
    mw_draw_uniform(w, -A.amax, __dsub_rn(A.amax, -A.amax), ad, [&](int, double u) { ra = u; });   // :179-180
    const int b = mw_draw_binomial1(w, A.random_eps, A.qn);                        // :182
    if (lane < ad) {
        // :182 action += binomial * (random_actions - action), float64 arithmetic rounded to float32 once
        a = (float)__dadd_rn((double)a, __dmul_rn((double)b, __dsub_rn(ra, (double)a)));
        if (A.clip_abs > 0) a = fminf(fmaxf(a, -clipf), clipf);                    // :118-119, float32
        pi[lane] = a;
        act[lane] = (double)a;
    }
}

// ddpg_agent.collect_episodes with explore=False for one element: action = pi.astype(float64), clipped in float64 from epoch 100 on
__device__ __forceinline__ void ro_plain_element(const ExploreArgs &A, float *pi, double *act) {
    double a = (double)*pi;
    if (A.clip_abs > 0) a = fmin(fmax(a, -A.clip_abs), A.clip_abs);
    *act = a;
    *pi = (float)a;
}

// ---- whole episodes in one launch ------------------------------------------------------------------------------------------
struct EpisodesArgs {
    PolicyArgs P;                  // the policy call of hp_agent_act_dev (obs / g / x / actions unused: the rows come from LDS)
    double *b_obs, *b_ag, *b_g, *b_act;   // block arrays, already offset to episode `first`
    MtState *st;                   // exploration stream of environment 0 (explore != 0)
    MtState *reset_st;             // reset stream of environment 0; nullptr: the environments were reset by the caller
    int rows, T, explore;          // rows: episodes of the launch = waves of n_envs environments, the last one possibly partial
    int n_envs, waves;             // (hp_rollout_episodes: n_envs = rows, one wave)
    ExploreArgs x;
    hp_env_desc env;
    float *success;                // [rows]
};

// what a workgroup of k_rollout_episodes keeps beside the policy slab: one environment, one row of observations, one action row
// and -- exploring -- one MT19937 ring per row
template <class Env>
struct EpisodesLds {
    Env env[4];
    double obs[4][Env::OBS], ag[4][Env::GOAL], g[4][Env::GOAL];
    double zs[4][RO_MAX_ACT];
    float pi[4][RO_MAX_ACT];
    uint32_t ring[4][4][MT_N];
    int verdict[4];                // of a row's reset attempt, lane 0 to its wave (env_reset_run)
};

// LDS: 111552 bytes of policy slab + 39936 of rings + the rows: one workgroup per CU, which is what the policy slab's weight ring
// asks for anyway.  Wave r < 4 owns row r outside the policy slab: its lane 0 steps the environment, its lanes j < act_dim hold
// action j (s8_policy_slab's emit), and the whole wave walks the row's stream.  Barriers per timestep: one __syncthreads() behind
// observe, the policy slab's own, none in the draws (wave-local: the rejection loops of different rows need not agree on a trip count).
//
// The wave loop.  Workgroup b owns ENVIRONMENTS 4b .. 4b+3 for the whole launch (A.P.rows = the environments that take part at
// all); environment i collects episode w * n_envs + i in wave w if that is < rows, and sits the wave out otherwise (only in the
// last wave, only a suffix of the environments: the rows of a slab that take part are its first `nrows`).  Whether a row takes part
// is wave-uniform, everything it does between two episodes is wave-local, and a row that sits out still reaches every workgroup
// barrier of the timestep loop.  With reset streams a row's wave, before each of its episodes: commits the exploration stream out
// of its ring (mt_commit's rule: numpy's lazy form), loads the environment's reset stream INTO THE SAME RING (a second ring per
// row does not fit the 160 KiB four times), draws the reset (env_reset_run: a kind with RESET_ATTEMPTS > 1 goes round a
// data-dependent number of times, wave-locally -- the rows of a slab need not agree on the count, and what carries the exploration
// stream across the detour are registers the loop does not touch), commits that stream once, and loads the exploration stream
// again -- 2.5 KB read per stream and episode, and a key written only when the walk left its block.  The weight ring has drained when s8_trunk
// returns and the next s8_ring_prologue is issued after all of this, so its counted waits stay exact.  One wave and no reset stream
// is hp_rollout_episodes' launch, unchanged.
template <class Env>
__global__ __launch_bounds__(S8_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_rollout_episodes(const EpisodesArgs A) {
    __shared__ s8ro::PolicyLds L;
    __shared__ EpisodesLds<Env> E;
    constexpr int OD = Env::OBS, GD = Env::GOAL, AD = Env::ACT;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long row0 = (long long)blockIdx.x * 4;
    const int nenv = A.P.rows - row0 < 4 ? (int)(A.P.rows - row0) : 4;   // environments of this slab
    const bool mine = wave < nenv;               // this wave owns environment row0 + wave
    const long long env = row0 + wave;
    const int T = A.T;
    MwState w;
    if (mine) {
        if (lane == 0) E.env[wave].load(A.env, env);
        if (A.explore && !A.reset_st) w.load(A.st + env, E.ring[wave]);
    }
    for (int wv = 0; wv < A.waves; ++wv) {
        const long long ep0 = (long long)wv * A.n_envs + row0;               // episode of the slab's row 0 in this wave
        const int nrows = A.rows - ep0 < nenv ? (A.rows - ep0 < 0 ? 0 : (int)(A.rows - ep0)) : nenv;
        const bool part = wave < nrows;          // this wave's environment collects episode ep0 + wave
        const long long row = ep0 + wave;
        if constexpr (Env::RESET_DRAWS > 0) {
            if (A.reset_st && part) {
                // what the exploration stream's commit writes from lane 0 stays in registers across the detour, so the reload
                // depends on no other lane's global store: each lane reads back only the key words it wrote itself
                const bool resume = A.explore && wv > 0;
                long long xblock = 0;
                int xpos = 0, xhas = 0;
                double xgauss = 0.0;
                if (resume) {
                    mt_final_block(w.g.cursor, xblock, xpos);
                    xhas = w.has_gauss;
                    xgauss = w.gauss;
                    w.store(A.st + env);
                    mw_sync();                   // the commit has read the ring before the next stream's key overwrites it
                }
                w.load(A.reset_st + env, E.ring[wave]);
                env_reset_run<Env>(w, E.env[wave], E.zs[wave], &E.verdict[wave]);   // as many attempts as this row needs
                w.store(A.reset_st + env);
                mw_sync();
                if (A.explore) w.load(A.st + env, E.ring[wave]);
                if (resume) {
                    w.g.cursor = xpos;
                    w.has_gauss = xhas;
                    w.gauss = xgauss;
                }
            }
        }
        // record the rows observed into E at timestep t (t == T: the closing record, no goal row)
        auto record = [&](int t) {
            const int per = OD + GD + (t < T ? GD : 0);
            for (int e = tid; e < nrows * per; e += S8_THREADS) {
                const int r = e / per, c = e - r * per;
                const long long i = ep0 + r;
                if (c < OD) A.b_obs[(i * (T + 1) + t) * OD + c] = E.obs[r][c];
                else if (c < OD + GD) A.b_ag[(i * (T + 1) + t) * GD + (c - OD)] = E.ag[r][c - OD];
                else A.b_g[(i * T + t) * GD + (c - OD - GD)] = E.g[r][c - OD - GD];
            }
        };
        for (int t = 0; t < T; ++t) {
            if (part && lane == 0) E.env[wave].observe(E.obs[wave], E.ag[wave], E.g[wave]);
            __syncthreads();
            record(t);
            s8ro::s8_policy_slab(A.P, L, (size_t)row0,
                [&](int r, int c) -> float {
                    if (r >= nrows) return 0.f;  // an environment that sits this wave out
                    if (c < OD) return tr_net_input(E.obs[r][c], A.P.clip_obs, A.P.onz->mean[c], A.P.onz->std[c], A.P.clip_o);
                    const int j = c - OD;
                    return tr_net_input(E.g[r][j], A.P.clip_obs, A.P.gnz->mean[j], A.P.gnz->std[j], A.P.clip_g);
                },
                [&](int r, int j, float a) { E.pi[r][j] = a; });
            if (part) {
                mw_sync();
                double *act = A.b_act + (row * T + t) * AD;
                if (A.explore) ro_explore_row(A.x, w, E.zs[wave], E.pi[wave], act);
                else if (lane < AD) ro_plain_element(A.x, &E.pi[wave][lane], act + lane);
                mw_sync();
                if (lane == 0) E.env[wave].step(E.pi[wave]);
            }
        }
        if (part && lane == 0) E.env[wave].observe(E.obs[wave], E.ag[wave], E.g[wave]);
        __syncthreads();
        record(T);
        if (part && lane == 0) A.success[row] = E.env[wave].is_success() ? 1.f : 0.f;
        if (wv + 1 < A.waves) __syncthreads();   // record(T) has read the rows the next wave's first observe rewrites
    }
    if (mine) {
        if (lane == 0) E.env[wave].store(A.env, env);
        if (A.explore) w.store(A.st + env);
    }
}

// A reset as a launch of its own (hp_env_reset): workgroup i = one wave = environment i, like k_rollout_step_streams -- load reset
// stream i, draw (every attempt the kind's reset needs), commit it by mt_commit's rule, and lane 0 writes the fresh state.
template <class Env>
__global__ __launch_bounds__(MW_THREADS) void k_env_reset(const hp_env_desc env, MtState *reset_st) {
    __shared__ uint32_t ring[4][MT_N];
    __shared__ double u[Env::RESET_DRAWS > 0 ? Env::RESET_DRAWS : 1];
    __shared__ int verdict;
    if constexpr (Env::RESET_DRAWS > 0) {
        const long long i = blockIdx.x;
        MtState *st = reset_st + i;
        MwState w(st, ring);
        Env e;
        if (mw_lane() == 0) e.load(env, i);      // the parameters; the state it reads is replaced
        env_reset_run<Env>(w, e, u, &verdict);
        w.store(st);
        if (mw_lane() == 0) e.store(env, i);
    }
}

// ---- the table of kinds ------------------------------------------------------------------------------------------------------
// What the host side of rollout.hip knows of a kind: its constant, what it compares with the block and the descriptor before any
// launch, and how to launch its three kernels.  launch_episodes issues one launch of k_rollout_episodes over `blocks` workgroups with
// the arguments of that launch (the split by the launch cap stays in rollout.hip), launch_reset one of k_env_reset over `rows`
// environments, launch_demo one of k_demo_episodes (demo_episodes.h: scripted episodes, no policy) over `blocks` environments;
// each returns the launch's hipError_t.  The third kernel is compiled by a unit of its own (demo_<kind>.hip), which this file
// names only by the launch function's declaration.
struct DemoArgs;                                 // demo_episodes.h
template <class Env> hipError_t env_launch_demo(hipStream_t stream, unsigned blocks, const DemoArgs &L);   // defined there too

struct EnvKind {
    int kind, obs, goal, act, state_arrays, reset_draws;
    hipError_t (*launch_episodes)(hipStream_t stream, unsigned blocks, const EpisodesArgs &L);
    hipError_t (*launch_reset)(hipStream_t stream, const hp_env_desc &env, MtState *reset_st, int64_t rows);
    hipError_t (*launch_demo)(hipStream_t stream, unsigned blocks, const DemoArgs &L);
};

// The row of kind `kind` = the struct Env of env_device.h: what a kind must be for these kernels, and the kernels' instantiation
// (in the one unit that calls this for Env).
template <class Env>
EnvKind env_kind_entry(int kind) {
    static_assert(Env::ACT <= 4 && Env::ACT <= RO_MAX_ACT && Env::OBS + Env::GOAL <= S8_LDX, "an environment of the policy slab's shape");
    static_assert(Env::RESET_DRAWS <= RO_MAX_ACT, "the reset's values pass through the row's zs");
    static_assert(Env::STATE_ARRAYS >= 1 && Env::STATE_ARRAYS <= 4, "hp_env_desc has four state arrays");
    return EnvKind{kind, Env::OBS, Env::GOAL, Env::ACT, Env::STATE_ARRAYS, Env::RESET_DRAWS,
                   [](hipStream_t stream, unsigned blocks, const EpisodesArgs &L) {
                       hipLaunchKernelGGL(k_rollout_episodes<Env>, dim3(blocks), dim3(S8_THREADS), 0, stream, L);
                       return hipGetLastError();
                   },
                   [](hipStream_t stream, const hp_env_desc &env, MtState *reset_st, int64_t rows) {
                       hipLaunchKernelGGL(k_env_reset<Env>, dim3((unsigned)rows), dim3(MW_THREADS), 0, stream, env, reset_st);
                       return hipGetLastError();
                   },
                   &env_launch_demo<Env>};
}

// the rows, one per unit (the table itself: env_kind_lookup() in rollout.hip)
extern const EnvKind env_kind_point_mass;   // env_point_mass.hip
extern const EnvKind env_kind_push_block;   // env_push_block.hip
extern const EnvKind env_kind_pick_place;   // env_pick_place.hip
